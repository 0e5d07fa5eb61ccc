"""Time the 16-bit pair-distance kernels (fedagg_pairgram2_16,
fedagg_pairdist2_16; csrc/robust16.hip) beside the fp32 Gram on the widened
copy of the same rows (tool only).

    python tools/pairgram16_probe.py [--out FILE] [--cols N] [--iters I]

Shapes: --cols columns (default 4,194,304), K = 128 and the padded K = 100,
bf16 and f16 rows of the "base + small update" kind (P = 1 planes a stage for
bf16, 2 for f16), and one bf16 run at K = 128 whose elements carry scattered
exponents (x * 2^randint(-12, 12): every stage needs P = 3).  Per shape the
16-bit Gram, the 16-bit exact kernel, the fp32 Gram and the fp32 exact kernel
(the last two on the widened copy; the fp32 exact kernel is the 16-bit one's
code built WITH packed fp32 operations, so the pair prices their absence from
robust16.hip's build) are launched in turn on the same rows, --iters times
(default 10) after a warm-up round, each call between two device events; the median of each with its min and max, the
ratios, the largest |gram - exact| / exact, and whether the Gram wins by
defense.py's rule (its median below the exact kernel's by more than the larger
min-max spread of the two).  "auto" lists, per dtype, whether K = 128 and
K = 100 both win, against the 16-bit exact kernel and against the fp32 one
as well: PAIRGRAM16_AUTO's entries.  Writes
profiles/pairgram16_probe.json.
"""
from __future__ import annotations

import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = ((torch.bfloat16, 128, "close"), (torch.bfloat16, 100, "close"), (torch.float16, 128, "close"),
        (torch.float16, 100, "close"), (torch.bfloat16, 128, "scattered"))


def make_rows(dev, K: int, N: int, dtype, kind: str, seed: int = 0):
    """16-bit rows (a common base 0.05 randn plus 0.01 randn per client, row by
    row) and their exactly widened fp32 copy, with the pointer tables."""
    rows = torch.empty((K, N), dtype=dtype, device=dev)
    wide = torch.empty((K, N), dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    base = 0.05 * torch.randn(N, generator=g, device=dev)
    for i in range(K):
        x = base + 0.01 * torch.randn(N, generator=g, device=dev)
        if kind == "scattered":
            x = x * torch.exp2(torch.randint(-12, 13, (N,), generator=g, device=dev).float())
        rows[i] = x.to(dtype)
        wide[i] = rows[i].float()
    ptr = lambda t: kn.upload_i64([t[i].data_ptr() for i in range(K)], dev)
    return rows, wide, ptr(rows), ptr(wide)


def _event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts) -> dict:
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def time_run(dev, dtype, K: int, N: int, kind: str, iters: int) -> dict:
    rows, wide, p16, p32 = make_rows(dev, K, N, dtype, kind)
    st = np.arange(0, N, nat.PAIR_CHUNK, dtype=np.int64)
    tab = np.stack([st, np.minimum(nat.PAIR_CHUNK, N - st)], axis=1).ravel()
    chunks, n = kn.upload_i64(tab.tolist(), dev), len(st)
    res = {}
    legs = {"gram16": lambda: res.__setitem__("g", dfn.pairdist2_rows(p16, K, chunks, n, dev, "gram", dtype=dtype)),
            "exact16": lambda: res.__setitem__("e", dfn.pairdist2_rows(p16, K, chunks, n, dev, "exact", dtype=dtype)),
            "gram32": lambda: dfn.pairdist2_rows(p32, K, chunks, n, dev, "gram"),
            "exact32": lambda: dfn.pairdist2_rows(p32, K, chunks, n, dev, "exact")}
    ts = {k: [] for k in legs}
    for it in range(iters + 1):  # round 0 warms every leg up
        for name, fn in legs.items():
            ms = _event_ms(fn)
            if it:
                ts[name].append(ms)
    g, e, f, x = (_stats(ts[k]) for k in ("gram16", "exact16", "gram32", "exact32"))
    spread = max(g["max_ms"] - g["min_ms"], e["max_ms"] - e["min_ms"])
    spread32 = max(g["max_ms"] - g["min_ms"], x["max_ms"] - x["min_ms"])
    Dg, De = res["g"].cpu().numpy(), res["e"].cpu().numpy()
    off = ~np.eye(K, dtype=bool)
    r = {"dtype": str(dtype).replace("torch.", ""), "K": K, "N": N, "rows": kind, "iters": iters,
         "gram16": g, "exact16": e, "gram32_on_widened_rows": f, "exact32_on_widened_rows": x,
         "exact16_over_exact32": round(e["median_ms"] / x["median_ms"], 2),
         "gram16_wins_over_exact32": bool(x["median_ms"] - g["median_ms"] > spread32),
         "exact16_over_gram16": round(e["median_ms"] / g["median_ms"], 2),
         "gram32_over_gram16": round(f["median_ms"] / g["median_ms"], 2),
         "median_gap_ms": round(e["median_ms"] - g["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "gram16_wins": bool(e["median_ms"] - g["median_ms"] > spread),
         "rows_GB": round(K * N * 2 / 1e9, 3), "gram16_row_TBps": round(K * N * 2 / g["median_ms"] / 1e9, 2),
         "max_rel_diff": float((np.abs(Dg - De)[off] / De[off]).max()), "condition": dfn.gram_condition(Dg)}
    print(r, flush=True)
    return r


def main(argv) -> int:
    opt = {"--out": os.path.join(ROOT, "profiles", "pairgram16_probe.json"), "--cols": "4194304", "--iters": "10"}
    for i in range(0, len(argv), 2):
        if argv[i] not in opt or i + 1 >= len(argv):
            raise SystemExit(__doc__)
        opt[argv[i]] = argv[i + 1]
    if not torch.cuda.is_available():
        raise SystemExit("pairgram16_probe: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    rs = []
    for dtype, K, kind in RUNS:
        rs.append(time_run(dev, dtype, K, int(opt["--cols"]), kind, int(opt["--iters"])))
        torch.cuda.empty_cache()
    auto = {d: all(r["gram16_wins"] and r["gram16_wins_over_exact32"]
                   for r in rs if r["dtype"] == d and r["rows"] == "close")
            for d in ("bfloat16", "float16")}
    out = {"device": torch.cuda.get_device_name(0), "timings": rs, "auto": auto}
    os.makedirs(os.path.dirname(opt["--out"]), exist_ok=True)
    with open(opt["--out"], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("auto:", auto, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
