"""Time the 16-bit wide Gram (fedagg_pairgram2_wide_16, csrc/pairgram_wide16.hip;
pairdist2_rows' "gram_wide" on bf16 / f16 rows) against the 16-bit exact kernel
that "auto" ran above 128 clients before it, and beside the fp32 wide Gram on
the widened copy of the same rows (tool only).

    python tools/pairgram_wide16_probe.py [--out FILE] [--cols N] [--iters I] [--ks 256,200,...]

Shapes: --cols columns (default 4,194,304) of "base + small update" rows in
bf16 and f16 (P = 1 plane a stage for bf16, 2 for f16), K = 256 / 200,
512 / 384 and 1024 / 700 (a tier's full and padded K), and one bf16 run at
K = 512 whose elements carry scattered exponents (x * 2^randint(-12, 12): every
stage needs P = 3), which shows what the plane count is worth.  Per shape three
paths are launched in turn on the same rows, --iters times (default 10) after
a warm-up round, each call between two device events:

  exact16  fedagg_pairdist2_16: the baseline;
  wide16   the new kernel INCLUDING its centre pass (client_mean_row in the
           rows' dtype);
  wide32   fedagg_pairgram2_wide_f32 with its centre pass, on the widened fp32
           copy: for the record only.

The median of each with its min and max, the ratios, the largest
|wide16 - exact16| / exact16, and whether wide16 wins by defense.py's rule (its
median below exact16's by more than the larger min-max spread of the two).
"tiers" lists per dtype whether a tier's two K values both win:
PAIRGRAM_WIDE16_AUTO's entries.  Writes profiles/pairgram_wide16_probe.json.
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
TIERS = ((256, 256, 200), (512, 512, 384), (1024, 1024, 700))
SCATTERED_K = 512
DTYPES = (torch.bfloat16, torch.float16)


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
    ptr = lambda t: kn.upload_i64([t[i].data_ptr() for i in range(K)], dev)  # noqa: E731
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
    legs = {"exact16": lambda: res.__setitem__("e", dfn.pairdist2_rows(p16, K, chunks, n, dev, "exact", dtype=dtype)),
            "wide16": lambda: res.__setitem__("w", dfn.pairdist2_rows(p16, K, chunks, n, dev, "gram_wide", length=N,
                                                                      aligned=True, dtype=dtype)),
            "centre16": lambda: dfn.client_mean_row(p16, K, N, dev, True, dtype),
            "wide32": lambda: dfn.pairdist2_rows(p32, K, chunks, n, dev, "gram_wide", length=N, aligned=True)}
    ts = {k: [] for k in legs}
    for it in range(iters + 1):  # round 0 warms every leg up
        for name, fn in legs.items():
            ms = _event_ms(fn)
            if it:
                ts[name].append(ms)
    e, w, c, f = (_stats(ts[k]) for k in ("exact16", "wide16", "centre16", "wide32"))
    spread = max(w["max_ms"] - w["min_ms"], e["max_ms"] - e["min_ms"])
    Dw, De = res["w"].cpu().numpy(), res["e"].cpu().numpy()
    off = ~np.eye(K, dtype=bool)
    r = {"dtype": str(dtype).replace("torch.", ""), "K": K, "N": N, "rows": kind, "iters": iters,
         "exact16": e, "wide16_with_centre_pass": w, "centre16_alone": c, "wide32_with_centre_pass_on_widened_rows": f,
         "exact16_over_wide16": round(e["median_ms"] / w["median_ms"], 2),
         "wide32_over_wide16": round(f["median_ms"] / w["median_ms"], 2),
         "median_gap_ms": round(e["median_ms"] - w["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "wide16_wins": bool(e["median_ms"] - w["median_ms"] > spread),
         "wide16_beats_wide32": bool(f["median_ms"] - w["median_ms"] >
                                     max(w["max_ms"] - w["min_ms"], f["max_ms"] - f["min_ms"])),
         "rows_GB": round(K * N * 2 / 1e9, 3),
         "max_rel_diff": float((np.abs(Dw - De)[off] / De[off]).max()), "condition": dfn.gram_condition(Dw)}
    print(r, flush=True)
    return r


def main(argv) -> int:
    opt = {"--out": os.path.join(ROOT, "profiles", "pairgram_wide16_probe.json"), "--cols": "4194304", "--iters": "10",
           "--ks": ",".join(str(k) for t in TIERS for k in t[1:])}
    for i in range(0, len(argv), 2):
        if argv[i] not in opt or i + 1 >= len(argv):
            raise SystemExit(__doc__)
        opt[argv[i]] = argv[i + 1]
    if not torch.cuda.is_available():
        raise SystemExit("pairgram_wide16_probe: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    cols, iters, ks = int(opt["--cols"]), int(opt["--iters"]), [int(k) for k in opt["--ks"].split(",")]
    runs = [(dt, K, "close") for dt in DTYPES for K in ks] + [(torch.bfloat16, SCATTERED_K, "scattered")]
    rs = []
    for dtype, K, kind in runs:
        rs.append(time_run(dev, dtype, K, cols, kind, iters))
        torch.cuda.empty_cache()
    won = {(r["dtype"], r["K"]): r["wide16_wins"] for r in rs if r["rows"] == "close"}
    # a tier whose two K values were not both measured stays False
    tiers = {d: {str(t): bool(won.get((d, full), False) and won.get((d, padded), False)) for t, full, padded in TIERS}
             for d in ("bfloat16", "float16")}
    out = {"device": torch.cuda.get_device_name(0), "timings": rs, "tiers": tiers}
    os.makedirs(os.path.dirname(opt["--out"]), exist_ok=True)
    with open(opt["--out"], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("tiers:", tiers, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
