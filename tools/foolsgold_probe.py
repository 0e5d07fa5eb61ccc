"""Time one round's history update and Gram of the "foolsgold_cos" defense:
the fused kernel (fedagg_histgram_f32, csrc/histgram.hip) beside the composed
path (the torch history update, pairdist2_rows "auto" about a zero centre and
dist2_rows: defense.histgram_rows_composed) (tool only).

    python tools/foolsgold_probe.py --k K [--out FILE] [--cols N] [--iters I]

One run times one K (128, and the padded 100) at --cols fp32 columns (default
4,194,304) of "base + small update" rows and gaussian histories, so a job can
bound each K with its own time limit; the result joins the others in
profiles/foolsgold_probe.json.  The two paths are launched alternately on the
same rows, --iters times (default 10) after a warm-up round, each between two
device events; the histories are restored from a saved copy before every
launch (outside the timed span), so both paths see the same values.  Recorded:
the median of each with its min and max, the fused kernel's achieved bytes per
second against its 3 K N 4-byte model, the largest cosine difference between
the two Grams, and whether the fused kernel wins by defense.py's rule (the
composed median above the fused one by more than the larger min-max spread).
"auto" is HISTGRAM_AUTO's entry: True only if every K measured so far wins and
both K = 128 and K = 100 are there.
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


def _event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts) -> dict:
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def time_run(dev, K: int, N: int, iters: int) -> dict:
    g = torch.Generator(device=dev).manual_seed(K)
    ref = 0.05 * torch.randn(N, generator=g, device=dev)
    rows = torch.empty((K, N), dtype=torch.float32, device=dev)
    hist0 = torch.empty((K, N), dtype=torch.float32, device=dev)
    for i in range(K):
        rows[i] = ref + 0.01 * torch.randn(N, generator=g, device=dev)
        hist0[i] = 0.02 * torch.randn(N, generator=g, device=dev)
    hist = hist0.clone()
    zero = torch.zeros(N, dtype=torch.float32, device=dev)
    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    hptrs = kn.upload_i64([hist[i].data_ptr() for i in range(K)], dev)
    st = np.arange(0, N, nat.PAIR_CHUNK, dtype=np.int64)
    tab = np.stack([st, np.minimum(nat.PAIR_CHUNK, N - st)], axis=1).ravel()
    chunks, n = kn.upload_i64(tab.tolist(), dev), len(st)
    res = {}
    legs = {"fused": lambda: res.__setitem__("f", dfn.histgram_rows(ptrs, K, ref, hptrs, chunks, n, dev)),
            "composed": lambda: res.__setitem__("c", dfn.histgram_rows_composed(rows, ref, hist, None, hptrs, K,
                                                                               [(0, N)], chunks, n, dev, zero))}
    ts = {k: [] for k in legs}
    for it in range(iters + 1):  # round 0 warms both legs up
        for name, fn in legs.items():
            hist.copy_(hist0)
            ms = _event_ms(fn)
            if it:
                ts[name].append(ms)
    f, c = _stats(ts["fused"]), _stats(ts["composed"])
    spread = max(f["max_ms"] - f["min_ms"], c["max_ms"] - c["min_ms"])
    Gf, Gc = res["f"].cpu().numpy(), res["c"].cpu().numpy()
    nrm = np.sqrt(np.outer(np.diag(Gc), np.diag(Gc)))
    r = {"K": K, "N": N, "iters": iters, "fused": f, "composed": c,
         "composed_over_fused": round(c["median_ms"] / f["median_ms"], 2),
         "median_gap_ms": round(c["median_ms"] - f["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "fused_wins": bool(c["median_ms"] - f["median_ms"] > spread),
         "model_GB": round(3 * K * N * 4 / 1e9, 3), "fused_model_TBps": round(3 * K * N * 4 / f["median_ms"] / 1e9, 2),
         "max_cosine_diff": float((np.abs(Gf - Gc) / nrm).max())}
    print(r, flush=True)
    return r


def main(argv) -> int:
    opt = {"--out": os.path.join(ROOT, "profiles", "foolsgold_probe.json"), "--cols": "4194304", "--iters": "10",
           "--k": None}
    for i in range(0, len(argv), 2):
        if argv[i] not in opt or i + 1 >= len(argv):
            raise SystemExit(__doc__)
        opt[argv[i]] = argv[i + 1]
    if opt["--k"] is None:
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("foolsgold_probe: no GPU (nothing is measured without one)")
    r = time_run(torch.device("cuda", 0), int(opt["--k"]), int(opt["--cols"]), int(opt["--iters"]))
    rs = []
    if os.path.exists(opt["--out"]):
        with open(opt["--out"]) as f:
            rs = [t for t in json.load(f)["timings"] if (t["K"], t["N"]) != (r["K"], r["N"])]
    rs = sorted(rs + [r], key=lambda t: -t["K"])
    auto = {"128": bool({128, 100} <= {t["K"] for t in rs} and all(t["fused_wins"] for t in rs))}
    os.makedirs(os.path.dirname(opt["--out"]), exist_ok=True)
    with open(opt["--out"], "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "timings": rs, "auto": auto}, f, indent=1)
        f.write("\n")
    print("auto:", auto, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
