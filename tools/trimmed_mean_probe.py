"""Check and time the coordinate-wise trimmed mean kernel (tool only).

    python tools/trimmed_mean_probe.py [--out FILE]   # default: profiles/trimmed_mean_probe.json

First a few shapes bit for bit against the torch path
(fedml_amd.defense.trimmed_mean_rows_torch), then the two headline shapes,
128 clients x 25,610,152 fp32 (config 3) and 128 clients x 86.6M bf16, with
fedagg_median timed at the same shapes in the same process as the yardstick.
Prints ms, TB/s of rows read and the fraction of 8 TB/s.  --quick: one tenth
of the columns.
"""
from __future__ import annotations

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402

HBM_TBPS = 8.0


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    nan = torch.isnan(b)
    return bool(torch.equal(torch.isnan(a), nan) and ((a.view(it) == b.view(it)) | nan).all())


def check(dev) -> list:
    res = []
    g = torch.Generator(device=dev).manual_seed(1)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for K, trim, N in ((5, 1, 1000), (33, 8, 4099), (100, 10, 70_001), (128, 12, 262_144)):
            rows = (0.05 * torch.randn((K, N), generator=g, device=dev)).to(dt)
            rows[0, ::97] = float("nan")
            rows[1, ::89] = float("inf")
            rows[2, ::83] = -float("inf")
            out = torch.empty(N, dtype=dt, device=dev)
            ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
            dfn.trimmed_mean_rows(ptrs, K, N, trim, out)
            ok = same(out, dfn.trimmed_mean_rows_torch(rows, trim))
            res.append({"dtype": str(dt), "K": K, "trim": trim, "N": N, "bit_identical": ok})
            print(res[-1], flush=True)
    return res


def timed(fn, iters: int = 10, warmup: int = 2) -> float:
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def headline(dev, dt, K: int, N: int, trim: int) -> dict:
    L = (N + 63) // 64 * 64
    rows = torch.empty((K, L), dtype=dt, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for i in range(K):  # row by row: no K x L fp32 temporary
        rows[i] = (0.05 * torch.randn(L, generator=g, device=dev)).to(dt)
    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    out = torch.empty(L, dtype=dt, device=dev)
    t_trim = timed(lambda: dfn.trimmed_mean_rows(ptrs, K, N, trim, out, aligned=True))
    t_med = timed(lambda: dfn.median_rows(ptrs, K, N, out, aligned=True))
    nbytes = K * N * rows.element_size()
    r = {"dtype": str(dt), "K": K, "N": N, "trim": trim, "trimmed_mean_ms": round(t_trim, 4),
         "median_ms": round(t_med, 4), "ratio_to_median": round(t_trim / t_med, 3),
         "trimmed_mean_TBps": round(nbytes / t_trim / 1e9, 3),
         "trimmed_mean_hbm_fraction": round(nbytes / t_trim / 1e9 / HBM_TBPS, 3),
         "median_TBps": round(nbytes / t_med / 1e9, 3)}
    print(r, flush=True)
    return r


def main():
    dev = torch.device("cuda:0")
    scale = 10 if "--quick" in sys.argv else 1
    summary = {"device": torch.cuda.get_device_name(dev), "checks": check(dev), "timings": []}
    summary["timings"].append(headline(dev, torch.float32, 128, 25_610_152 // scale, 12))
    torch.cuda.empty_cache()
    summary["timings"].append(headline(dev, torch.bfloat16, 128, 86_600_000 // scale, 12))
    summary["all_bit_identical"] = all(c["bit_identical"] for c in summary["checks"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "trimmed_mean_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary["timings"], indent=1))
    return 0 if summary["all_bit_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
