"""Check and time the fused Weiszfeld step of the "geomed" defense (tool only).

    python tools/geomed_probe.py [--out FILE] [--quick]   # default: profiles/geomed_probe.json

First a few shapes of fedagg_wsum_dist2_f32 against the unfused pair
(fedml_amd.defense.weiszfeld_step_unfused: fedagg_wsum_f32, then
fedagg_dist2_f32 with the sum as reference): z bit for bit, D to 1e-12
relative.  Then, at config 3's row length (25,610,152 fp32) and every K tier
of the kernel (8, 16, 32, 64, 128 clients), the fused step against the
unfused pair, alternating in the same process, 12 runs of each after warm-up:
median, min and max, the ratio, TB/s of rows read once and the fraction of
8 TB/s.  fedagg_median at 128 clients is the one-lane-per-column yardstick.
Last, the wall time and the iteration count of one whole geometric_median
call over 128 device dicts of that size.

The decision rule of defense.GEOMED_AUTO_FUSED is evaluated per K: the fused
kernel wins where its median time beats the unfused pair's by more than the
larger of the two min-max spreads.  --quick: one tenth of the columns.
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time
import types
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402

HBM_TBPS = 8.0
RUNS = 12


def table_for(segs, dev):
    g = types.SimpleNamespace(keys=[f"k{j}.weight" for j in range(len(segs))], offsets=[o for o, _ in segs],
                              numels=[n for _, n in segs])
    return dfn.weight_chunks(g, nat.DIST_CHUNK, dev)


def check(dev) -> list:
    res = []
    gen = torch.Generator(device=dev).manual_seed(1)
    for K, segs in ((3, [(0, 1000)]), (9, [(1, 63), (70, 4099)]), (33, [(4, 1025), (1040, 70_001)]),
                    (100, [(0, 262_144)]), (128, [(3, 65), (128, 200_000)])):
        L = (segs[-1][0] + segs[-1][1] + 127) // 64 * 64
        rows = 0.05 * torch.randn((K, L), generator=gen, device=dev)
        w = torch.rand(K, generator=gen, device=dev) + 0.1
        w = w / w.sum()
        ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
        chunks, n_chunks = table_for(segs, dev)
        z1 = torch.zeros(L, dtype=torch.float32, device=dev)
        z2 = torch.zeros(L, dtype=torch.float32, device=dev)
        D1 = dfn.wsum_dist2_rows(ptrs, w, K, chunks, n_chunks, z1, dev)
        D2 = dfn.weiszfeld_step_unfused(ptrs, w, K, L, chunks, n_chunks, z2, dev, aligned=True)
        cols = torch.cat([torch.arange(o, o + n, device=dev) for o, n in segs])
        same = bool(torch.equal(z1[cols].view(torch.int32), z2[cols].view(torch.int32)))
        rel = float(((D1 - D2).abs() / D2).max())
        res.append({"K": K, "segments": segs, "z_bit_identical": same, "D_max_rel_diff": rel,
                    "ok": same and rel <= 1e-12})
        print(res[-1], flush=True)
    return res


def timed_pair(fa, fb, runs: int = RUNS, warmup: int = 2):
    """fa and fb alternating; -> two lists of milliseconds."""
    for _ in range(warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(runs):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return ta, tb


def stats(ts) -> dict:
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def headline(rows, K: int, N: int, dev) -> dict:
    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    chunks, n_chunks = table_for([(0, N)], dev)
    w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
    z = torch.zeros(rows.shape[1], dtype=torch.float32, device=dev)
    tf, tu = timed_pair(lambda: dfn.wsum_dist2_rows(ptrs, w, K, chunks, n_chunks, z, dev),
                        lambda: dfn.weiszfeld_step_unfused(ptrs, w, K, N, chunks, n_chunks, z, dev, aligned=True))
    f, u = stats(tf), stats(tu)
    nbytes = K * N * 4
    spread = max(f["max_ms"] - f["min_ms"], u["max_ms"] - u["min_ms"])
    r = {"K": K, "N": N, "fused": f, "unfused": u, "unfused_over_fused": round(u["median_ms"] / f["median_ms"], 3),
         "bytes_bound_ratio": round((2 * K + 3) / (K + 1), 3),
         "fused_rows_TBps": round(nbytes / f["median_ms"] / 1e9, 3),
         "fused_hbm_fraction": round(nbytes / f["median_ms"] / 1e9 / HBM_TBPS, 3),
         "unfused_rows_TBps": round(2 * nbytes / u["median_ms"] / 1e9, 3),
         "larger_spread_ms": round(spread, 4),
         "fused_wins": bool(u["median_ms"] - f["median_ms"] > spread)}
    print(r, flush=True)
    return r


def whole_call(rows, K: int, N: int, dev) -> dict:
    """One whole geometric_median call over K device dicts of N columns with
    the default nu / maxiter / ftol, per method: wall time from the call to
    the synchronised result (ingest into the bucket, every pass with its
    K-double copy to the host, the output dict) and the iteration count.  12
    of the clients are replaced by 1e4 randn first, so the loop has something
    to reject; a plain call before the timed ones warms the allocator."""
    gen = torch.Generator(device=dev).manual_seed(3)
    corrupted = list(range(5, K, 11))[:12]
    for i in corrupted:
        rows[i] = 1e4 * torch.randn(rows.shape[1], generator=gen, device=dev)
    counts = [int(v) for v in np.random.default_rng(0).integers(50, 150, K)]
    raw = [(counts[i], OrderedDict(w=rows[i, :N])) for i in range(K)]
    dfn.geometric_median(raw, maxiter=0, method="unfused")
    out = {"corrupted_clients": len(corrupted)}
    for method in ("fused", "unfused", "auto"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = dfn.geometric_median(raw, method=method, return_info=True)
        torch.cuda.synchronize()
        out[method] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 2), "ran": info.method,
                       "iterations": info.iterations, "passes": info.iterations + 1,
                       "corrupted_weight": float(sum(info.weights[corrupted]))}
        print(method, out[method], flush=True)
    return out


def main():
    dev = torch.device("cuda:0")
    scale = 10 if "--quick" in sys.argv else 1
    N = 25_610_152 // scale
    L = (N + 63) // 64 * 64
    summary = {"device": torch.cuda.get_device_name(dev), "checks": check(dev), "runs_each": RUNS, "timings": []}
    rows = torch.empty((128, L), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.randn(L, generator=gen, device=dev)
    for i in range(128):  # honest clients around a common point: row by row, no 128 x L temporary
        rows[i] = base + 0.05 * torch.randn(L, generator=gen, device=dev)
    for K in (128, 64, 32, 16, 8):
        summary["timings"].append(headline(rows, K, N, dev))
    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(128)], dev)
    out = torch.empty(L, dtype=torch.float32, device=dev)
    tm, _ = timed_pair(lambda: dfn.median_rows(ptrs, 128, N, out, aligned=True), lambda: None)
    summary["median_yardstick"] = {"K": 128, "N": N, **stats(tm)}
    print(summary["median_yardstick"], flush=True)
    summary["geometric_median_call"] = {"K": 128, "N": N, **whole_call(rows, 128, N, dev)}
    summary["auto_fused_by_rule"] = {str(t["K"]): t["fused_wins"] for t in summary["timings"]}
    summary["auto_fused_shipped"] = {str(k): v for k, v in dfn.GEOMED_AUTO_FUSED.items()}
    summary["all_checks_ok"] = all(c["ok"] for c in summary["checks"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "geomed_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary["auto_fused_by_rule"]))
    return 0 if summary["all_checks_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
