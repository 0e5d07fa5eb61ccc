"""Time the 16-bit fused Weiszfeld step against the fp32 one (tool only).

    python tools/geomed16_probe.py [--out FILE] [--quick]   # default: profiles/geomed16_probe.json

At config 3's row length (25,610,152 columns), for bf16 and f16 rows, for K at
every full tier of the kernel (8, 16, 32, 64, 128) and at one padded K per tier
(6, 12, 24, 48, 100): fedagg_wsum_dist2_16 on the 16-bit rows against
fedagg_wsum_dist2_f32 on the widened copy of the same rows, launched
alternately in the same process, median of 10 after warm-up, min and max.  z is
compared bit for bit and D to 1e-12 relative at every shape timed.  The one-off
widening of the round (K rows .float()) is timed separately: it is what the
widened path pays once and the 16-bit path never.

The decision rule of defense.GEOMED16_AUTO is evaluated per dtype and tier: an
entry is True only where the fp32 pass's median exceeds the 16-bit pass's by
more than the larger of the two min-max spreads, at the full K and at the
padded K.  --quick: one tenth of the columns.
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402

RUNS = 10
TIERS = {8: 6, 16: 12, 32: 24, 64: 48, 128: 100}  # tier -> its padded K


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


def one(rows16, rows32, K: int, N: int, chunks, n_chunks, dev) -> dict:
    p16 = kn.upload_i64([rows16[i].data_ptr() for i in range(K)], dev)
    p32 = kn.upload_i64([rows32[i].data_ptr() for i in range(K)], dev)
    w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
    z16 = torch.zeros(rows32.shape[1], dtype=torch.float32, device=dev)
    z32 = torch.zeros_like(z16)
    D16 = dfn.wsum_dist2_rows(p16, w, K, chunks, n_chunks, z16, dev, dtype=rows16.dtype)
    D32 = dfn.wsum_dist2_rows(p32, w, K, chunks, n_chunks, z32, dev)
    same = bool(torch.equal(z16[:N].view(torch.int32), z32[:N].view(torch.int32)))
    rel = float(((D16 - D32).abs() / D32).max())
    t16, t32 = timed_pair(lambda: dfn.wsum_dist2_rows(p16, w, K, chunks, n_chunks, z16, dev, dtype=rows16.dtype),
                          lambda: dfn.wsum_dist2_rows(p32, w, K, chunks, n_chunks, z32, dev))
    a, b = stats(t16), stats(t32)
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    r = {"K": K, "N": N, "rows16": a, "rows32": b, "fp32_over_16": round(b["median_ms"] / a["median_ms"], 3),
         "rows16_TBps": round(K * N * 2 / a["median_ms"] / 1e9, 3), "rows32_TBps": round(K * N * 4 / b["median_ms"] / 1e9, 3),
         "gap_ms": round(b["median_ms"] - a["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "wins": bool(b["median_ms"] - a["median_ms"] > spread), "z_bit_identical": same, "D_max_rel_diff": rel,
         "ok": same and rel <= 1e-12}
    print(str(rows16.dtype), r, flush=True)
    return r


def main():
    dev = torch.device("cuda:0")
    N = 25_610_152 // (10 if "--quick" in sys.argv else 1)
    L = (N + 63) // 64 * 64
    g = types.SimpleNamespace(keys=["k.weight"], offsets=[0], numels=[N])
    chunks, n_chunks = dfn.weight_chunks(g, nat.DIST_CHUNK, dev)
    summary = {"device": torch.cuda.get_device_name(dev), "columns": N, "runs_each": RUNS, "dtypes": {}}
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.randn(L, generator=gen, device=dev)
    for dt in (torch.bfloat16, torch.float16):
        rows16 = torch.empty((128, L), dtype=dt, device=dev)
        for i in range(128):  # honest clients around a common point: row by row, no 128 x L fp32 temporary
            rows16[i] = (base + 0.05 * torch.randn(L, generator=gen, device=dev)).to(dt)
        rows32 = torch.empty((128, L), dtype=torch.float32, device=dev)
        tw, _ = timed_pair(lambda: rows32.copy_(rows16), lambda: None)  # the widened path's one-off copy, 128 rows
        res = {"widen_128_rows": stats(tw), "timings": []}
        print(str(dt), "widen", res["widen_128_rows"], flush=True)
        for tier, padded in TIERS.items():
            for K in (tier, padded):
                res["timings"].append(one(rows16, rows32, K, N, chunks, n_chunks, dev))
        res["auto_by_rule"] = {str(t): all(r["wins"] for r in res["timings"] if r["K"] in (t, p))
                               for t, p in TIERS.items()}
        res["auto_shipped"] = {str(t): v for t, v in dfn.GEOMED16_AUTO[dt].items()}
        summary["dtypes"][str(dt)] = res
        del rows16, rows32
    summary["all_checks_ok"] = all(r["ok"] for d in summary["dtypes"].values() for r in d["timings"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "geomed16_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps({k: v["auto_by_rule"] for k, v in summary["dtypes"].items()}))
    return 0 if summary["all_checks_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
