"""Check and time the nearest-to-median mean kernel of "wise_bulyan" (tool only).

    python tools/bulyan_probe.py [--out FILE]   # default: profiles/bulyan_probe.json

First a few shapes bit for bit against the torch path
(fedml_amd.defense.nearmedian_mean_rows_torch).  Then, in one process and on
the same rows, fedagg_nearmedian_mean_f32 and fedagg_trimmed_mean launched
alternately at 25,610,152 fp32 columns (config 3) for K = 128, 96, 64, 32 rows:
keep = K - 2f for a small and a near-maximal f and keep = K / 2, the trimmed
mean at the trim that keeps the same count; median of 10 and the min-max
spread of each.  Last one whole bulyan() call at config 3's size (128 clients,
f = 10) and the same call stage by stage (ingest, distances, selection on the
host, window kernel): for the record, not a gate.  --quick: one tenth of the
columns.
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402

HBM_TBPS = 8.0
RUNS = 10


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    nan = torch.isnan(b)
    return bool(torch.equal(torch.isnan(a), nan) and ((a.view(torch.int32) == b.view(torch.int32)) | nan).all())


def check(dev) -> list:
    res = []
    g = torch.Generator(device=dev).manual_seed(1)
    for K, keep, N in ((5, 3, 1000), (33, 17, 4099), (100, 80, 70_001), (128, 88, 262_144), (128, 4, 262_144)):
        rows = 0.05 * torch.randn((K, N), generator=g, device=dev)
        rows[:, ::5] = torch.round(rows[:, ::5] * 40) / 40  # ties
        rows[0, ::97] = float("nan")
        rows[1, ::89] = float("inf")
        rows[2, ::83] = -float("inf")
        out = torch.empty(N, dtype=torch.float32, device=dev)
        ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
        dfn.nearmedian_mean_rows(ptrs, K, N, keep, out)
        ok = same(out, dfn.nearmedian_mean_rows_torch(rows, keep))
        res.append({"K": K, "keep": keep, "N": N, "bit_identical": ok})
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


def keeps(K: int) -> list:
    """(label, keep): K rows are Bulyan's theta, so K + 2f >= 4f + 3 bounds f by (K - 3) // 2."""
    return [("f=2", K - 4), (f"f={(K - 3) // 2}", K - 2 * ((K - 3) // 2)), ("K/2", K // 2)]


def headline(rows, K: int, N: int, label: str, keep: int, dev) -> dict:
    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    out = torch.empty(rows.shape[1], dtype=torch.float32, device=dev)
    trim = (K - keep) // 2
    assert K - 2 * trim == keep
    tn, tt = timed_pair(lambda: dfn.nearmedian_mean_rows(ptrs, K, N, keep, out),
                        lambda: dfn.trimmed_mean_rows(ptrs, K, N, trim, out, aligned=True))
    n, t = stats(tn), stats(tt)
    nbytes = K * N * 4
    r = {"K": K, "N": N, "case": label, "keep": keep, "trim": trim, "nearmedian": n, "trimmed_mean": t,
         "ratio_to_trimmed_mean": round(n["median_ms"] / t["median_ms"], 3),
         "larger_spread_ms": round(max(n["max_ms"] - n["min_ms"], t["max_ms"] - t["min_ms"]), 4),
         "nearmedian_rows_TBps": round(nbytes / n["median_ms"] / 1e9, 3),
         "nearmedian_hbm_fraction": round(nbytes / n["median_ms"] / 1e9 / HBM_TBPS, 3)}
    print(r, flush=True)
    return r


def whole_call(rows, K: int, N: int, f: int, dev) -> dict:
    """One whole bulyan() call over K device dicts of N columns (f of them
    replaced by 1e4 randn first, so stage 1 has something to reject), wall
    time from the call to the synchronised result; then the same work stage by
    stage, each synchronised.  A plain call before the timed ones warms the
    allocator."""
    gen = torch.Generator(device=dev).manual_seed(3)
    corrupted = list(range(5, K, 11))[:f]
    for i in corrupted:
        rows[i] = 1e4 * torch.randn(rows.shape[1], generator=gen, device=dev)
    raw = [(1, OrderedDict(w=rows[i, :N])) for i in range(K)]
    dfn.bulyan(raw, f)
    out = {"f": f, "theta": K - 2 * f, "beta": K - 4 * f, "corrupted_clients": corrupted}
    for method in ("auto", "exact"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = dfn.bulyan(raw, f, method=method, return_info=True)
        torch.cuda.synchronize()
        out[method] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 2),
                       "corrupted_selected": sorted(set(info.selected) & set(corrupted))}
        print(method, out[method], flush=True)

    def lap(t0):
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 2), time.perf_counter()

    stages = {}
    torch.cuda.synchronize()
    t = time.perf_counter()
    bucket, _ = dfn._float_bucket(raw[0][1], K, "wise_bulyan", dev)
    for i, (_, d) in enumerate(raw):
        dfn._put_float(bucket, i, d, ["w"])
    bucket.sync_ingest()
    g = bucket.groups[torch.float32]
    stages["ingest_ms"], t = lap(t)
    chunks, n_chunks = dfn.weight_chunks(g, nat.PAIR_CHUNK, dev)
    D = dfn.pairdist2_rows(g.d_ptrs, K, chunks, n_chunks, dev, "auto").cpu().numpy()
    stages["distances_auto_ms"], t = lap(t)
    selected, _ = dfn.bulyan_select(D, f)
    stages["selection_host_ms"], t = lap(t)
    ptrs = kn.upload_i64([g.rows[i].data_ptr() for i in selected], dev)
    row = torch.zeros(g.padded, dtype=torch.float32, device=dev)
    dfn.nearmedian_mean_rows(ptrs, K - 2 * f, g.length, K - 4 * f, row)
    stages["window_kernel_ms"], t = lap(t)
    out["stages"] = stages
    print(stages, flush=True)
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
    for K in (128, 96, 64, 32):
        for label, keep in keeps(K):
            summary["timings"].append(headline(rows, K, N, label, keep, dev))
    if "--no-call" not in sys.argv:
        summary["bulyan_call"] = {"K": 128, "N": N, **whole_call(rows, 128, N, 10, dev)}
    summary["all_bit_identical"] = all(c["bit_identical"] for c in summary["checks"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "bulyan_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps([{k: t[k] for k in ("K", "case", "keep", "ratio_to_trimmed_mean")} for t in summary["timings"]]))
    return 0 if summary["all_bit_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
