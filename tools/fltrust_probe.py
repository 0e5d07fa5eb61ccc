"""Check and time the two kernels of the "fltrust" defense (tool only).

    python tools/fltrust_probe.py --step build            # no GPU: the two batch builds of dotnorm2_kernel
    python tools/fltrust_probe.py --step check [--out F]  # default: profiles/fltrust_probe.json
    python tools/fltrust_probe.py --step time [--out F] [--quick]

build: csrc/robust.hip compiled twice more, with -DFEDAGG_DOTNORM_BATCH=8 and
=16 (the clients a wave of dotnorm2_kernel holds per pass), each linked with
the product's other objects into tools/_build/libfedagg_dotnorm_b<B>.so.  Run
it where the compiler is; the other steps only load the libraries.

check: a few shapes of fedagg_dotnorm2_f32 (the product library and both batch
builds) against defense.dotnorm2_rows_torch within n 2^-52 sum|terms|, and of
fedagg_wsum_diff_f32 against defense.wsum_diff_rows_torch bit for bit.

time: at config 3's row (25,610,152 fp32 columns) for K = 128, 32 and 512
clients, each pair launched alternately on the same rows, 10 runs of each
after warm-up, median with min - max:
  dotnorm2 against ONE fedagg_dist2_f32 launch (the same bytes: the floor) and
      against TWO (what a caller without it needs for a dot product);
  fedagg_wsum_diff_f32 over K rows and the reference against fedagg_wsum_f32
      over K + 1 rows (the same bytes);
  the 8-client build of dotnorm2_kernel against the 16-client build.
Each step adds its part to the JSON.  tools/gpu_fltrust_probe.sh runs check
and time on a GPU box, each under its own time limit.  --quick: a tenth of
the columns.
"""
from __future__ import annotations

import ctypes
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import build as fbuild  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tools", "_build")
BATCHES = (8, 16)
HBM_TBPS = 8.0
RUNS = 10
ROBUST = os.path.join(fbuild.HERE, "csrc", "robust.hip")


def variant_path(batch: int) -> str:
    return os.path.join(OUT_DIR, f"libfedagg_dotnorm_b{batch}.so")


def build_variants() -> list:
    fbuild.build()  # the product's other objects, which the variants link with
    os.makedirs(OUT_DIR, exist_ok=True)
    others = [fbuild._obj(s) for s in fbuild.SRCS if s != ROBUST]
    outs = []
    for b in BATCHES:
        obj = os.path.join(OUT_DIR, f"robust_dotnorm_b{b}.o")
        subprocess.run([fbuild.hipcc(), *fbuild.HIPCC_FLAGS, f"-DFEDAGG_DOTNORM_BATCH={b}", "-c", "-o", obj, ROBUST],
                       check=True)
        subprocess.run([fbuild.hipcc(), f"--offload-arch={fbuild.ARCH}", "-shared", "-fPIC", "-o", variant_path(b),
                        obj, *others], check=True)
        outs.append(variant_path(b))
    return outs


def load_variant(batch: int) -> ctypes.CDLL:
    path = variant_path(batch)
    if not os.path.exists(path):
        raise nat.FedAggNativeError(f"{path} not found: python tools/fltrust_probe.py --step build")
    handle = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in nat.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


def table_for(segs, dev):
    from fedml_amd import defense as dfn

    g = types.SimpleNamespace(keys=[f"k{j}.weight" for j in range(len(segs))], offsets=[o for o, _ in segs],
                              numels=[n for _, n in segs])
    return dfn.weight_chunks(g, nat.DIST_CHUNK, dev)


def dotnorm2_with(lib, ptrs, K, ref, direction, chunks, n_chunks, out, work):
    rc = lib.fedagg_dotnorm2_f32(ptrs.data_ptr(), K, ref.data_ptr(), direction.data_ptr(), chunks.data_ptr(),
                                 n_chunks, out.data_ptr(), work.data_ptr(), work.numel(), nat.stream_handle())
    if rc != 0:
        raise nat.FedAggNativeError(f"dotnorm2 (rc={rc}): {lib.fedagg_last_error().decode(errors='replace')}")


def check(dev) -> list:
    import torch

    from fedml_amd import defense as dfn
    from fedml_amd import kernels as kn

    libs = {"product": nat.lib(), **{f"batch{b}": load_variant(b) for b in BATCHES}}
    res = []
    gen = torch.Generator(device=dev).manual_seed(1)
    for K, segs in ((3, [(0, 1000)]), (9, [(1, 63), (70, 4099)]), (33, [(4, 1025), (1040, 70_001)]),
                    (130, [(3, 65), (128, 200_000)])):
        L = (segs[-1][0] + segs[-1][1] + 127) // 64 * 64
        g = 0.05 * torch.randn(L, generator=gen, device=dev)
        b = 0.01 * torch.randn(L, generator=gen, device=dev)
        rows = g + b + 0.01 * torch.randn((K, L), generator=gen, device=dev)
        rows[K - 1] = g + b  # the root as the last row
        ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
        chunks, n_chunks = table_for(segs, dev)
        cols = torch.cat([torch.arange(o, o + n, device=dev) for o, n in segs])
        wd, wn = dfn.dotnorm2_rows_torch(rows, g, rows[K - 1], cols)
        a = (rows[:, cols] - g[cols]).double()
        mag = (a * (rows[K - 1][cols] - g[cols]).double()).abs().sum(dim=1)
        tol = len(cols) * 2.0 ** -52
        entry = {"K": K, "segments": segs}
        for name, lib in libs.items():
            out = torch.empty(2 * K, dtype=torch.float64, device=dev)
            work = torch.empty(2 * K * min(n_chunks, 1024), dtype=torch.float64, device=dev)
            dotnorm2_with(lib, ptrs, K, g, rows[K - 1], chunks, n_chunks, out, work)
            ok = bool(((out[:K] - wd).abs() <= tol * mag).all()) and bool(((out[K:] - wn).abs() <= tol * wn).all()) \
                and bool(out[K - 1] == out[2 * K - 1])
            entry[f"dotnorm2_{name}_ok"] = ok
        c = (torch.rand(K, generator=gen, device=dev) / K).tolist()
        N = segs[-1][0] + segs[-1][1]
        y = torch.empty(L, dtype=torch.float32, device=dev)
        dfn.wsum_diff_rows(ptrs, kn.upload_f32(c, dev), K, g, N, y)
        spec = dfn.wsum_diff_rows_torch(rows, c, g)
        entry["wsum_diff_bit_identical"] = bool(torch.equal(y[:N].view(torch.int32), spec[:N].view(torch.int32)))
        entry["ok"] = all(v for k, v in entry.items() if k.endswith("_ok") or k.endswith("identical"))
        res.append(entry)
        print(entry, flush=True)
    return res


def timed(fns, runs: int = RUNS, warmup: int = 2):
    """The functions launched in turn, `runs` rounds after warm-up; -> one list
    of milliseconds each (device events around every call)."""
    import torch

    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    return ts


def stats(ts, nbytes: int) -> dict:
    med = statistics.median(ts)
    return {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "TBps": round(nbytes / med / 1e9, 3), "hbm_fraction": round(nbytes / med / 1e9 / HBM_TBPS, 3)}


def time_one(rows, K: int, N: int, ref, root, dev) -> dict:
    import torch

    from fedml_amd import defense as dfn
    from fedml_amd import kernels as kn

    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    ptrs1 = kn.upload_i64([rows[i].data_ptr() for i in range(K)] + [ref.data_ptr()], dev)
    chunks, n_chunks = table_for([(0, N)], dev)
    libs = {b: load_variant(b) for b in BATCHES}
    out = torch.empty(2 * K, dtype=torch.float64, device=dev)
    work = torch.empty(2 * K * min(n_chunks, 1024), dtype=torch.float64, device=dev)
    y = torch.empty(rows.shape[1], dtype=torch.float32, device=dev)
    c = kn.upload_f32([1.0 / K] * K, dev)
    w1 = torch.full((K + 1,), 1.0 / (K + 1), dtype=torch.float32, device=dev)
    row_bytes = N * 4
    r = {"K": K, "N": N}

    def dist2():
        dfn.dist2_rows(ptrs, K, ref, chunks, n_chunks, dev)

    def dist2_twice():
        dist2()
        dist2()

    dn, d1, d2 = timed([lambda: dotnorm2_with(nat.lib(), ptrs, K, ref, root, chunks, n_chunks, out, work),
                        dist2, dist2_twice])
    r["dotnorm2"] = stats(dn, (K + 2) * row_bytes)
    r["dist2_once"] = stats(d1, (K + 1) * row_bytes)
    r["dist2_twice"] = stats(d2, 2 * (K + 1) * row_bytes)
    r["dotnorm2_over_dist2_once"] = round(r["dotnorm2"]["median_ms"] / r["dist2_once"]["median_ms"], 3)
    r["dotnorm2_over_dist2_twice"] = round(r["dotnorm2"]["median_ms"] / r["dist2_twice"]["median_ms"], 3)
    wd, ws = timed([lambda: dfn.wsum_diff_rows(ptrs, c, K, ref, N, y),
                    lambda: kn.wsum_ptrs(torch.float32, ptrs1, w1, K + 1, N, y, True)])
    r["wsum_diff"] = stats(wd, (K + 2) * row_bytes)
    r["wsum_f32_K_plus_1"] = stats(ws, (K + 2) * row_bytes)
    r["wsum_diff_over_wsum"] = round(r["wsum_diff"]["median_ms"] / r["wsum_f32_K_plus_1"]["median_ms"], 3)
    tb = timed([(lambda lib: lambda: dotnorm2_with(lib, ptrs, K, ref, root, chunks, n_chunks, out, work))(libs[b])
                for b in BATCHES])
    for b, t in zip(BATCHES, tb):
        r[f"dotnorm2_batch{b}"] = stats(t, (K + 2) * row_bytes)
    r["batch16_over_batch8"] = round(r["dotnorm2_batch16"]["median_ms"] / r["dotnorm2_batch8"]["median_ms"], 3)
    print(r, flush=True)
    return r


def time_all(dev, quick: bool) -> list:
    import torch

    N = 25_610_152 // (10 if quick else 1)
    L = (N + 63) // 64 * 64
    KMAX = 512
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = torch.empty((KMAX, L), dtype=torch.float32, device=dev)
    ref = torch.randn(L, generator=gen, device=dev)
    root = ref + 0.05 * torch.randn(L, generator=gen, device=dev)
    for i in range(KMAX):  # honest clients around the root update: row by row, no KMAX x L temporary
        rows[i] = root + 0.05 * torch.randn(L, generator=gen, device=dev)
    return [time_one(rows, K, N, ref, root, dev) for K in (128, 32, 512)]


def main() -> int:
    step = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else None
    if step == "build":
        for p in build_variants():
            print(p)
        return 0
    if step not in ("check", "time"):
        print(__doc__)
        return 2
    import torch

    path = os.path.join(ROOT, "profiles", "fltrust_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    summary = {}
    if os.path.exists(path):
        with open(path) as f:
            summary = json.load(f)
    dev = torch.device("cuda:0")
    summary["device"] = torch.cuda.get_device_name(dev)
    rc = 0
    if step == "check":
        summary["checks"] = check(dev)
        summary["all_checks_ok"] = all(c["ok"] for c in summary["checks"])
        rc = 0 if summary["all_checks_ok"] else 1
    else:
        summary["runs_each"] = RUNS
        summary["shipped_batch"] = 8
        summary["timings"] = time_all(dev, "--quick" in sys.argv)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
