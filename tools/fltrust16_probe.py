"""Time the two kernels of the "fltrust" defense on bf16 / f16 rows (tool only).

    python tools/fltrust16_probe.py --step build           # no GPU: the two batch builds of dotnorm2_16_kernel
    python tools/fltrust16_probe.py --step time [--out F]  # default: profiles/fltrust16_probe.json

build: csrc/fltrust16.hip compiled twice more, with -DFEDAGG_DOTNORM16_BATCH=8
and =16 (the clients a wave of dotnorm2_16_kernel holds per pass), each linked
with the product's other objects into tools/_build/libfedagg_dotnorm16_b<B>.so.
Run it where the compiler is; the time step only loads the libraries.

time: K = 128 and K = 100 rows of 4,194,304 columns, bf16 and f16.  The 16-bit
pair (fedagg_dotnorm2_16 with the root as row K, fedagg_wsum_diff_16) against
the fp32 pair on an exactly widened copy of the same rows, each pair of
functions launched alternately, 10 runs of each after warm-up, median with
min - max; then the 8-client build of the dot kernel against the 16-client
build.  Before the timing the results are compared: the dot products and norms
within n 2^-51 sum|terms| of the fp32 kernel's (each within n 2^-52 of the
exact sum), the rebuild bit for bit the fp32 kernel's row rounded by .to(dtype).
`keep_batch`: 16 where its median wins by more than the larger min-max spread
of the two builds in every shape, else 8.
"""
from __future__ import annotations

import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import build as fbuild  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tools", "_build")
BATCHES = (8, 16)
HBM_TBPS = 8.0
RUNS = 10
N = 4_194_304
UNIT = os.path.join(fbuild.HERE, "csrc", "fltrust16.hip")


def variant_path(batch: int) -> str:
    return os.path.join(OUT_DIR, f"libfedagg_dotnorm16_b{batch}.so")


def build_variants() -> list:
    fbuild.build()  # the product's other objects, which the variants link with
    os.makedirs(OUT_DIR, exist_ok=True)
    others = [fbuild._obj(s) for s in fbuild.SRCS if s != UNIT]
    outs = []
    for b in BATCHES:
        obj = os.path.join(OUT_DIR, f"fltrust16_b{b}.o")
        subprocess.run([fbuild.hipcc(), *fbuild.HIPCC_FLAGS, *fbuild.UNIT_FLAGS["fltrust16.hip"],
                        f"-DFEDAGG_DOTNORM16_BATCH={b}", "-c", "-o", obj, UNIT], check=True)
        subprocess.run([fbuild.hipcc(), f"--offload-arch={fbuild.ARCH}", "-shared", "-fPIC", "-o", variant_path(b),
                        obj, *others], check=True)
        outs.append(variant_path(b))
    return outs


def load_variant(batch: int) -> ctypes.CDLL:
    path = variant_path(batch)
    if not os.path.exists(path):
        raise nat.FedAggNativeError(f"{path} not found: python tools/fltrust16_probe.py --step build")
    handle = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in nat.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


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


def time_one(dt, K: int, dev) -> dict:
    import torch

    from fedml_amd import defense as dfn
    from fedml_amd import kernels as kn

    gen = torch.Generator(device=dev).manual_seed(K)
    ref32 = 0.05 * torch.randn(N, generator=gen, device=dev)
    rows16 = torch.empty((K + 1, N), dtype=dt, device=dev)  # row K: the root
    rows16[K] = ref32 + 0.01 * torch.randn(N, generator=gen, device=dev)
    for i in range(K):  # honest clients around the root update: row by row, no K x N fp32 temporary
        rows16[i] = rows16[K].float() + 0.01 * torch.randn(N, generator=gen, device=dev)
    ref16 = ref32.to(dt)
    rows32, ref32 = rows16.float(), ref16.float()  # the exactly widened copy
    p16 = kn.upload_i64([rows16[i].data_ptr() for i in range(K + 1)], dev)
    p32 = kn.upload_i64([rows32[i].data_ptr() for i in range(K + 1)], dev)
    g = type("G", (), {"keys": ["k.weight"], "offsets": [0], "numels": [N]})
    chunks, n_chunks = dfn.weight_chunks(g, nat.DIST_CHUNK, dev)
    c = kn.upload_f32([1.0 / K] * K, dev)
    y16 = torch.empty(N, dtype=dt, device=dev)
    y32 = torch.empty(N, dtype=torch.float32, device=dev)
    code = {torch.bfloat16: nat.DT_BF16, torch.float16: nat.DT_F16}[dt]
    out = torch.empty(2 * (K + 1), dtype=torch.float64, device=dev)
    work = torch.empty(2 * (K + 1) * min(n_chunks, 1024), dtype=torch.float64, device=dev)

    def dot16_with(lib):
        def run():
            rc = lib.fedagg_dotnorm2_16(code, p16.data_ptr(), K + 1, ref16.data_ptr(), rows16[K].data_ptr(),
                                        chunks.data_ptr(), n_chunks, out.data_ptr(), work.data_ptr(), work.numel(),
                                        nat.stream_handle())
            if rc != 0:
                raise nat.FedAggNativeError(f"dotnorm2_16 (rc={rc}): {lib.fedagg_last_error().decode()}")
        return run

    r = {"dtype": str(dt), "K": K, "N": N}
    # the results first: the two pairs compute the same thing
    d16, n16 = dfn.dotnorm2_rows(p16, K + 1, ref16, rows16[K], chunks, n_chunks, dev)
    d32, n32 = dfn.dotnorm2_rows(p32, K + 1, ref32, rows32[K], chunks, n_chunks, dev)
    a = (rows32[K] - ref32).double()
    tol = N * 2.0 ** -51
    mag = torch.stack([((rows32[i] - ref32).double() * a).abs().sum() for i in range(K + 1)])
    r["dot_within_bound"] = bool(((d16 - d32).abs() <= tol * mag).all()) and \
        bool(((n16 - n32).abs() <= tol * n32).all())
    dfn.wsum_diff_rows(p16, c, K, ref16, N, y16)
    dfn.wsum_diff_rows(p32, c, K, ref32, N, y32)
    r["rebuild_bit_identical"] = bool(torch.equal(y16.view(torch.int16), y32.to(dt).view(torch.int16)))
    del a, mag

    t16, t32 = timed([lambda: dfn.dotnorm2_rows(p16, K + 1, ref16, rows16[K], chunks, n_chunks, dev),
                      lambda: dfn.dotnorm2_rows(p32, K + 1, ref32, rows32[K], chunks, n_chunks, dev)])
    r["dotnorm2_16"] = stats(t16, (K + 3) * N * 2)
    r["dotnorm2_f32_widened"] = stats(t32, (K + 3) * N * 4)
    w16, w32 = timed([lambda: dfn.wsum_diff_rows(p16, c, K, ref16, N, y16),
                      lambda: dfn.wsum_diff_rows(p32, c, K, ref32, N, y32)])
    r["wsum_diff_16"] = stats(w16, (K + 2) * N * 2)
    r["wsum_diff_f32_widened"] = stats(w32, (K + 2) * N * 4)
    pair16 = r["dotnorm2_16"]["median_ms"] + r["wsum_diff_16"]["median_ms"]
    pair32 = r["dotnorm2_f32_widened"]["median_ms"] + r["wsum_diff_f32_widened"]["median_ms"]
    r["pair16_ms"], r["pair_f32_ms"] = round(pair16, 4), round(pair32, 4)
    r["pair16_over_f32"] = round(pair16 / pair32, 3)
    tb = timed([dot16_with(load_variant(b)) for b in BATCHES])
    for b, t in zip(BATCHES, tb):
        r[f"dotnorm2_16_batch{b}"] = stats(t, (K + 3) * N * 2)
    s8, s16 = r["dotnorm2_16_batch8"], r["dotnorm2_16_batch16"]
    spread = max(s8["max_ms"] - s8["min_ms"], s16["max_ms"] - s16["min_ms"])
    r["batch16_wins"] = bool(s8["median_ms"] - s16["median_ms"] > spread)
    print(r, flush=True)
    return r


def main() -> int:
    step = sys.argv[sys.argv.index("--step") + 1] if "--step" in sys.argv else None
    if step == "build":
        for p in build_variants():
            print(p)
        return 0
    if step != "time":
        print(__doc__)
        return 2
    import torch

    path = os.path.join(ROOT, "profiles", "fltrust16_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    dev = torch.device("cuda:0")
    timings = [time_one(dt, K, dev) for dt in (torch.bfloat16, torch.float16) for K in (128, 100)]
    summary = {"device": torch.cuda.get_device_name(dev), "runs_each": RUNS, "timings": timings,
               "results_agree": all(t["dot_within_bound"] and t["rebuild_bit_identical"] for t in timings),
               "keep_batch": 16 if all(t["batch16_wins"] for t in timings) else 8}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    return 0 if summary["results_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
