"""A/B of two builds of libfedagg.so on the same buffers (tool only): the
fused FedAvg + server SGD / Adam steps of config 5 and the plain fp32 / bf16
FedAvg, each build's launch timed back to back (`--launches` per sample),
the builds interleaved round by round, medians reported.

    python tools/ab_libs.py fedml_amd/lib/ab/libfedagg_r05start.so fedml_amd/lib/libfedagg.so

`--cases lanes` times the lane-group kernels above 128 clients instead (the
median, the wide trimmed mean and the wide nearest-to-median mean, each tier
at its full K and at one padded K): any number of builds, all of them writing
the SAME output buffer (NOTES.md: a buffer of its own per build read 2.5 %
apart), the order of the builds reversed every other round, outputs compared
bit for bit with the first build's, median and min-max per build.  A second
copy of the first build's file is the control:

    python tools/ab_libs.py --cases lanes lib/ab/parent.so lib/ab/parent_copy.so lib/libfedagg.so
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fedml_amd import _native as nat  # noqa: E402

P, I32, I64, U32, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path), mode=ctypes.RTLD_LOCAL)
    lib.fedagg_wsum_fedopt_sgd_f32.argtypes = [P, P, I32, I64, P, P, F, F, I32, U32, P]
    lib.fedagg_wsum_f32.argtypes = [P, P, I32, I64, P, U32, P]
    lib.fedagg_wsum_bf16.argtypes = [P, P, I32, I64, P, I32, U32, P]
    return lib


# tier (the full K), a padded K of it, columns; the last two are the median's alone
LANE_TIERS = [(256, 200, 4_194_304), (512, 384, 4_194_304), (1024, 700, 4_194_304),
              (2048, 1500, 1_048_576), (4096, 3000, 1_048_576)]
LANE_DT = {"f32": (nat.DT_F32, torch.float32), "bf16": (nat.DT_BF16, torch.bfloat16),
           "f16": (nat.DT_F16, torch.float16)}


def lanes(a):
    dev = torch.device("cuda:0")
    libs = [ctypes.CDLL(os.path.abspath(p), mode=ctypes.RTLD_LOCAL) for p in a.libs]
    for lib in libs:
        lib.fedagg_median.argtypes = [I32, P, I32, I64, P, U32, P]
        lib.fedagg_trimmed_mean_wide.argtypes = [I32, P, I32, I64, I32, P, U32, P]
        lib.fedagg_nearmedian_mean_wide_f32.argtypes = [P, I32, I64, I32, P, U32, P]
    st = nat.stream_handle()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    names = [os.path.basename(p) for p in a.libs]
    results = []

    def wanted(name):
        return not a.only or any(w in name for w in a.only.split(","))

    for tier, padded, N in LANE_TIERS:
        for dname, (code, dt) in LANE_DT.items():
            if not any(wanted(f"{op}-K{k}-{dname}") for op in ("median", "median16", "trimmed", "nearmedian")
                       for k in (tier, padded)):
                continue  # no rows for a tier that --only leaves out
            rows = torch.empty((tier, N), device=dev, dtype=dt).normal_(0.0, 0.05)
            ptrs = torch.tensor([rows[i].data_ptr() for i in range(tier)], dtype=torch.int64, device=dev)
            out = torch.empty(N, device=dev, dtype=dt)
            o, s = out.data_ptr(), ptrs.data_ptr()
            for K in (tier, padded):
                # flags 0: the widening kernels for 16-bit rows too; median16: the packed ones
                cases = [("median", lambda lib: lib.fedagg_median(code, s, K, N, o, 0, st))]
                if dt != torch.float32 and tier > 1024:
                    cases.append(("median16", lambda lib: lib.fedagg_median(code, s, K, N, o, nat.FEDAGG_ALIGNED16, st)))
                if tier <= 1024:
                    cases.append(("trimmed", lambda lib: lib.fedagg_trimmed_mean_wide(code, s, K, N, K // 10, o, 0, st)))
                    if dt == torch.float32:
                        cases.append(("nearmedian", lambda lib: lib.fedagg_nearmedian_mean_wide_f32(
                            s, K, N, K - 2 * (K // 8), o, 0, st)))
                for op, fn in cases:
                    name = f"{op}-K{K}-{dname}"
                    if not wanted(name):
                        continue
                    ref = None
                    for lib, n in zip(libs, names):
                        out.zero_()
                        nat.check(fn(lib), name)
                        torch.cuda.synchronize()
                        bits = out.view(torch.int16 if out.element_size() == 2 else torch.int32).clone()
                        ref = bits if ref is None else ref
                        assert torch.equal(bits, ref), f"{name}: {n} differs from {names[0]}"
                    times = [[] for _ in libs]
                    for r in range(a.rounds):
                        for i in (range(len(libs)) if r % 2 == 0 else reversed(range(len(libs)))):
                            fn(libs[i])
                            ev0.record()
                            for _ in range(a.launches):
                                fn(libs[i])
                            ev1.record()
                            ev1.synchronize()
                            times[i].append(ev0.elapsed_time(ev1) / a.launches)
                    res = {"case": name, "N": N, "launches": a.launches, "rounds": a.rounds, "bit_identical": True,
                           "builds": {n: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
                                      for n, t in zip(names, times)}}
                    results.append(res)
                    print(f"{name:22s} " + "   ".join(f"{n}: {statistics.median(t):.4f} ({min(t):.4f}-{max(t):.4f})"
                                                      for n, t in zip(names, times)), flush=True)
                    if a.out:
                        with open(a.out, "w") as f:
                            json.dump(results, f, indent=1)
            del rows, ptrs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--cases", default="fedavg", choices=["fedavg", "lanes"])
    ap.add_argument("--only", default="", help="lanes: the cases whose name (op-K<K>-<dtype>) contains one of "
                                               "these, comma-separated (--only=-f32,trimmed-)")
    ap.add_argument("--out", default=None, help="lanes: the results as JSON")
    ap.add_argument("--rounds", type=int, default=None, help="samples per build (default 7; lanes: 10)")
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    if a.rounds is None:
        a.rounds = 10 if a.cases == "lanes" else 7
    if a.cases == "lanes":
        return lanes(a)
    if len(a.libs) != 2:
        ap.error("--cases fedavg takes two libraries")
    dev = torch.device("cuda:0")
    libs = [load(p) for p in a.libs]
    st = nat.stream_handle()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cases = []
    # config 5: 64 x 4,194,304 fp32 + SGD (lr 1, momentum 0.9)
    K, N = 64, 4_194_304
    rows5 = torch.empty((K, N), device=dev).normal_(0.0, 0.05)
    p5 = torch.tensor([rows5[i].data_ptr() for i in range(K)], dtype=torch.int64, device=dev)
    w5 = torch.full((K,), 1.0 / K, device=dev)
    param = [torch.zeros(N, device=dev) for _ in libs]
    mom = [torch.zeros(N, device=dev) for _ in libs]
    cases.append(("cfg5 FedAvg+SGD", lambda i: libs[i].fedagg_wsum_fedopt_sgd_f32(
        p5.data_ptr(), w5.data_ptr(), K, N, param[i].data_ptr(), mom[i].data_ptr(), 1.0, 0.9, 0, 1, st)))
    hw = (ctypes.c_float * K)(*([1.0 / K] * K))  # FEDAGG_HOST_WEIGHTS: kernel-argument weights
    cases.append(("cfg5 SGD host-w", lambda i: libs[i].fedagg_wsum_fedopt_sgd_f32(
        p5.data_ptr(), ctypes.addressof(hw), K, N, param[i].data_ptr(), mom[i].data_ptr(), 1.0, 0.9, 0, 3, st)))
    out5 = [torch.empty(N, device=dev) for _ in libs]
    cases.append(("cfg5 FedAvg", lambda i: libs[i].fedagg_wsum_f32(p5.data_ptr(), w5.data_ptr(), K, N,
                                                                   out5[i].data_ptr(), 1, st)))
    # config 3's fp32 row
    K3, N3 = 128, 25_610_205
    L3 = (N3 + 63) // 64 * 64
    rows3 = torch.empty((K3, L3), device=dev).normal_(0.0, 0.05)
    p3 = torch.tensor([rows3[i].data_ptr() for i in range(K3)], dtype=torch.int64, device=dev)
    w3 = torch.full((K3,), 1.0 / K3, device=dev)
    out3 = [torch.empty(L3, device=dev) for _ in libs]
    cases.append(("cfg3 FedAvg", lambda i: libs[i].fedagg_wsum_f32(p3.data_ptr(), w3.data_ptr(), K3, N3,
                                                                   out3[i].data_ptr(), 1, st)))
    hw3 = (ctypes.c_float * K3)(*([1.0 / K3] * K3))
    cases.append(("cfg3 FedAvg host-w", lambda i: libs[i].fedagg_wsum_f32(p3.data_ptr(), ctypes.addressof(hw3), K3,
                                                                          N3, out3[i].data_ptr(), 3, st)))
    for name, fn in cases:
        for i in range(2):
            nat.check(fn(i), name)
        torch.cuda.synchronize()
        times = [[], []]
        for _ in range(a.rounds):
            for i in range(2):
                ev0.record()
                for _ in range(a.launches):
                    fn(i)
                ev1.record()
                ev1.synchronize()
                times[i].append(ev0.elapsed_time(ev1) / a.launches)
        m = [statistics.median(t) for t in times]
        print(f"{name:18s} {os.path.basename(a.libs[0])}: {m[0]:.4f} ms   {os.path.basename(a.libs[1])}: {m[1]:.4f} ms"
              f"   ({(m[1] / m[0] - 1) * 100:+.1f} %)", flush=True)


if __name__ == "__main__":
    main()
