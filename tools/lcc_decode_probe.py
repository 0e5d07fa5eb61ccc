"""Time the two kernels of the LightSecAgg mask decode against each other, and
numpy's decode on the host (tool only).

    python tools/lcc_decode_probe.py [--out FILE] [--quick]   # default: profiles/lcc_decode_probe.json

fedagg_lcc_decode_i64 (csrc/lccdecode.hip) with FEDAGG_LCC_VALU (the exact
64-bit kernel) and FEDAGG_LCC_MFMA (int8 matrix cores) on the same rows, at the
server's shapes: p = 2^15 - 19, T = U / 2, d = 25,610,152, so M = ceil(d / (U - T))
columns and the R = U - T target rows that [0:d] keeps; U = 32, 128, 512 (the
tiers of secagg.LCC_MFMA_AUTO) and one padded U of each (24, 100, 384).  The
two are launched alternately in the same process, median of 10 after warm-up,
min and max; the outputs are compared bit for bit at every shape timed.

The rule of LCC_MFMA_AUTO: the matrix-core kernel wins a tier only where the
exact kernel's median exceeds its median by more than the larger of the two
min-max spreads, at the tier's U and at the padded U.

The baseline is what FedML runs, numpy's (C.dot(F)) % p on int64, timed on this
host at U = 64, T = 32 and 200,000 columns (median of 3) and compared with the
exact kernel there.  --quick: one tenth of d.
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402
from geomed16_probe import RUNS, stats, timed_pair  # noqa: E402

P = 2 ** 15 - 19
TIERS = {32: 24, 128: 100, 512: 384}  # tier -> its padded U


def launcher(F, C, n_out, method, dev):
    U, M = F.shape
    R = C.shape[0]
    ptrs = kn.upload_i64([F[i].data_ptr() for i in range(U)], dev)
    out = torch.empty(n_out, dtype=torch.int64, device=dev)
    work = torch.empty(max(nat.lib().fedagg_lcc_work_bytes(U, R, M), 16), dtype=torch.uint8, device=dev)

    def run():
        nat.check(nat.lib().fedagg_lcc_decode_i64(ptrs.data_ptr(), U, M, C.data_ptr(), R, P, out.data_ptr(), n_out,
                                                  method, work.data_ptr(), work.numel(), nat.stream_handle()),
                  "lcc_decode_i64")
    run.out, run.keep = out, (ptrs, work)
    return run


def one(U: int, d: int, dev, gen) -> dict:
    T = U // 2
    M = -(-d // (U - T))
    R = -(-d // M)
    F = torch.randint(0, P, (U, M), generator=gen, device=dev, dtype=torch.int64)
    C = torch.randint(0, P, (R, U), generator=gen, device=dev, dtype=torch.int64)
    valu, mfma = launcher(F, C, d, nat.LCC_VALU, dev), launcher(F, C, d, nat.LCC_MFMA, dev)
    valu(), mfma()
    same = bool(torch.equal(valu.out, mfma.out))
    a, b = (stats(t) for t in timed_pair(mfma, valu))
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    r = {"U": U, "T": T, "R": R, "M": M, "mfma": a, "valu": b, "valu_over_mfma": round(b["median_ms"] / a["median_ms"], 3),
         "mfma_read_TBps": round(U * M * 8 / a["median_ms"] / 1e9, 3),
         "valu_Gmac_per_s": round(U * R * M / b["median_ms"] / 1e6, 1),
         "gap_ms": round(b["median_ms"] - a["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "wins": bool(b["median_ms"] - a["median_ms"] > spread), "bit_identical": same}
    print(r, flush=True)
    return r


def numpy_baseline(dev, gen) -> dict:
    U, R, M = 64, 32, 200_000
    F = torch.randint(0, P, (U, M), generator=gen, device=dev, dtype=torch.int64)
    C = torch.randint(0, P, (R, U), generator=gen, device=dev, dtype=torch.int64)
    valu = launcher(F, C, R * M, nat.LCC_VALU, dev)
    gpu = stats(timed_pair(valu, lambda: None)[0])
    Fh, Ch = F.cpu().numpy(), C.cpu().numpy()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = Ch.dot(Fh) % P
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(ts)
    r = {"U": U, "R": R, "M": M, "numpy_ms": round(ms, 1), "numpy_Gmac_per_s": round(U * R * M / ms / 1e6, 3),
         "valu": gpu, "numpy_over_valu": round(ms / gpu["median_ms"], 1),
         "bit_identical": bool(np.array_equal(valu.out.cpu().numpy().reshape(R, M), want))}
    print(r, flush=True)
    return r


def main():
    dev = torch.device("cuda:0")
    d = 25_610_152 // (10 if "--quick" in sys.argv else 1)
    gen = torch.Generator(device=dev).manual_seed(0)
    summary = {"device": torch.cuda.get_device_name(dev), "p": P, "d": d, "runs_each": RUNS, "timings": []}
    for tier, padded in TIERS.items():
        for U in (tier, padded):
            summary["timings"].append(one(U, d, dev, gen))
            torch.cuda.empty_cache()
    summary["wins_by_rule"] = {str(t): all(r["wins"] for r in summary["timings"] if r["U"] in (t, p))
                               for t, p in TIERS.items()}
    summary["numpy_baseline"] = numpy_baseline(dev, gen)
    summary["all_checks_ok"] = all(r["bit_identical"] for r in summary["timings"] + [summary["numpy_baseline"]])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "lcc_decode_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary["wins_by_rule"]))
    return 0 if summary["all_checks_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
