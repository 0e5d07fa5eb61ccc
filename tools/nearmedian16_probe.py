"""Check and time Bulyan's nearest-to-median mean kernels on bf16 / f16 rows
against the torch path (which decides NEARMEDIAN_WIDE16_AUTO) and against the
fp32 kernels on a widened copy of the same rows (tool only).

    python tools/nearmedian16_probe.py --step check|time [--dtype bf16|f16] [--out FILE] [--cols N] [--iters I]

Every step adds its section to the JSON file (default:
profiles/nearmedian16_probe.json; check starts it afresh), so a job script can
give each step a time limit of its own:

  check  a few small shapes per dtype, fedagg_nearmedian_mean_16 and
         fedagg_nearmedian_mean_wide_16 bit for bit against
         fedml_amd.defense.nearmedian_mean_rows16_torch;
  time   per dtype (default: both) K = 128, 256, 512, 1024 (full tiers) and
         100, 200, 384, 700 (padded) at keep = K - 2 (K // 8) and --cols columns
         (default 4,194,304): the 16-bit kernel, the fp32 kernel on the
         exactly widened copy of the same rows (what the 16-bit path costs or
         saves; it decides nothing) and, above 128 rows,
         nearmedian_mean_rows16_torch, launched in turn --iters times (default
         10) after a warm-up round; the median of each with its min and max,
         the ratios, and whether the kernel wins by defense.py's rule (its
         median time is below the torch path's by more than the larger min-max
         spread of the two).  The last round's outputs are compared bit for bit.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBPS = 8.0
TIME_KS = (128, 100, 256, 200, 512, 384, 1024, 700)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    nan = torch.isnan(b)
    return bool(torch.equal(torch.isnan(a), nan) and ((a.view(torch.int16) == b.view(torch.int16)) | nan).all())


def make_rows(dev, K: int, N: int, dtype, seed: int = 0):
    L = (N + 63) // 64 * 64
    rows = torch.empty((K, L), dtype=dtype, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    for i in range(K):  # row by row: no K x L fp32 temporary
        rows[i] = (0.05 * torch.randn(L, generator=g, device=dev)).to(dtype)
    return rows


def table(rows, dev):
    return kn.upload_i64([rows[i].data_ptr() for i in range(rows.shape[0])], dev)


def kernel16(K: int):
    return dfn.nearmedian_mean_rows16 if K <= dfn.NEARMEDIAN_MAX_CLIENTS else dfn.nearmedian_mean_rows_wide16


def check(dev) -> dict:
    res = []
    for name, dtype in DTYPES.items():
        for K, keep, N in ((9, 5, 1000), (100, 76, 4099), (128, 96, 70_001), (129, 105, 1000), (256, 192, 4099),
                           (300, 226, 70_001), (700, 128, 9_001), (1024, 768, 40_000)):
            rows = make_rows(dev, K, N, dtype, seed=K)
            rows[0, ::97] = float("nan")
            rows[1, ::89] = float("inf")
            rows[2, ::83] = -float("inf")
            out = torch.empty(N, dtype=dtype, device=dev)
            kernel16(K)(table(rows, dev), K, N, keep, out)
            ok = same(out, dfn.nearmedian_mean_rows16_torch(rows[:, :N], keep))
            res.append({"dtype": name, "K": K, "keep": keep, "N": N, "bit_identical": ok})
            print(res[-1], flush=True)
    return {"checks": res, "all_bit_identical": all(c["bit_identical"] for c in res)}


def _event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts) -> dict:
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def time_shape(dev, name: str, dtype, K: int, N: int, iters: int) -> dict:
    keep = K - 2 * (K // 8)
    rows = make_rows(dev, K, N, dtype)
    rows32 = rows.float()  # the copy this path exists to avoid
    ptrs, ptrs32 = table(rows, dev), table(rows32, dev)
    out16 = torch.empty(rows.shape[1], dtype=dtype, device=dev)
    out32 = torch.empty(rows.shape[1], dtype=torch.float32, device=dev)
    wide = K > dfn.NEARMEDIAN_MAX_CLIENTS
    fp32 = dfn.nearmedian_mean_rows_wide if wide else dfn.nearmedian_mean_rows
    res = {}
    legs = {"kernel16": lambda: kernel16(K)(ptrs, K, N, keep, out16),
            "kernel_fp32_widened": lambda: fp32(ptrs32, K, N, keep, out32)}
    if wide:
        legs["torch"] = lambda: res.__setitem__("t", dfn.nearmedian_mean_rows16_torch(rows[:, :N], keep))
    ts = {k: [] for k in legs}
    for it in range(iters + 1):  # round 0 warms every leg up
        for leg, fn in legs.items():
            ms = _event_ms(fn)
            if it:
                ts[leg].append(ms)
    k, w = _stats(ts["kernel16"]), _stats(ts["kernel_fp32_widened"])
    nbytes = K * N * rows.element_size()
    r = {"dtype": name, "K": K, "N": N, "keep": keep, "iters": iters, "kernel16": k, "kernel_fp32_widened": w,
         "kernel16_over_fp32": round(k["median_ms"] / w["median_ms"], 3),
         "kernel16_TBps": round(nbytes / k["median_ms"] / 1e9, 3),
         "kernel16_hbm_fraction": round(nbytes / k["median_ms"] / 1e9 / HBM_TBPS, 3),
         # the fp32 kernel's mean, rounded once, is the 16-bit kernel's
         "bit_identical": same(out16[:N], out32[:N].to(dtype))}
    if wide:
        t = _stats(ts["torch"])
        spread = max(k["max_ms"] - k["min_ms"], t["max_ms"] - t["min_ms"])
        r.update({"torch": t, "torch_over_kernel16": round(t["median_ms"] / k["median_ms"], 2),
                  "larger_spread_ms": round(spread, 4), "kernel_wins": bool(t["median_ms"] - k["median_ms"] > spread),
                  "bit_identical": r["bit_identical"] and same(out16[:N], res["t"])})
    print(r, flush=True)
    return r


def timings(dev, names, cols: int, iters: int, prev: list) -> dict:
    rs = [r for r in prev if r["dtype"] not in names]  # a dtype timed again replaces its rows
    for name in names:
        for K in TIME_KS:
            rs.append(time_shape(dev, name, DTYPES[name], K, cols, iters))
            torch.cuda.empty_cache()
    return {"timings": rs, "timings_cols": cols}


def main() -> int:
    def arg(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    step = arg("--step", "check")
    path = arg("--out", os.path.join(ROOT, "profiles", "nearmedian16_probe.json"))
    dev = torch.device("cuda:0")
    summary = {}
    if os.path.exists(path) and step != "check":  # check, the first step, starts the file afresh
        with open(path) as f:
            summary = json.load(f)
    summary["device"] = torch.cuda.get_device_name(dev)
    if step == "check":
        part = check(dev)
    elif step == "time":
        names = [arg("--dtype", None)] if "--dtype" in sys.argv else list(DTYPES)
        part = timings(dev, names, int(arg("--cols", 4_194_304)), int(arg("--iters", 10)), summary.get("timings", []))
    else:
        raise SystemExit(f"unknown step {step!r}")
    summary.update(part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    ok = part.get("all_bit_identical", True) and all(r["bit_identical"] for r in part.get("timings", []))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
