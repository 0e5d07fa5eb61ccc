"""Check and time the coordinate-wise trimmed mean kernel for 129 to 1024
clients against the torch path it replaces (tool only).

    python tools/trimmed_wide_probe.py --step check|time|config4 [--out FILE] [--cols N] [--iters I]

Every step adds its section to the JSON file (default:
profiles/trimmed_wide_probe.json; check starts it afresh), so a job script
(tools/gpu_trimmed_wide_probe.sh) can give each step a time limit of its own:

  check    a few small shapes, fedagg_trimmed_mean_wide bit for bit against
           fedml_amd.defense.trimmed_mean_rows_torch, in fp32, bf16 and f16;
  time     K = 256, 512, 1024 (full tiers) and 200, 384, 700 (padded), fp32
           and bf16, trim = int(0.1 K), at --cols columns (default 4,194,304,
           the column count of the median's lane tiers): the kernel,
           fedagg_median and trimmed_mean_rows_torch launched in turn on the
           same rows, --iters times (default 10) after a warm-up round; the
           median of each with its min-max spread, the ratios, and whether the
           kernel wins by defense.py's rule (its median time is below the
           torch path's by more than the larger spread of the two).  The last
           round's outputs are compared bit for bit.  Prints the seconds the
           torch legs took, from which a full run's time limit follows;
  config4  512 clients x 86.6M bf16 (config 4): the kernel alone, launched
           once after a small launch has loaded its code, and its last 4,096
           columns compared with the torch path.
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBPS = 8.0
TIME_KS = (256, 512, 1024, 200, 384, 700)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    nan = torch.isnan(b)
    return bool(torch.equal(torch.isnan(a), nan) and ((a.view(it) == b.view(it)) | nan).all())


def make_rows(dev, dt, K: int, N: int, seed: int = 0):
    L = (N + 63) // 64 * 64
    rows = torch.empty((K, L), dtype=dt, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    for i in range(K):  # row by row: no K x L fp32 temporary
        rows[i] = (0.05 * torch.randn(L, generator=g, device=dev)).to(dt)
    return rows, kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)


def check(dev) -> dict:
    res = []
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for K, trim, N in ((129, 12, 1000), (256, 25, 4099), (300, 30, 70_001), (512, 51, 65_537), (700, 0, 9_001),
                           (1024, 102, 40_000)):
            rows, ptrs = make_rows(dev, dt, K, N, seed=K)
            rows[0, ::97] = float("nan")
            rows[1, ::89] = float("inf")
            rows[2, ::83] = -float("inf")
            out = torch.empty(N, dtype=dt, device=dev)
            dfn.trimmed_mean_rows_wide(ptrs, K, N, trim, out)
            ok = same(out, dfn.trimmed_mean_rows_torch(rows[:, :N], trim))
            res.append({"dtype": str(dt), "K": K, "trim": trim, "N": N, "bit_identical": ok})
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


def time_shape(dev, dt, K: int, N: int, iters: int) -> dict:
    trim = int(0.1 * K)
    rows, ptrs = make_rows(dev, dt, K, N)
    out_k = torch.empty(rows.shape[1], dtype=dt, device=dev)
    out_m = torch.empty(rows.shape[1], dtype=dt, device=dev)
    res = {}
    legs = {"kernel": lambda: dfn.trimmed_mean_rows_wide(ptrs, K, N, trim, out_k),
            "median": lambda: dfn.median_rows(ptrs, K, N, out_m, aligned=True),
            "torch": lambda: res.__setitem__("t", dfn.trimmed_mean_rows_torch(rows[:, :N], trim))}
    ts = {k: [] for k in legs}
    torch_s = 0.0
    for it in range(iters + 1):  # round 0 warms every leg up
        for name, fn in legs.items():
            t0 = time.perf_counter()
            ms = _event_ms(fn)
            if name == "torch":
                torch_s += time.perf_counter() - t0
            if it:
                ts[name].append(ms)
    k, m, t = (_stats(ts[n]) for n in ("kernel", "median", "torch"))
    spread = max(k["max_ms"] - k["min_ms"], t["max_ms"] - t["min_ms"])
    nbytes = K * N * rows.element_size()
    r = {"dtype": str(dt), "K": K, "N": N, "trim": trim, "iters": iters, "kernel": k, "median": m, "torch": t,
         "torch_over_kernel": round(t["median_ms"] / k["median_ms"], 2),
         "kernel_over_median": round(k["median_ms"] / m["median_ms"], 3),
         "kernel_wins": bool(t["median_ms"] - k["median_ms"] > spread),
         "kernel_TBps": round(nbytes / k["median_ms"] / 1e9, 3),
         "kernel_hbm_fraction": round(nbytes / k["median_ms"] / 1e9 / HBM_TBPS, 3),
         "bit_identical": same(out_k[:N], res["t"]), "torch_leg_seconds": round(torch_s, 2)}
    print(r, flush=True)
    return r


def timings(dev, cols: int, iters: int) -> dict:
    rs = []
    for dt in (torch.float32, torch.bfloat16):
        for K in TIME_KS:
            rs.append(time_shape(dev, dt, K, cols, iters))
            torch.cuda.empty_cache()
    total = sum(r["torch_leg_seconds"] for r in rs)
    print(f"torch_leg_seconds_total {total:.1f} cols {cols} rounds {iters + 1}", flush=True)
    return {"timings": rs, "timings_cols": cols, "torch_leg_seconds_total": round(total, 1)}


def config4(dev) -> dict:
    K, N, dt = 512, 86_600_000, torch.bfloat16
    trim = int(0.1 * K)
    rows, ptrs = make_rows(dev, dt, K, N)
    out = torch.empty(rows.shape[1], dtype=dt, device=dev)
    dfn.trimmed_mean_rows_wide(ptrs, K, 4096, trim, out)  # loads the code object
    torch.cuda.synchronize(dev)
    ms = _event_ms(lambda: dfn.trimmed_mean_rows_wide(ptrs, K, N, trim, out))
    tail = dfn.trimmed_mean_rows_torch(rows[:, N - 4096:N], trim)
    nbytes = K * N * 2
    r = {"dtype": str(dt), "K": K, "N": N, "trim": trim, "launches": 1, "kernel_ms": round(ms, 3),
         "kernel_TBps": round(nbytes / ms / 1e9, 3), "kernel_hbm_fraction": round(nbytes / ms / 1e9 / HBM_TBPS, 3),
         "last_4096_columns_bit_identical": same(out[N - 4096:N], tail)}
    print(r, flush=True)
    return {"config4": r}


def main() -> int:
    def arg(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    step = arg("--step", "check")
    path = arg("--out", os.path.join(ROOT, "profiles", "trimmed_wide_probe.json"))
    dev = torch.device("cuda:0")
    summary = {}
    if os.path.exists(path) and step != "check":  # check, the first step, starts the file afresh
        with open(path) as f:
            summary = json.load(f)
    summary["device"] = torch.cuda.get_device_name(dev)
    if step == "check":
        part = check(dev)
    elif step == "time":
        part = timings(dev, int(arg("--cols", 4_194_304)), int(arg("--iters", 10)))
    elif step == "config4":
        part = config4(dev)
    else:
        raise SystemExit(f"unknown step {step!r}")
    summary.update(part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    ok = part.get("all_bit_identical", True) and all(r["bit_identical"] for r in part.get("timings", [])) and \
        part.get("config4", {}).get("last_4096_columns_bit_identical", True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
