"""Check and time Bulyan's nearest-to-median mean kernel for 129 to 1024
selected clients against the torch path it replaces (tool only).

    python tools/nearmedian_wide_probe.py --step check|time [--out FILE] [--cols N] [--iters I]

Every step adds its section to the JSON file (default:
profiles/nearmedian_wide_probe.json; check starts it afresh), so a job script
can give each step a time limit of its own:

  check  a few small shapes, fedagg_nearmedian_mean_wide_f32 bit for bit
         against fedml_amd.defense.nearmedian_mean_rows_torch;
  time   K = 256, 512, 1024 (full tiers) and 200, 384, 700 (padded), fp32, at
         keep = K - 2 (K // 8) and keep = K, at --cols columns (default
         4,194,304): the kernel, fedagg_trimmed_mean_wide at trim =
         (K - keep) // 2 (a diagnostic: what the window costs on top of the
         sort) and nearmedian_mean_rows_torch launched in turn on the same
         rows, --iters times (default 10) after a warm-up round; the median of
         each with its min and max, the ratios, and whether the kernel wins by
         defense.py's rule (its median time is below the torch path's by more
         than the larger min-max spread of the two).  The last round's outputs
         are compared bit for bit.  Prints the seconds the torch legs took,
         from which a full run's time limit follows.
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
    nan = torch.isnan(b)
    return bool(torch.equal(torch.isnan(a), nan) and ((a.view(torch.int32) == b.view(torch.int32)) | nan).all())


def make_rows(dev, K: int, N: int, seed: int = 0):
    L = (N + 63) // 64 * 64
    rows = torch.empty((K, L), dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    for i in range(K):  # row by row: no second K x L temporary
        rows[i] = 0.05 * torch.randn(L, generator=g, device=dev)
    return rows, kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)


def check(dev) -> dict:
    res = []
    for K, keep, N in ((129, 105, 1000), (256, 192, 4099), (300, 1, 70_001), (300, 226, 70_001), (512, 384, 65_537),
                       (700, 700, 9_001), (700, 128, 9_001), (1024, 768, 40_000), (1024, 513, 40_000)):
        rows, ptrs = make_rows(dev, K, N, seed=K)
        rows[0, ::97] = float("nan")
        rows[1, ::89] = float("inf")
        rows[2, ::83] = -float("inf")
        out = torch.empty(N, dtype=torch.float32, device=dev)
        dfn.nearmedian_mean_rows_wide(ptrs, K, N, keep, out)
        ok = same(out, dfn.nearmedian_mean_rows_torch(rows[:, :N], keep))
        res.append({"K": K, "keep": keep, "N": N, "bit_identical": ok})
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


def time_shape(dev, rows, ptrs, K: int, N: int, keep: int, iters: int) -> dict:
    trim = (K - keep) // 2
    out_k = torch.empty(rows.shape[1], dtype=torch.float32, device=dev)
    out_t = torch.empty(rows.shape[1], dtype=torch.float32, device=dev)
    res = {}
    legs = {"kernel": lambda: dfn.nearmedian_mean_rows_wide(ptrs, K, N, keep, out_k),
            "trimmed_wide": lambda: dfn.trimmed_mean_rows_wide(ptrs, K, N, trim, out_t),
            "torch": lambda: res.__setitem__("t", dfn.nearmedian_mean_rows_torch(rows[:, :N], keep))}
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
    k, w, t = (_stats(ts[n]) for n in ("kernel", "trimmed_wide", "torch"))
    spread = max(k["max_ms"] - k["min_ms"], t["max_ms"] - t["min_ms"])
    nbytes = K * N * rows.element_size()
    r = {"K": K, "N": N, "keep": keep, "trim": trim, "iters": iters, "kernel": k, "trimmed_wide": w, "torch": t,
         "torch_over_kernel": round(t["median_ms"] / k["median_ms"], 2),
         "kernel_over_trimmed_wide": round(k["median_ms"] / w["median_ms"], 3),
         "larger_spread_ms": round(spread, 4),
         "kernel_wins": bool(t["median_ms"] - k["median_ms"] > spread),
         "kernel_TBps": round(nbytes / k["median_ms"] / 1e9, 3),
         "kernel_hbm_fraction": round(nbytes / k["median_ms"] / 1e9 / HBM_TBPS, 3),
         "bit_identical": same(out_k[:N], res["t"]), "torch_leg_seconds": round(torch_s, 2)}
    print(r, flush=True)
    return r


def timings(dev, cols: int, iters: int) -> dict:
    rs = []
    for K in TIME_KS:
        rows, ptrs = make_rows(dev, K, cols)
        for keep in (K - 2 * (K // 8), K):
            rs.append(time_shape(dev, rows, ptrs, K, cols, keep, iters))
        del rows, ptrs
        torch.cuda.empty_cache()
    total = sum(r["torch_leg_seconds"] for r in rs)
    print(f"torch_leg_seconds_total {total:.1f} cols {cols} rounds {iters + 1}", flush=True)
    return {"timings": rs, "timings_cols": cols, "torch_leg_seconds_total": round(total, 1)}


def main() -> int:
    def arg(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    step = arg("--step", "check")
    path = arg("--out", os.path.join(ROOT, "profiles", "nearmedian_wide_probe.json"))
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
