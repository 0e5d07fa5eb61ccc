"""Time the wide fused Weiszfeld step against the two-pass path (tool only).

    python tools/geomed_wide_probe.py [--out FILE] [--quick]   # default: profiles/geomed_wide_probe.json

One Weiszfeld pass at 4,194,304 columns, for fp32, bf16 and f16 rows, at the
full and one padded K of each tier of the wide kernel (256 / 200, 512 / 384,
1024 / 700): fedagg_wsum_dist2_wide_f32 / _16 against what geometric_median
runs above 128 clients without it, weiszfeld_step_unfused (fedagg_wsum_f32,
then fedagg_dist2_f32) -- for 16-bit rows on the widened fp32 copy of the same
rows, whose one-off widening (K rows, a torch copy) is timed separately.  The
two are launched alternately in the same process, median of 10 after warm-up,
min and max.  z is compared bit for bit and D to 1e-12 relative at every shape
timed.

The rule of defense.GEOMED_AUTO_FUSED is evaluated per dtype and tier: the wide
kernel wins a tier only where the pair's median exceeds its median by more
than the larger of the two min-max spreads, at the full K and at the padded K.
"auto" does not take the wide kernel either way; the verdicts are what a
follow-up would route it by.  --quick: one tenth of the columns.
"""
from __future__ import annotations

import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402
from geomed16_probe import RUNS, stats, timed_pair  # noqa: E402

TIERS = {256: 200, 512: 384, 1024: 700}  # tier -> its padded K
KMAX = max(TIERS)


def one(rows, rows32, K: int, N: int, chunks, n_chunks, dev) -> dict:
    pw = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    p32 = kn.upload_i64([rows32[i].data_ptr() for i in range(K)], dev)
    w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
    zw = torch.zeros(rows32.shape[1], dtype=torch.float32, device=dev)
    zp = torch.zeros_like(zw)

    def wide():
        return dfn.wsum_dist2_rows_wide(pw, w, K, chunks, n_chunks, zw, dev, dtype=rows.dtype)

    def pair():
        return dfn.weiszfeld_step_unfused(p32, w, K, N, chunks, n_chunks, zp, dev, aligned=True)

    Dw, Dp = wide(), pair()
    same = bool(torch.equal(zw[:N].view(torch.int32), zp[:N].view(torch.int32)))
    rel = float(((Dw - Dp).abs() / Dp).max())
    a, b = (stats(t) for t in timed_pair(wide, pair))
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    r = {"K": K, "N": N, "wide": a, "pair": b, "pair_over_wide": round(b["median_ms"] / a["median_ms"], 3),
         "wide_TBps": round(K * N * rows.element_size() / a["median_ms"] / 1e9, 3),
         "pair_TBps": round(2 * K * N * 4 / b["median_ms"] / 1e9, 3),
         "gap_ms": round(b["median_ms"] - a["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "wins": bool(b["median_ms"] - a["median_ms"] > spread), "z_bit_identical": same, "D_max_rel_diff": rel,
         "ok": same and rel <= 1e-12}
    print(str(rows.dtype), r, flush=True)
    return r


def main():
    dev = torch.device("cuda:0")
    N = 4_194_304 // (10 if "--quick" in sys.argv else 1)
    L = (N + 63) // 64 * 64
    g = types.SimpleNamespace(keys=["k.weight"], offsets=[0], numels=[N])
    chunks, n_chunks = dfn.weight_chunks(g, nat.DIST_CHUNK, dev)
    summary = {"device": torch.cuda.get_device_name(dev), "columns": N, "runs_each": RUNS, "dtypes": {}}
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.randn(L, generator=gen, device=dev)
    rows32 = torch.empty((KMAX, L), dtype=torch.float32, device=dev)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        rows = rows32 if dt == torch.float32 else torch.empty((KMAX, L), dtype=dt, device=dev)
        for i in range(KMAX):  # honest clients around a common point, row by row
            rows[i] = (base + 0.05 * torch.randn(L, generator=gen, device=dev)).to(dt)
        res = {"timings": []}
        if dt != torch.float32:
            tw, _ = timed_pair(lambda: rows32.copy_(rows), lambda: None)  # the pair's one-off copy, 1024 rows
            res["widen_1024_rows"] = stats(tw)
            print(str(dt), "widen", res["widen_1024_rows"], flush=True)
        for tier, padded in TIERS.items():
            for K in (tier, padded):
                res["timings"].append(one(rows, rows32, K, N, chunks, n_chunks, dev))
        res["wins_by_rule"] = {str(t): all(r["wins"] for r in res["timings"] if r["K"] in (t, p))
                               for t, p in TIERS.items()}
        summary["dtypes"][str(dt)] = res
        del rows
    summary["all_checks_ok"] = all(r["ok"] for d in summary["dtypes"].values() for r in d["timings"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "geomed_wide_probe.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps({k: v["wins_by_rule"] for k, v in summary["dtypes"].items()}))
    return 0 if summary["all_checks_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
