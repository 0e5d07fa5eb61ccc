"""Check and time the wide Gram (fedagg_pairgram2_wide_f32, pairdist2_rows'
"gram_wide") against the exact pair-distance kernel it stands beside above 128
clients (tool only).

    python tools/pairgram_wide_probe.py --step check|time|stages|pmc_run|pmc_read [--out FILE] [--cols N] [--iters I]

Every step adds its section to the JSON file (default:
profiles/pairgram_wide_probe.json; check starts it afresh), so a job script
can give each step a time limit of its own:

  check    a few small shapes, "gram_wide" against "exact" (rtol 1e-5 on these
           well-conditioned rows), symmetric, zero diagonal, non-negative;
  time     K = 256, 512, 1024 (full tiers) and 200, 384, 700 (padded) at --cols
           fp32 columns (default 4,194,304): "gram_wide" (its centre pass, the
           FedAvg kernel with weights 1/K, included), that centre pass alone and
           "exact" launched in turn on the same rows, --iters times (default
           10) after a warm-up round; the median of each with its min and max,
           the ratio, and whether the Gram wins by defense.py's rule (its
           median time is below the exact kernel's by more than the larger
           min-max spread of the two);
  stages   one whole bulyan() and one whole krum_before_aggregation() call at
           K = 1024 (f = 100) with either method, and their stages on their
           own: the bucket ingest, the distances, the host selection
           (bulyan_select, krum_scores) and Bulyan's stage 2;
  pmc_run  the workload of a counter pass: two "gram_wide" calls at K = 1024.
           Run it under `rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR
           -o b -- python tools/pairgram_wide_probe.py --step pmc_run`, with no
           tracing flags;
  pmc_read --csv DIR/.../b_counter_collection.csv: FETCH_SIZE of the wide
           kernel against K N 4 bytes, with the centre pass of the same run,
           whose traffic is known (it reads every row once), as the
           calibration of the counter.
"""
from __future__ import annotations

import csv
import json
import os
import statistics
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_KS = (256, 512, 1024, 200, 384, 700)
STAGE_K, STAGE_F = 1024, 100


def make_rows(dev, K: int, N: int, seed: int = 0):
    """A common base (0.05 randn) plus 0.01 randn per client, row by row."""
    L = (N + 63) // 64 * 64
    rows = torch.empty((K, L), dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    base = 0.05 * torch.randn(L, generator=g, device=dev)
    for i in range(K):  # row by row: no second K x L temporary
        rows[i] = base + 0.01 * torch.randn(L, generator=g, device=dev)
    return rows, kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)


def chunk_table(segs, dev):
    tab = []
    for off, n in segs:
        st = np.arange(off, off + n, nat.PAIR_CHUNK, dtype=np.int64)
        ln = np.minimum(nat.PAIR_CHUNK, off + n - st)
        tab.append(np.stack([st, ln], axis=1).ravel())
    tab = np.concatenate(tab)
    return kn.upload_i64(tab.tolist(), dev), len(tab) // 2


def check(dev) -> dict:
    res = []
    for K, N in ((129, 1000), (200, 4099), (256, 70_001), (384, 9_001), (700, 9_001), (1024, 40_000)):
        rows, ptrs = make_rows(dev, K, N, seed=K)
        chunks, n = chunk_table([(0, 1), (3, N - 3)], dev)
        Dw = dfn.pairdist2_rows(ptrs, K, chunks, n, dev, "gram_wide", length=N, aligned=True).cpu().numpy()
        De = dfn.pairdist2_rows(ptrs, K, chunks, n, dev, "exact").cpu().numpy()
        off = ~np.eye(K, dtype=bool)
        rel = float((np.abs(Dw - De)[off] / De[off]).max())
        ok = bool(rel <= 1e-5 and np.array_equal(Dw, Dw.T) and (np.diag(Dw) == 0).all() and (Dw >= 0).all())
        res.append({"K": K, "N": N, "max_rel_diff": rel, "condition": dfn.gram_condition(Dw), "ok": ok})
        print(res[-1], flush=True)
    return {"checks": res, "all_ok": all(c["ok"] for c in res)}


def _event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts) -> dict:
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def time_shape(dev, ptrs, K: int, N: int, iters: int) -> dict:
    chunks, n = chunk_table([(0, N)], dev)
    res = {}
    legs = {"gram_wide": lambda: res.__setitem__("w", dfn.pairdist2_rows(ptrs, K, chunks, n, dev, "gram_wide",
                                                                         length=N, aligned=True)),
            "centre": lambda: dfn.client_mean_row(ptrs, K, N, dev, aligned=True),
            "exact": lambda: res.__setitem__("e", dfn.pairdist2_rows(ptrs, K, chunks, n, dev, "exact"))}
    ts = {k: [] for k in legs}
    for it in range(iters + 1):  # round 0 warms every leg up
        for name, fn in legs.items():
            ms = _event_ms(fn)
            if it:
                ts[name].append(ms)
    w, c, e = (_stats(ts[k]) for k in ("gram_wide", "centre", "exact"))
    spread = max(w["max_ms"] - w["min_ms"], e["max_ms"] - e["min_ms"])
    Dw, De = res["w"].cpu().numpy(), res["e"].cpu().numpy()
    off = ~np.eye(K, dtype=bool)
    T = (K + 63) // 64
    r = {"K": K, "N": N, "iters": iters, "gram_wide": w, "centre": c, "exact": e,
         "exact_over_gram_wide": round(e["median_ms"] / w["median_ms"], 2),
         "median_gap_ms": round(e["median_ms"] - w["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "gram_wide_wins": bool(e["median_ms"] - w["median_ms"] > spread),
         "rows_GB": round(K * N * 4 / 1e9, 3),
         # each 64-row panel is read by the T + 1 tile pairs that hold it (twice by none: a diagonal pair stages it once)
         "panel_reads": T + 1,
         "gram_wide_row_TBps_counting_rereads": round((T + 1) * K * N * 4 / (w["median_ms"] - c["median_ms"]) / 1e9, 2),
         "max_rel_diff": float((np.abs(Dw - De)[off] / De[off]).max()), "condition": dfn.gram_condition(Dw)}
    print(r, flush=True)
    return r


def timings(dev, cols: int, iters: int) -> dict:
    rs = []
    for K in TIME_KS:
        rows, ptrs = make_rows(dev, K, cols)
        rs.append(time_shape(dev, ptrs, K, cols, iters))
        del rows, ptrs
        torch.cuda.empty_cache()
    tiers = {}
    for tier, full, padded in ((256, 256, 200), (512, 512, 384), (1024, 1024, 700)):
        tiers[str(tier)] = all(r["gram_wide_wins"] for r in rs if r["K"] in (full, padded))
    return {"timings": rs, "timings_cols": cols, "tiers": tiers}


def _wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 2)


def stages(dev, cols: int) -> dict:
    """The whole calls and their stages at K = 1024: one weight key of `cols`
    columns per client, the clients' tensors views of one allocation."""
    K, f = STAGE_K, STAGE_F
    rows, _ = make_rows(dev, K, cols, seed=5)
    raw = [(1, OrderedDict([("w", rows[i, :cols])])) for i in range(K)]
    out = {"K": K, "f": f, "N": cols, "theta": K - 2 * f, "beta": K - 4 * f}
    for method in ("gram_wide", "exact"):
        for rep in range(2):  # the second call: allocator and kernels warm
            out[f"bulyan_{method}_ms"] = _wall_ms(lambda: dfn.bulyan(raw, f, dev, method=method))
            out[f"krum_{method}_ms"] = _wall_ms(lambda: dfn.krum_before_aggregation(raw, f, 1, dev, method=method))
    hold = {}
    out["ingest_ms"] = _wall_ms(lambda: hold.__setitem__("b", dfn._weight_bucket([d for _, d in raw], "krum", dev)))
    bucket, g, _, _ = hold["b"]
    chunks, n = dfn.weight_chunks(g, nat.PAIR_CHUNK, dev)
    for method in ("gram_wide", "exact"):
        for rep in range(2):
            out[f"distances_{method}_ms"] = _wall_ms(lambda: hold.__setitem__("D", dfn.pairdist2_rows(
                g.d_ptrs, K, chunks, n, dev, method, length=g.length, aligned=True).cpu().numpy()))
    D = hold["D"]
    out["krum_scores_ms"] = _wall_ms(lambda: dfn.krum_scores(D, f))
    out["krum_scores_loop_ms"] = _wall_ms(lambda: dfn.krum_scores_loop(D, f))
    out["bulyan_select_ms"] = _wall_ms(lambda: hold.__setitem__("s", dfn.bulyan_select(D, f)))
    selected = hold["s"][0]
    ptrs = kn.upload_i64([g.rows[i].data_ptr() for i in selected], dev)
    row = torch.zeros(g.padded, dtype=torch.float32, device=dev)
    for rep in range(2):
        out["stage2_ms"] = _wall_ms(lambda: dfn.nearmedian_mean_rows_wide(ptrs, K - 2 * f, g.length, K - 4 * f, row))
    print(out, flush=True)
    return {"stages": out}


def pmc_run(dev, cols: int) -> dict:
    K = 1024
    rows, ptrs = make_rows(dev, K, cols)
    chunks, n = chunk_table([(0, cols)], dev)
    for _ in range(2):
        dfn.pairdist2_rows(ptrs, K, chunks, n, dev, "gram_wide", length=cols, aligned=True)
    torch.cuda.synchronize()
    return {}


def pmc_read(path: str, cols: int) -> dict:
    K = 1024
    by = {}
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == "FETCH_SIZE":
            by.setdefault(r["Kernel_Name"], []).append(float(r["Counter_Value"]))
    wide = next(v for k, v in by.items() if "pairgram_wide_kernel" in k)
    alg = K * cols * 4
    # the centre pass: the FedAvg kernel, the other launch that reads every row (exactly once)
    centre = max((v for k, v in by.items() if "pairgram" not in k and "gram_" not in k),
                 key=lambda v: statistics.median(v))
    wk, ck = statistics.median(wide) * 1024, statistics.median(centre) * 1024
    T = (K + 63) // 64
    out = {"K": K, "N": cols, "rows_bytes": alg, "FETCH_SIZE_bytes_wide_kernel": wk,
           "FETCH_SIZE_bytes_centre_pass": ck, "launches": [len(wide), len(centre)],
           "centre_pass_over_rows": round(ck / alg, 4), "wide_kernel_over_rows": round(wk / alg, 4),
           "wide_kernel_over_centre_pass": round(wk / ck, 3), "panel_reads_issued": T + 1}
    print(out, flush=True)
    return {"pmc": out}


def main() -> int:
    def arg(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    step = arg("--step", "check")
    path = arg("--out", os.path.join(ROOT, "profiles", "pairgram_wide_probe.json"))
    cols = int(arg("--cols", 4_194_304))
    summary = {}
    if os.path.exists(path) and step != "check":  # check, the first step, starts the file afresh
        with open(path) as f:
            summary = json.load(f)
    if step == "pmc_read":
        part = pmc_read(arg("--csv", ""), cols)
    else:
        dev = torch.device("cuda:0")
        summary["device"] = torch.cuda.get_device_name(dev)
        if step == "check":
            part = check(dev)
        elif step == "time":
            part = timings(dev, cols, int(arg("--iters", 10)))
        elif step == "stages":
            part = stages(dev, cols)
        elif step == "pmc_run":
            pmc_run(dev, cols)
            return 0
        else:
            raise SystemExit(f"unknown step {step!r}")
    summary.update(part)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    return 0 if part.get("all_ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
