"""Time one round's history update and Gram of the "foolsgold_cos" defense on
a bf16 / f16 model: the fused 16-bit kernel (fedagg_histgram_16,
csrc/histgram16.hip) beside the composed 16-bit path, which is what "auto" runs
otherwise (defense.histgram_rows_composed on the 16-bit rows: the torch update
widening them, then pairdist2_rows about a zero centre and dist2_rows on the
fp32 histories), and beside fedagg_histgram_f32 on a widened fp32 copy of the
same rows (tool only; foolsgold_probe.py is the fp32 model's).

    python tools/foolsgold16_probe.py --dtype bf16|f16 --k K [--out FILE] [--cols N] [--iters I]

One run times one dtype and one K (128, and the padded 100) at --cols columns
(default 4,194,304) of "base + small update" rows rounded to the dtype and
gaussian fp32 histories; the result joins the others in
profiles/foolsgold16_probe.json.  The three legs are launched alternately on
the same rows, --iters times (default 10) after a warm-up round, each between
two device events; the histories are restored from a saved copy before every
launch (outside the timed span).  Recorded: the median of each leg with its
min and max, whether the fused kernel wins by defense.py's rule (the composed
median above the fused one by more than the larger min-max spread of the two),
the fused kernel's time over the fp32 kernel's on the widened copy (below 1:
the 16-bit loads save time, not only the copy), its achieved bytes per second
against its 10 K N-byte model, and the largest cosine difference between the
fused and the composed Gram.  "auto" is HISTGRAM16_AUTO's entry per dtype: True
only if K = 128 and K = 100 are both there and both win.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fedml_amd import _native as nat  # noqa: E402
from fedml_amd import defense as dfn  # noqa: E402
from fedml_amd import kernels as kn  # noqa: E402
from foolsgold_probe import ROOT, _event_ms, _stats  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def time_run(dev, name: str, K: int, N: int, iters: int) -> dict:
    dt = DTYPES[name]
    g = torch.Generator(device=dev).manual_seed(K)
    ref = (0.05 * torch.randn(N, generator=g, device=dev)).to(dt)
    rows = torch.empty((K, N), dtype=dt, device=dev)
    hist0 = torch.empty((K, N), dtype=torch.float32, device=dev)
    for i in range(K):
        rows[i] = ref.float() + 0.01 * torch.randn(N, generator=g, device=dev)
        hist0[i] = 0.02 * torch.randn(N, generator=g, device=dev)
    hist = hist0.clone()
    rows32, ref32 = rows.float(), ref.float()  # the copy a caller without the 16-bit kernel would have to make
    zero = torch.zeros(N, dtype=torch.float32, device=dev)
    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    ptrs32 = kn.upload_i64([rows32[i].data_ptr() for i in range(K)], dev)
    hptrs = kn.upload_i64([hist[i].data_ptr() for i in range(K)], dev)
    st = np.arange(0, N, nat.PAIR_CHUNK, dtype=np.int64)
    tab = np.stack([st, np.minimum(nat.PAIR_CHUNK, N - st)], axis=1).ravel()
    chunks, n = kn.upload_i64(tab.tolist(), dev), len(st)
    res = {}
    legs = {"fused": lambda: res.__setitem__("f", dfn.histgram_rows(ptrs, K, ref, hptrs, chunks, n, dev)),
            "composed": lambda: res.__setitem__("c", dfn.histgram_rows_composed(rows, ref, hist, None, hptrs, K,
                                                                               [(0, N)], chunks, n, dev, zero)),
            "fp32_widened": lambda: res.__setitem__("w", dfn.histgram_rows(ptrs32, K, ref32, hptrs, chunks, n, dev))}
    ts = {k: [] for k in legs}
    for it in range(iters + 1):  # round 0 warms the legs up
        for leg, fn in legs.items():
            hist.copy_(hist0)
            ms = _event_ms(fn)
            if it:
                ts[leg].append(ms)
    f, c, w = _stats(ts["fused"]), _stats(ts["composed"]), _stats(ts["fp32_widened"])
    spread = max(f["max_ms"] - f["min_ms"], c["max_ms"] - c["min_ms"])
    Gf, Gc = res["f"].cpu().numpy(), res["c"].cpu().numpy()
    nrm = np.sqrt(np.outer(np.diag(Gc), np.diag(Gc)))
    r = {"dtype": name, "K": K, "N": N, "iters": iters, "fused": f, "composed": c, "fp32_widened": w,
         "composed_over_fused": round(c["median_ms"] / f["median_ms"], 2),
         "median_gap_ms": round(c["median_ms"] - f["median_ms"], 4), "larger_spread_ms": round(spread, 4),
         "fused_wins": bool(c["median_ms"] - f["median_ms"] > spread),
         "fused_over_fp32_widened": round(f["median_ms"] / w["median_ms"], 3),
         "fused_equals_fp32_widened": bool(np.array_equal(Gf, res["w"].cpu().numpy())),
         "model_GB": round(10 * K * N / 1e9, 3), "fused_model_TBps": round(10 * K * N / f["median_ms"] / 1e9, 2),
         "max_cosine_diff": float((np.abs(Gf - Gc) / nrm).max())}
    print(r, flush=True)
    return r


def main(argv) -> int:
    opt = {"--out": os.path.join(ROOT, "profiles", "foolsgold16_probe.json"), "--cols": "4194304", "--iters": "10",
           "--k": None, "--dtype": None}
    for i in range(0, len(argv), 2):
        if argv[i] not in opt or i + 1 >= len(argv):
            raise SystemExit(__doc__)
        opt[argv[i]] = argv[i + 1]
    if opt["--k"] is None or opt["--dtype"] not in DTYPES:
        raise SystemExit(__doc__)
    if not torch.cuda.is_available():
        raise SystemExit("foolsgold16_probe: no GPU (nothing is measured without one)")
    r = time_run(torch.device("cuda", 0), opt["--dtype"], int(opt["--k"]), int(opt["--cols"]), int(opt["--iters"]))
    rs = []
    if os.path.exists(opt["--out"]):
        with open(opt["--out"]) as f:
            rs = [t for t in json.load(f)["timings"] if (t["dtype"], t["K"], t["N"]) != (r["dtype"], r["K"], r["N"])]
    rs = sorted(rs + [r], key=lambda t: (t["dtype"], -t["K"]))
    auto = {}
    for name in DTYPES:
        mine = [t for t in rs if t["dtype"] == name]
        auto[name] = {"128": bool({128, 100} <= {t["K"] for t in mine} and all(t["fused_wins"] for t in mine))}
    os.makedirs(os.path.dirname(opt["--out"]), exist_ok=True)
    with open(opt["--out"], "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "timings": rs, "auto": auto}, f, indent=1)
        f.write("\n")
    print("auto:", auto, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
