"""Reference of the "wise_bulyan" defense for test_bulyan.py and
test_gpu_bulyan.py (no tests here).

nearmedian_mean_f32 restates the specification of fedagg_nearmedian_mean_f32
(include/fedagg.h) as the LITERAL two-pointer rule, vectorised over columns:
the loop runs over the keep - 1 steps, every column carrying its own l and h.
It is deliberately not the counting form the kernel and the torch path use, so
that the two are derived independently.  bulyan_select_ref is stage 1 in plain
Python loops."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from trimmed_mean_ref import order_keys


def nearmedian_mean_f32(x: np.ndarray, keep: int) -> np.ndarray:
    """x: (K, N) float32 -> (N,) float32, the mean of the `keep` values nearest
    the lower median of every column, by the header's rule."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    K, N = x.shape
    assert 1 <= keep <= K
    idx = np.argsort(order_keys(x), axis=0, kind="stable")
    s = np.take_along_axis(x, idx, axis=0)
    nan = np.isnan(s)
    nans = nan.sum(axis=0)
    sel = np.where(nan, np.float32(np.inf), s)  # for the selection a NaN counts as +inf
    r = (K - 1) // 2
    m = sel[r]
    cols = np.arange(N)

    def d(v):
        with np.errstate(all="ignore"):
            return np.where(v == m, np.float32(0), np.abs((v - m).astype(np.float32))).astype(np.float32)

    l = np.full(N, r, dtype=np.int64)
    h = np.full(N, r, dtype=np.int64)
    for _ in range(keep - 1):
        dl = d(sel[np.maximum(l - 1, 0), cols])  # only looked at where l > 0
        dh = d(sel[np.minimum(h + 1, K - 1), cols])  # only looked at where h < K - 1
        left = (h == K - 1) | ((l > 0) & (dl <= dh))
        l = np.where(left, l - 1, l)
        h = np.where(left, h, h + 1)
    assert bool(np.all(h - l == keep - 1)) and bool(np.all(l >= 0)) and bool(np.all(h <= K - 1))
    with np.errstate(all="ignore"):
        acc = s[l, cols].copy()
        for t in range(1, keep):
            acc = (acc + s[l + t, cols]).astype(np.float32)
        out = (acc / np.float32(keep)).astype(np.float32)
    out[l + keep > K - nans] = np.float32(np.nan)
    return out


def nearmedian_mean_ref(rows: torch.Tensor, keep: int) -> torch.Tensor:
    """rows: a (K, N) fp32 tensor -> (N,) fp32, on the CPU."""
    return torch.from_numpy(nearmedian_mean_f32(rows.detach().cpu().float().numpy(), keep))


def all_columns(alphabet, K: int) -> torch.Tensor:
    """Every column of length K over `alphabet`: (K, len(alphabet) ** K) fp32."""
    a = np.asarray(alphabet, dtype=np.float32)
    grid = np.stack(np.meshgrid(*([a] * K), indexing="ij")).reshape(K, -1)
    return torch.from_numpy(np.ascontiguousarray(grid))


INF, NAN = float("inf"), float("nan")
ALPHABET9 = [-INF, -2.0, -1.0, -0.0, 0.0, 1.0, 2.0, INF, NAN]
ALPHABET5 = [-INF, -1.0, 0.0, 1.0, NAN]
ALPHABET4 = [-INF, -1.0, 1.0, NAN]


def keeps(K: int) -> list:
    """keep values 1, 2, (K+1)//2, K-1 and K, valid for K, without repeats."""
    out = []
    for k in (1, 2, (K + 1) // 2, K - 1, K):
        if 1 <= k <= K and k not in out:
            out.append(k)
    return out


def bulyan_select_ref(D, f: int, gaps=None):
    """Stage 1 in plain loops: (selected in pick order, each pick's score).
    gaps: a list that receives, per round, (next distinct score - lowest
    score) / lowest score: how far the pick is from going the other way."""
    K = len(D)
    if f == 0:
        return list(range(K)), [0.0] * K
    R = list(range(K))
    selected, scores = [], []
    for _ in range(K - 2 * f):
        n = len(R)
        best = None
        every = []
        for i in R:
            vals = [float(D[i][j]) for j in R if j != i]
            vals.sort(key=lambda v: (1, 0.0) if v != v else (0, v))  # NaN last, above +inf
            sc = 0.0
            for v in vals[:max(1, n - f - 2)]:
                sc += v
            if sc != sc:
                sc = float("inf")
            every.append(sc)
            if best is None or sc < best[0]:  # strict: equal scores keep the lowest index
                best = (sc, i)
        if gaps is not None:
            # over distinct scores: in a round that scores on one neighbour, two
            # clients nearest each other share D[i][j] itself, an exact tie in
            # any symmetric D, which goes to the lower index everywhere
            every = sorted(set(every))
            gaps.append((every[1] - every[0]) / every[0] if len(every) > 1 and every[0] > 0 else float("inf"))
        selected.append(best[1])
        scores.append(best[0])
        R.remove(best[1])
    return selected, scores


def pair_d2(rows, cols=None) -> np.ndarray:
    """K x K float64 squared distances from the fp32 differences of the rows
    ((K, N) fp32) over the columns `cols` (default: all)."""
    x = np.ascontiguousarray(torch.as_tensor(rows).detach().cpu().numpy(), dtype=np.float32)
    if cols is not None:
        x = np.ascontiguousarray(x[:, np.asarray(cols)])
    K = x.shape[0]
    D = np.zeros((K, K), dtype=np.float64)
    with np.errstate(all="ignore"):
        for i in range(K):
            for j in range(K):
                if i != j:
                    diff = (x[i] - x[j]).astype(np.float32).astype(np.float64)
                    D[i, j] = np.sum(diff * diff)
    return D


def is_weight_key(k: str) -> bool:
    return "running_mean" not in k and "running_var" not in k and "num_batches_tracked" not in k


def bulyan_ref(raw, f: int):
    """raw: [(n, OrderedDict of CPU tensors)] -> (result dict, selected,
    scores, D).  Distances over the weight keys, the window over every key;
    integer keys enter as fl32(v)."""
    dicts = [d for _, d in raw]
    K = len(dicts)
    keys = list(dicts[0].keys())
    flat = {k: torch.stack([d[k].detach().cpu().reshape(-1).float() for d in dicts]) for k in keys}
    wrows = torch.cat([flat[k] for k in keys if is_weight_key(k)], dim=1)
    D = pair_d2(wrows)
    selected, scores = bulyan_select_ref(D, f)
    beta = K - 4 * f
    out = OrderedDict()
    for k in keys:
        out[k] = nearmedian_mean_ref(flat[k][selected], beta).view(dicts[0][k].shape)
    return out, selected, scores, D
