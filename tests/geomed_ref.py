"""numpy reference of the "geomed" defense (fedml_amd.defense.geometric_median):
the smoothed Weiszfeld iteration as include/fedagg.h and geometric_median_loop
specify it, written independently of the package's code.

    w = a                                   a_i = n_i / sum(n)
    for t = 0, 1, ...:
        z_t = chain(rows, fl32(w))          fp32: fl(x_0 w_0), fl(acc + fl(x_i w_i))
        D_i = sum_e double(fl32(x_i[e] - z_t[e]))^2      over the columns that count
        f_t = sum_i a_i sqrt(D_i)           float64, left to right
        stop if t == maxiter or (t >= 1 and |f_{t-1} - f_t| <= ftol f_t)
        b_i = a_i / max(nu, sqrt(D_i)); w_i = b_i / sum(b)   left to right
"""
from __future__ import annotations

import numpy as np

MAX_NORM2 = 2.0 ** 252


def chain(rows: np.ndarray, w32) -> np.ndarray:
    """The FedAvg chain in fp32: two roundings per client, clients in order."""
    w = np.asarray(w32, dtype=np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        acc = rows[0] * w[0]
        for i in range(1, len(rows)):
            acc = acc + rows[i] * w[i]
    return acc


def dist2(rows: np.ndarray, z: np.ndarray, cols=None) -> np.ndarray:
    sl = slice(None) if cols is None else cols
    with np.errstate(all="ignore"):
        return np.array([(((r[sl] - z[sl]).astype(np.float64)) ** 2).sum() for r in rows], dtype=np.float64)


def step(rows: np.ndarray, w32, cols=None):
    z = chain(rows, w32)
    return z, dist2(rows, z, cols)


def weights(D, a, nu: float) -> np.ndarray:
    b = np.asarray(a, dtype=np.float64) / np.maximum(nu, np.sqrt(np.asarray(D, dtype=np.float64)))
    total = np.float64(0.0)
    for x in b:
        total = total + x
    return b / total


def loop(rows: np.ndarray, a, nu: float = 1e-6, maxiter: int = 16, ftol: float = 1e-6, cols=None):
    """-> (z_T, w_T, [f_0 .. f_T])"""
    a = np.asarray(a, dtype=np.float64)
    w = a.copy()
    fs = []
    t = 0
    while True:
        z, D = step(rows, w.astype(np.float32), cols)
        f = np.float64(0.0)
        for ai, di in zip(a, np.sqrt(D)):
            f = f + ai * di
        fs.append(float(f))
        if t == maxiter or (t >= 1 and abs(fs[-2] - fs[-1]) <= ftol * fs[-1]):
            return z, w, fs
        w = weights(D, a, nu)
        t += 1


def screen(rows: np.ndarray, cols=None) -> list:
    """Clients the lazy screen drops: squared norm non-finite or above 2^252."""
    n2 = dist2(rows, np.zeros_like(rows[0]), cols)
    return [i for i in range(len(rows)) if not np.isfinite(n2[i]) or n2[i] > MAX_NORM2]


ROBUST_CASES = [(9, 2), (16, 5), (33, 16), (128, 40)]  # (clients, corrupted)
ROBUST_N = 4099


def robust_clients(K: int, bad: int, seed: int = 0, N: int = ROBUST_N):
    """The robustness inputs: honest rows m + 0.05 randn around a common m,
    corrupted rows 1e4 randn, sample counts random in [50, 150).
    -> (rows fp32 (K, N), counts, indices of the corrupted clients)"""
    rng = np.random.default_rng(1000 * K + seed)
    m = rng.standard_normal(N)
    rows = (m + 0.05 * rng.standard_normal((K, N))).astype(np.float32)
    corrupted = sorted(rng.choice(K, size=bad, replace=False).tolist())
    for i in corrupted:
        rows[i] = (1e4 * rng.standard_normal(N)).astype(np.float32)
    counts = [int(v) for v in rng.integers(50, 150, K)]
    return rows, counts, corrupted


def robust_check(z: np.ndarray, w, rows: np.ndarray, corrupted, cols=None) -> dict:
    """The two robustness figures: |z - honest mean| over the largest honest
    distance to the honest mean (must be < 1), and the corrupted clients'
    final weight (must be < 1e-4)."""
    sl = slice(None) if cols is None else cols
    honest = [i for i in range(len(rows)) if i not in set(corrupted)]
    h = rows[honest][:, sl].astype(np.float64)
    mean = h.mean(axis=0)
    radius = max(float(np.linalg.norm(r - mean)) for r in h)
    off = float(np.linalg.norm(np.asarray(z, dtype=np.float64)[sl] - mean))
    return {"ratio": off / radius, "corrupted_weight": float(sum(np.asarray(w, dtype=np.float64)[corrupted]))}
