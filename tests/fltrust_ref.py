"""numpy / Python reference of the FLTrust defense (fedml_amd.defense.fltrust),
written independently of defense.py: the fp32 differences, math.fsum of their
exact float64 products (the correctly rounded sums), the coefficient rule in
plain Python floats, and the rebuild chain in np.float32 operations (numpy
rounds every float32 operation once and keeps denormals, as the kernel).
"""
from __future__ import annotations

import math

import numpy as np

# c * d = 1 + 2^-11 + 2^-24 exactly for c = d = 1 + 2^-12: the product's fp32
# rounding drops the 2^-24 (a tie, to even), an FMA keeps it.  Added to
# -(1 + 2^-11) the rounded product gives 0 and the FMA 2^-24.
FMA_C = float(np.float32(1.0 + 2.0 ** -12))
FMA_D = np.float32(1.0 + 2.0 ** -12)
FMA_ACC = np.float32(-(1.0 + 2.0 ** -11))


def diff32(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """fl32(x - g), elementwise (overflow to inf and NaN pass through)."""
    with np.errstate(all="ignore"):
        return (np.asarray(x, dtype=np.float32) - np.asarray(g, dtype=np.float32)).astype(np.float32)


def fsum_products(a: np.ndarray, b: np.ndarray):
    """-> (math.fsum of the float64 products a[e] * b[e], the sum of their
    magnitudes): a product of two fp32 values is exact in float64.  A
    non-finite product gives (nan, nan)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    if not np.isfinite(p).all():
        return float("nan"), float("nan")
    return math.fsum(p.tolist()), math.fsum(np.abs(p).tolist())


def dot_norm(rows, g: np.ndarray, r: np.ndarray, cols=None):
    """The K clients' (dot, n2) and the root's nb2 over cols (None: all), each
    with the sum of its terms' magnitudes: -> (dot, dot_abs, n2, nb2), lists of
    K floats and one float (n2 and nb2 are their own magnitude sums)."""
    sel = slice(None) if cols is None else np.asarray(cols)
    gs = np.asarray(g, dtype=np.float32)[sel]
    b = diff32(np.asarray(r, dtype=np.float32)[sel], gs)
    nb2, _ = fsum_products(b, b)
    dot, dot_abs, n2 = [], [], []
    for x in rows:
        a = diff32(np.asarray(x, dtype=np.float32)[sel], gs)
        d, da = fsum_products(a, b)
        n, _ = fsum_products(a, a)
        dot.append(d)
        dot_abs.append(da)
        n2.append(n)
    return dot, dot_abs, n2, nb2


def coeffs(dot, n2, nb2, lr: float = 1.0):
    """The coefficient rule in Python floats: -> (cos, trust, c), lists of K.
    cos_i = dot_i / (sqrt(n2_i) sqrt(nb2)), nan where that is not a number;
    trust_i = cos_i where finite and positive, else 0; S their sum from left
    to right; c_i = lr trust_i sqrt(nb2) / (sqrt(n2_i) S), all 0 when S is 0.
    ValueError unless nb2 is finite and positive."""
    nb2 = float(nb2)
    if not (math.isfinite(nb2) and nb2 > 0.0):
        raise ValueError(f"root update with squared norm {nb2}")
    nb = math.sqrt(nb2)
    cos, trust, norms = [], [], []
    for d, s in zip(dot, n2):
        d, s = float(d), float(s)
        n = math.sqrt(s)  # nan for nan, inf for inf
        norms.append(n)
        try:
            v = d / (n * nb)  # nan for nan operands and inf / inf
        except ZeroDivisionError:  # a client that did not move
            v = float("nan")
        cos.append(v)
        trust.append(v if math.isfinite(v) and v > 0.0 else 0.0)
    S = 0.0
    for t in trust:
        S = S + t
    c = [0.0] * len(trust)
    if S != 0.0:
        for i, t in enumerate(trust):
            if t > 0.0:
                c[i] = lr * t * nb / (norms[i] * S)
    return cos, trust, c


def rebuild(rows, c32, g: np.ndarray) -> np.ndarray:
    """fl(g + chain) with acc = fl(c_0 fl(x_0 - g)), acc = fl(acc + fl(c_i
    fl(x_i - g))): every operation one np.float32 rounding; g itself for no
    rows."""
    g = np.asarray(g, dtype=np.float32)
    if len(rows) == 0:
        return g.copy()
    with np.errstate(all="ignore"):
        acc = None
        for x, c in zip(rows, c32):
            term = (diff32(x, g) * np.float32(c)).astype(np.float32)
            acc = term if acc is None else (acc + term).astype(np.float32)
        return (g + acc).astype(np.float32)


def fma_chain_value(acc: np.float32, c: float, d: np.float32) -> np.float32:
    """What a fused multiply-add would give for acc + c * d: the exact product
    (float64 holds it) added to acc, rounded once to fp32.  For the constants
    above the float64 sum is exact too, so this is the FMA's result."""
    return np.float32(np.float64(np.float32(c)) * np.float64(d) + np.float64(acc))


def fltrust(rows_all, g_all: np.ndarray, r_all: np.ndarray, wcols, lr: float = 1.0):
    """The whole rule on flat fp32 rows: cosines over wcols, the rebuild over
    every column with the trusted clients in ascending order.
    -> (out, cos, trust, c32, trusted)."""
    dot, _, n2, nb2 = dot_norm(rows_all, g_all, r_all, wcols)
    cos, trust, c = coeffs(dot, n2, nb2, lr)
    trusted = [i for i, t in enumerate(trust) if t > 0.0]
    c32 = [float(np.float32(v)) for v in c]
    out = rebuild([rows_all[i] for i in trusted], [c32[i] for i in trusted], g_all)
    return out, cos, trust, c32, trusted
