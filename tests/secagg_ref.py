"""Reference of the LightSecAgg field kernels (fedagg_sum_mod_i64,
fedagg_lsa_reconstruct_f32) for test_secagg_ref.py and test_gpu_secagg.py (no
tests here).

ref_sum and ref_reconstruct restate include/fedagg.h in Python integers, one
column at a time.  Every int64 wrap is written out (wrap), the modulo is
Python's own floor modulo, and the float64 steps are Python floats, so nothing
here depends on numpy's int64 behaviour.  That is affordable up to a few
hundred thousand chain steps; above that the tests use the numpy oracle, which
test_secagg_ref.py pins to this file.

The rest builds the inputs both test files share: the moduli, the directed
columns and the seeded random columns (half field elements, half full-range
int64)."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# 32749 and 2^31-1 are the primes the project ships with; 2^53+1 and 2^53+3 are
# the first moduli whose (p-1)/2 is no float64; 2^61-1 is a Mersenne prime below
# the conditional-subtract bound 2^62, 2^62 sits on it, 2^62+1 is the first
# modulus past it (a + x can pass 2^63) and 2^63-25 is the largest int64 prime.
MODULI = [32749, 2 ** 31 - 1, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 61 - 1, 2 ** 62, 2 ** 62 + 1, 2 ** 63 - 25]
Q_BITS = [0, 10, 16, 62]


def wrap(v: int) -> int:
    """v as a two's complement int64."""
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def ref_sum(cols, p: int) -> list:
    """cols: N columns of K Python ints -> N ints: a = x_0; a = wrap(a + x_i) mod p."""
    out = []
    for col in cols:
        a = col[0]
        for x in col[1:]:
            a = wrap(a + x) % p  # p > 0: Python's % is the floor modulo
        out.append(a)
    return out


def ref_reconstruct(cols, mask, p: int, q: int, K: int) -> np.ndarray:
    """cols: N columns of Python ints, mask: N ints -> (N,) float32:
    m = wrap(wrapped sum - mask) mod p, its signed value in float64 over 2^q
    rounded to fp32, times fl32(1 / K) in fp32."""
    half = (p - 1) / 2  # int / int: the correctly rounded quotient
    w = np.float32(1 / K)
    out = np.empty(len(cols), dtype=np.float32)
    for j, col in enumerate(cols):
        s = col[0]
        for x in col[1:]:
            s = wrap(s + x)
        m = wrap(s - mask[j]) % p
        xq = float(m)
        v = xq - float(p) if xq - half > 0 else xq
        out[j] = np.float32(v / 2.0 ** q) * w
    return out


def columns(x: np.ndarray) -> list:
    """(K, N) int64 -> N columns of K Python ints."""
    return np.asarray(x).T.tolist()


def directed_sum(K: int, p: int) -> list:
    """Columns (K ints each) aimed at the branches of the modular step."""
    a = p // 3 + 2

    def pair(total):  # a + x = total at client 1, zeros after; K = 1 keeps a alone
        return ([a, total - a] + [0] * K)[:K]

    share = p // K
    return [
        pair(p),      # s2 == p: the subtract must fire on equality
        pair(p - 1),  # the largest sum that stays
        pair(p + 1),
        [share] * (K - 1) + [p - (K - 1) * share],  # the running sum reaches exactly p at the last client
        [0] * K,
        [p - 1] * K,  # p > 2^62: a + x passes 2^63, the exact floor modulo of a wrapped sum
        ([I64_MAX, 1] + [0] * K)[:K],   # wraps to INT64_MIN
        ([I64_MIN, -1] + [0] * K)[:K],  # wraps to INT64_MAX
        ([p, -p, p - 1] + [-1] * K)[:K],
        ([-1, I64_MIN, I64_MAX, p] + [p - 1] * K)[:K],
        ([0] * K + [p - 1, p - 1])[-K:],  # 2^63 passed at the last client, where no later step can repair it
    ]


def directed_reconstruct(K: int, p: int):
    """(columns, mask values): every residue around the sign threshold carried
    by client 0 alone, then negative differences and wrapping sums."""
    h = (p - 1) // 2
    cols, mask = [], []
    for m in (0, 1, h - 1, h, h + 1, h + 2, p - 2, p - 1):
        cols.append([m] + [0] * (K - 1))
        mask.append(0)
    for m in (h, h + 1, h + 2):  # the same residues reached through a mask: m = (m + 7) - 7
        cols.append([m] + [0] * (K - 1))
        cols[-1][-1] += 7
        mask.append(7)
    for col, m in [
        ([5], 7),          # mask above the sum: -2 -> p - 2
        ([0], p - 1),      # -(p - 1) -> 1
        ([I64_MAX, 1], 0),  # the sum wraps
        ([I64_MAX, I64_MAX, 2], p - 1),
        ([I64_MIN], 1),    # sum - mask wraps
        ([I64_MAX], -1),
    ]:
        cols.append((col + [0] * K)[:K])
        mask.append(m)
    return cols, mask


def _random(rng, K: int, N: int, p: int) -> np.ndarray:
    """(K, N): even columns hold field elements, odd columns any int64, with the
    values np.mod gets wrong first sprinkled over them."""
    x = rng.integers(0, p, size=(K, N), dtype=np.int64)
    if N > 1:
        wild = rng.integers(I64_MIN, I64_MAX, size=(K, N // 2), dtype=np.int64, endpoint=True)
        edge = np.array([I64_MIN, I64_MAX, -1, p, -p, p - 1], dtype=np.int64)
        flat = wild.reshape(-1)  # every fifth value: another set of columns in each client's row
        flat[::5] = edge[rng.integers(0, len(edge), size=len(flat[::5]))]
        x[:, 1::2] = wild
    return x


def _place(x: np.ndarray, cols) -> int:
    """The directed columns over the first columns of x (as many as fit)."""
    n = min(len(cols), x.shape[1])
    for j in range(n):
        x[:, j] = np.array([wrap(v) for v in cols[j]], dtype=np.int64)
    return n


def sum_inputs(K: int, N: int, p: int, seed: int) -> np.ndarray:
    """(K, N) int64 client rows for fedagg_sum_mod_i64."""
    x = _random(np.random.default_rng(seed), K, N, p)
    _place(x, directed_sum(K, p))
    return x


def reconstruct_inputs(K: int, N: int, p: int, seed: int):
    """((K, N) int64 client rows, (N,) int64 mask) for fedagg_lsa_reconstruct_f32."""
    rng = np.random.default_rng(seed)
    x = _random(rng, K, N, p)
    mask = rng.integers(0, p, size=N, dtype=np.int64)
    if N > 3:
        mask[3::4] = rng.integers(I64_MIN, I64_MAX, size=len(mask[3::4]), dtype=np.int64, endpoint=True)
    cols, mk = directed_reconstruct(K, p)
    n = _place(x, cols)
    mask[:n] = np.array([wrap(v) for v in mk[:n]], dtype=np.int64)
    return x, mask


def oracle_sum(orc, x: np.ndarray, p: int) -> np.ndarray:
    """oracle.finite_sum on the rows of x as one key."""
    return orc.finite_sum([OrderedDict(k=row) for row in x], p)["k"]


def oracle_reconstruct(orc, x: np.ndarray, mask: np.ndarray, p: int, q: int) -> np.ndarray:
    """oracle.lsa_reconstruct on the rows of x as one key: (N,) float32, w = 1 / K."""
    return orc.lsa_reconstruct([OrderedDict(k=row) for row in x], mask, p, q)["k"].numpy()
