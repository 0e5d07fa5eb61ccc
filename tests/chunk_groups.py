"""Helpers of the chunk-group tests (test_chunk_groups.py on the CPU,
test_gpu_chunk_groups.py on the device) of the distance kernels in
csrc/robust.hip and csrc/geomed.hip.

A block of those kernels owns the chunks g, g + G, ... of the chunk table and
writes one partial per chunk group g; a finish kernel sums the G partials.
Every entry point clamps G to work_len / (doubles per group), so a caller
chooses G through the workspace length it passes.  This module has the tables
of many tiny chunks that give G in the hundreds at a few thousand columns, the
workspace arithmetic that turns a wanted G into a work_len, and the numpy
references the device results are compared with.
"""
from __future__ import annotations

import numpy as np

from fedml_amd import _native as nat

PAIR_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)   # chunk lengths around the 64-column stage
DIST_EDGES = PAIR_EDGES + (257, 1023, 1024)                # ... and around dist2's 256-column lane rounds
EDGE_CYCLES = 3          # times the table's first chunks walk the edge set
MAX_TABLE_COLUMNS = 16384

# chunk-group counts that meet the empty, one-trip and two-trip 32-stride body
# of the quartered finishes (tri_finish, pair_finish, gram_sum) with every
# count of their predicated tail, and the 256-stride loop of sum_rows /
# wd_finish with one, two and three trips
QUARTERED_G = (1, 2, 3, 4, 5, 28, 29, 32, 33, 36, 61, 64, 65, 70)
STRIDE256_G = (1, 2, 3, 255, 256, 257, 513)
QUARTERED_CHUNKS = 71    # not a multiple of most G: blocks own unequal chunk counts
STRIDE256_CHUNKS = 600


def tiny_chunk_table(chunk_max: int, n_chunks: int, seed: int):
    """-> (table, cols): n_chunks disjoint (start, length) pairs in increasing
    order as an (n_chunks, 2) int64 array, and the flat index of their columns.
    The first EDGE_CYCLES * len(edges) lengths walk the edge set of the chunk
    size, each cycle rotated by one, so every length sits at the start and in
    the middle of some block's stream; the rest are 1 .. 8 columns.  Gaps of
    0 .. 3 columns put the starts at every alignment mod 4."""
    if chunk_max == nat.PAIR_CHUNK:
        edges = PAIR_EDGES
    elif chunk_max == nat.DIST_CHUNK:
        edges = DIST_EDGES
    else:
        raise ValueError(f"chunk size {chunk_max}: PAIR_CHUNK or DIST_CHUNK")
    rng = np.random.default_rng(seed)
    n_edge = min(n_chunks, EDGE_CYCLES * len(edges))
    lengths = [edges[(k + k // len(edges)) % len(edges)] for k in range(n_edge)]
    lengths += [int(v) for v in rng.integers(1, 9, n_chunks - n_edge)]
    gaps = [int(v) for v in rng.integers(0, 4, n_chunks)]
    table, start = [], 0
    for n, gap in zip(lengths, gaps):
        start += gap
        table.append((start, n))
        start += n
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    cols = np.concatenate([np.arange(s, s + n) for s, n in table]) if n_chunks else np.zeros(0, np.int64)
    return table, cols


# ---- workspace doubles per chunk group (csrc/robust.hip, csrc/geomed.hip) --------

def tri_blocks(K: int) -> int:
    nb = (K + 3) // 4
    return nb * (nb + 1) // 2


def pair_tiles(K: int) -> int:
    T = (K + 63) // 64
    return T * (T + 1) // 2


def gram_tiles(K: int) -> int:
    nb = (K + 15) // 16
    return nb * (nb + 1) // 2


def per_group(kind: int, K: int) -> int:
    if kind in (nat.WORK_DIST2, nat.WORK_WSUM_DIST2):
        return K
    if kind == nat.WORK_PAIRDIST2:
        return 16 * tri_blocks(K) if K <= 128 else pair_tiles(K) * 4096
    if kind == nat.WORK_PAIRGRAM:
        return 256 * gram_tiles(K)
    raise ValueError(kind)


def fixed_extra(kind: int, K: int) -> int:
    """doubles after the G groups: the Gram's K x K matrix M"""
    return K * K if kind == nat.WORK_PAIRGRAM else 0


def group_cap(kind: int, K: int) -> int:
    """the G a full workspace gives a long table"""
    if kind == nat.WORK_PAIRGRAM:
        return 256
    if kind == nat.WORK_PAIRDIST2 and K > 128:
        return -(-4096 // pair_tiles(K))
    return 1024


def default_work(kind: int, K: int, n_chunks: int) -> int:
    """fedagg_robust_work_len(kind, K, n_chunks), n_chunks >= 1"""
    return per_group(kind, K) * min(n_chunks, group_cap(kind, K)) + fixed_extra(kind, K)


def forced_work(kind: int, K: int, G: int) -> int:
    """The work_len that makes a call on a table of >= G chunks run exactly G
    chunk groups (G <= group_cap)."""
    if not 1 <= G <= group_cap(kind, K):
        raise ValueError(f"G = {G} outside [1, {group_cap(kind, K)}]")
    return per_group(kind, K) * G + fixed_extra(kind, K)


# ---- references -------------------------------------------------------------------

def np_pair(rows: np.ndarray, cols) -> np.ndarray:
    """K x K fp64 sums of the squared fp32 differences over cols."""
    X = rows[:, cols]
    K = X.shape[0]
    D = np.zeros((K, K))
    for i in range(K):
        d = (X[i][None, :] - X).astype(np.float32).astype(np.float64)
        D[i] = (d * d).sum(axis=1)
    return D


def np_dist2(rows: np.ndarray, ref, cols) -> np.ndarray:
    """fp64 sums of the squared fp32 differences to ref (None: norms) over cols."""
    X = rows[:, cols]
    r = ref[cols] if ref is not None else np.zeros(len(cols), np.float32)
    d = (X - r[None, :]).astype(np.float32).astype(np.float64)
    return (d * d).sum(axis=1)


def int_pair(rows: np.ndarray, cols) -> np.ndarray:
    """np_pair for integer-valued rows, in integer arithmetic: exact."""
    X = rows[:, cols].astype(np.int64)
    assert (X == rows[:, cols]).all()
    n = (X * X).sum(axis=1)
    return (n[:, None] + n[None, :] - 2 * (X @ X.T)).astype(np.float64)


def int_dist2(rows: np.ndarray, ref, cols) -> np.ndarray:
    X = rows[:, cols].astype(np.int64)
    assert (X == rows[:, cols]).all()
    if ref is not None:
        r = ref[cols].astype(np.int64)
        assert (r == ref[cols]).all()
        X = X - r[None, :]
    return (X * X).sum(axis=1).astype(np.float64)


def np_clip(x: np.ndarray, r: np.ndarray, c) -> np.ndarray:
    """fl(fl(fl(x - r) / c) + r): the clipped rebuild's three roundings."""
    with np.errstate(all="ignore"):
        d = (x - r).astype(np.float32)
        q = (d / np.float32(c)).astype(np.float32)
        return (q + r).astype(np.float32)


def np_scale(x: np.ndarray, r: np.ndarray, s) -> np.ndarray:
    """fl(fl(x - r) * s): CClip's two roundings."""
    with np.errstate(all="ignore"):
        d = (x - r).astype(np.float32)
        return (d * np.float32(s)).astype(np.float32)


def gaussian_rows(K: int, L: int, seed: int, outliers=()) -> np.ndarray:
    """A common base (0.05 randn) plus 0.01 randn per client, as the rows of
    test_gpu_dist_defenses.py; the outliers scaled by 3."""
    rng = np.random.default_rng(seed)
    base = 0.05 * rng.standard_normal(L)
    rows = (base[None, :] + 0.01 * rng.standard_normal((K, L))).astype(np.float32)
    for i in outliers:
        rows[i] *= np.float32(3.0)
    return rows


def integer_rows(K: int, L: int, seed: int, lo: int, hi: int) -> np.ndarray:
    """fp32 rows of integers in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, (K, L)).astype(np.float32)


def clip_shifts(K: int, case: int):
    """(source shifts, destination shifts, reference shift) of a clip / scale
    case, each 0 .. 3 elements: over the clients of one call (K >= 8) and over
    consecutive cases every pairing of an aligned or unaligned load with an
    aligned or unaligned store occurs."""
    src = [(i + case) % 4 for i in range(K)]
    dst = [(i + i // 4 + case // 4) % 4 for i in range(K)]
    return src, dst, (case // 3) % 4


# ---- device rows ------------------------------------------------------------------

def shifted_rows(rows_np: np.ndarray, shifts, dev, fill: float = 0.0):
    """-> (buffer, views): K device views holding rows_np's rows, row i
    starting shifts[i] elements past a 256-byte boundary, so one call sees
    rows of different alignment.  The rest of the (K, padded) buffer holds
    `fill`."""
    import torch

    K, L = rows_np.shape
    assert len(shifts) == K and all(0 <= s < 64 for s in shifts)
    buf = torch.full((K, (L + 64 + 63) // 64 * 64), fill, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 256 == 0
    src = torch.from_numpy(np.ascontiguousarray(rows_np)).to(dev)
    views = []
    for i, s in enumerate(shifts):
        v = buf[i, s:s + L]
        v.copy_(src[i])
        assert v.data_ptr() % 256 == 4 * s
        views.append(v)
    return buf, views
