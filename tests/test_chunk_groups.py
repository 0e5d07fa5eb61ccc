"""CPU checks of tests/chunk_groups.py, which test_gpu_chunk_groups.py relies
on: the tiny-chunk tables' invariants, the per-group workspace formulas
against the library's own fedagg_robust_work_len (if one drifts, a forced G
silently stops being the intended one), the numpy references against
brute-force loops, and the exactness argument of the Gram's {-1, 0, 1} test
emulated in numpy float32."""
from __future__ import annotations

import numpy as np
import pytest

import chunk_groups as cg
import geomed_ref
from fedml_amd import _native as nat
from fedml_amd import build as fbuild

# every K test_gpu_chunk_groups.py uses, per workspace kind
DIST2_KS = [1, 5, 63, 64, 65, 128, 129, 300]
PAIR_KS = [1, 2, 4, 5, 24, 25, 28, 37, 63, 64, 65, 100, 128, 129, 192, 193, 200]
GRAM_KS = [1, 2, 3, 16, 17, 33, 48, 64, 65, 81, 96, 100, 113, 127, 128]
GRAM_EXACT_KS = [2, 4, 16, 64]
WSUM_KS = [1, 8, 9, 16, 17, 32, 33, 64, 65, 128]
CLIP_KS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17]
CLIP_NS = [1, 3, 4, 5, 1023, 1024, 1025, 2049, 5000]
KIND_KS = [(nat.WORK_DIST2, DIST2_KS), (nat.WORK_PAIRDIST2, PAIR_KS),
           (nat.WORK_PAIRGRAM, GRAM_KS + GRAM_EXACT_KS), (nat.WORK_WSUM_DIST2, WSUM_KS)]


@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


@pytest.mark.parametrize("chunk_max,n_chunks", [(nat.PAIR_CHUNK, cg.QUARTERED_CHUNKS),
                                                (nat.DIST_CHUNK, cg.STRIDE256_CHUNKS)])
def test_tiny_chunk_table_invariants(chunk_max, n_chunks):
    edges = cg.PAIR_EDGES if chunk_max == nat.PAIR_CHUNK else cg.DIST_EDGES
    for seed in (0, 1, 2):
        tab, cols = cg.tiny_chunk_table(chunk_max, n_chunks, seed)
        assert tab.shape == (n_chunks, 2) and tab.dtype == np.int64
        start, length = tab[:, 0], tab[:, 1]
        assert length.min() >= 1 and length.max() == chunk_max
        gaps = start[1:] - (start[:-1] + length[:-1])
        assert start[0] >= 0 and gaps.min() >= 0 and gaps.max() <= 3   # disjoint, in order
        assert np.array_equal(cols, np.concatenate([np.arange(s, s + n) for s, n in tab]))
        assert len(np.unique(cols)) == len(cols) == length.sum() and (np.diff(cols) > 0).all()
        assert cols[-1] < cg.MAX_TABLE_COLUMNS
        assert set(edges) <= set(length.tolist())
        assert set((start % 4).tolist()) == {0, 1, 2, 3}
        # every edge length leads the table's edge part once per cycle position:
        # at the start of a block's stream for some G, in its middle for others
        n_edge = cg.EDGE_CYCLES * len(edges)
        assert sorted(length[:n_edge].tolist()) == sorted(edges * cg.EDGE_CYCLES)
        assert length[n_edge:].max() <= 8
        again, _ = cg.tiny_chunk_table(chunk_max, n_chunks, seed)
        assert np.array_equal(tab, again)


def test_quartered_table_streams_past_a_hundred_stages():
    """At G = 1 one block streams the whole table: more than a hundred
    64-column stages, so the Gram folds mid-stream some 25 times."""
    tab, _ = cg.tiny_chunk_table(nat.PAIR_CHUNK, cg.QUARTERED_CHUNKS, 0)
    assert int(((tab[:, 1] + 63) // 64).sum()) > 100


def test_group_counts_are_reachable():
    for G in cg.QUARTERED_G:
        assert G <= cg.QUARTERED_CHUNKS
        for K in PAIR_KS:
            assert G <= cg.group_cap(nat.WORK_PAIRDIST2, K)
        assert G <= cg.group_cap(nat.WORK_PAIRGRAM, 128)
    for G in cg.STRIDE256_G:
        assert G <= cg.STRIDE256_CHUNKS and G <= cg.group_cap(nat.WORK_DIST2, 1)
    with pytest.raises(ValueError):
        cg.forced_work(nat.WORK_PAIRGRAM, 16, 257)


@pytest.mark.parametrize("kind,ks", KIND_KS)
def test_workspace_formulas_match_the_library(kind, ks, lib):
    for K in ks:
        for n in (1, 2, 19, 257, 1100):
            assert lib.fedagg_robust_work_len(kind, K, n) == cg.default_work(kind, K, n), (kind, K, n)
        for G in (1, 3, 70):
            assert cg.forced_work(kind, K, G) == G * cg.per_group(kind, K) + cg.fixed_extra(kind, K)
    assert cg.fixed_extra(nat.WORK_PAIRGRAM, 7) == 49 and cg.fixed_extra(nat.WORK_DIST2, 7) == 0


def test_clip_shift_schedule_mixes_alignments():
    pairs, refs = set(), set()
    case = 0
    for K in CLIP_KS:
        for _ in CLIP_NS:
            src, dst, r = cg.clip_shifts(K, case)
            assert len(src) == len(dst) == K
            pairs |= set(zip(src, dst))
            refs.add(r)
            case += 1
    assert pairs == {(a, b) for a in range(4) for b in range(4)} and refs == {0, 1, 2, 3}
    src, dst, _ = cg.clip_shifts(17, 0)  # within one call: aligned / unaligned loads with either store
    al = {(a == 0, b == 0) for a, b in zip(src, dst)}
    assert al == {(True, True), (True, False), (False, True), (False, False)}


def test_references_against_brute_force():
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((3, 40)) * 0.3).astype(np.float32)
    ref = (rng.standard_normal(40) * 0.3).astype(np.float32)
    cols = np.array([0, 1, 5, 6, 7, 20, 39])
    D = np.zeros((3, 3))
    d2 = np.zeros(3)
    n2 = np.zeros(3)
    for i in range(3):
        for e in cols:
            d2[i] += float(np.float32(rows[i, e] - ref[e])) ** 2
            n2[i] += float(rows[i, e]) ** 2
            for j in range(3):
                D[i, j] += float(np.float32(rows[i, e] - rows[j, e])) ** 2
    np.testing.assert_allclose(cg.np_pair(rows, cols), D, rtol=1e-15)
    np.testing.assert_allclose(cg.np_dist2(rows, ref, cols), d2, rtol=1e-15)
    np.testing.assert_allclose(cg.np_dist2(rows, None, cols), n2, rtol=1e-15)
    np.testing.assert_allclose(geomed_ref.dist2(rows, ref, cols), d2, rtol=1e-15)
    for c in (1.0, 1.5, 3.0000002, 0.25, 1e-3):
        c32 = np.float32(c)
        clip, scale = cg.np_clip(rows, ref[None, :], c), cg.np_scale(rows, ref[None, :], c)
        for i in range(3):
            for e in range(40):
                d = np.float32(rows[i, e] - ref[e])
                assert clip[i, e] == np.float32(np.float32(d / c32) + ref[e])
                assert scale[i, e] == np.float32(d * c32)
    ints = cg.integer_rows(3, 40, 1, -8, 8)
    iref = cg.integer_rows(1, 40, 2, -8, 8)[0]
    assert np.abs(ints).max() == 8 and (ints == np.round(ints)).all()
    assert np.array_equal(cg.int_pair(ints, cols), cg.np_pair(ints, cols))
    assert np.array_equal(cg.int_dist2(ints, iref, cols), cg.np_dist2(ints, iref, cols))
    assert np.array_equal(cg.int_dist2(ints, None, cols), cg.np_dist2(ints, None, cols))
    w = np.array([0.5, 0.25, 0.25], np.float32)
    z = geomed_ref.chain(rows, w)
    for e in range(40):
        a = np.float32(rows[0, e] * w[0])
        for i in (1, 2):
            a = np.float32(a + np.float32(rows[i, e] * w[i]))
        assert z[e] == a


def _is_bf16(x: np.ndarray) -> bool:
    return not (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & 0xFFFF).any()


def emulate_gram(rows: np.ndarray, table: np.ndarray, G: int) -> np.ndarray:
    """pairgram_split8_kernel + gram_sum + gram_dist in numpy, fp32 where the
    kernel is fp32: per 64-column stage the fp32 column mean, c = fl32(x - r)
    (asserted to be a bf16, so h = c and m = l = 0), products accumulated in
    fp32 column after column over kSplitFold = 4 stages of a block's stream,
    folded into fp64.  Every fp32 partial sum is asserted equal to the fp64
    one: no order of the MFMA's additions can round."""
    K = rows.shape[0]
    inv = np.float32(1.0) / np.float32(K)
    M = np.zeros((K, K))
    for g in range(G):
        stages = []
        for s, n in table[g::G]:
            stages += [rows[:, s + o:s + min(o + 64, n)] for o in range(0, n, 64)]
        for k in range(0, len(stages), 4):
            cs = []
            for x in stages[k:k + 4]:
                r = (x.sum(axis=0, dtype=np.float32) * inv).astype(np.float32)
                c = (x - r[None, :]).astype(np.float32)
                assert _is_bf16(c)
                assert np.array_equal(c.astype(np.float64), x.astype(np.float64) - x.astype(np.float64).mean(axis=0))
                cs.append(c)
            c = np.concatenate(cs, axis=1)
            P = c[:, None, :] * c[None, :, :]   # bf16 x bf16: exact in fp32
            run32 = np.cumsum(P, axis=2, dtype=np.float32)
            run64 = np.cumsum(P.astype(np.float64), axis=2)
            assert np.array_equal(run32.astype(np.float64), run64)
            assert np.abs(P).sum(axis=2).max() <= 2.0 ** 10   # < 2^22 units of K^-2 >= 2^-12
            M += run32[:, :, -1].astype(np.float64)
    d = (np.diag(M)[:, None] + np.diag(M)[None, :]) - (M + M.T)
    D = np.where(d < 0, 0.0, d)
    np.fill_diagonal(D, 0.0)
    return D


@pytest.mark.parametrize("K", GRAM_EXACT_KS)
def test_gram_is_exact_on_minus_one_zero_one(K):
    """The derivation test_gpu_chunk_groups.py relies on: with entries in
    {-1, 0, 1} and K a power of two up to 64 the centred values are bf16s,
    every fp32 accumulation is exact, and the Gram's D equals the integer
    reference bit for bit at any G."""
    tab, cols = cg.tiny_chunk_table(nat.PAIR_CHUNK, cg.QUARTERED_CHUNKS, 0)
    rows = cg.integer_rows(K, int(cols[-1]) + 4, 300 + K, -1, 1)
    want = cg.int_pair(rows, cols)
    for G in (1, 29, 70):
        D = emulate_gram(rows, tab, G)
        assert np.array_equal(D.view(np.uint64), want.view(np.uint64)), (K, G)
