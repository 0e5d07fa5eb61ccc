"""CPU checks of the wide Gram's host side (fedagg_pairgram2_wide_f32 in
csrc/robust.hip, pairdist2_rows' "gram_wide" in fedml_amd/defense.py): the
entry point's argument checks, which all return before anything touches the
device, the workspace formula, the tier lookup, and the numpy form of
krum_scores against the Python loop, bit for bit."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn


@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


def _tiles(K):
    T = (K + 63) // 64
    return T * (T + 1) // 2


def _groups(K, n_chunks):
    """chunk groups of a full workspace: about 2,048 blocks, one per chunk at most"""
    return min(n_chunks, -(-4096 // (2 * _tiles(K))))


def test_constants():
    assert nat.WORK_PAIRGRAM_WIDE == 4 and nat.PAIRGRAM_WIDE_MAX_CLIENTS == 1024
    assert dfn.PAIRGRAM_WIDE_MAX_CLIENTS == 1024
    assert "fedagg_pairgram2_wide_f32" in nat.SIGNATURES


def test_work_len(lib):
    wl = lib.fedagg_robust_work_len
    assert wl(nat.WORK_PAIRGRAM_WIDE, 1025, 1) == -1
    assert wl(nat.WORK_PAIRGRAM_WIDE, 0, 1) == -1
    assert wl(nat.WORK_PAIRGRAM_WIDE, 1024, -1) == -1
    for K in (1, 64, 65, 129, 200, 1024):
        assert wl(nat.WORK_PAIRGRAM_WIDE, K, 0) == 0
        for n in (1, 2, 19, 700, 100_000):
            assert wl(nat.WORK_PAIRGRAM_WIDE, K, n) == _groups(K, n) * _tiles(K) * 4096 + K * K, (K, n)
    # the narrow kind keeps its limit
    assert wl(nat.WORK_PAIRGRAM, 129, 1) == -1


def test_entry_point_argument_checks(lib):
    """Every pointer below is a host buffer: a call that got past the checks
    would hand it to a launch.  All of them must return FEDAGG_EINVAL first."""
    fn = lib.fedagg_pairgram2_wide_f32
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    need = 4096 + 9   # K = 3: one tile pair's partials and the 3 x 3 matrix

    def msg():
        return lib.fedagg_last_error().decode()

    assert fn(p, 0, p, p, 1, p, p, need, None) == -1 and "K must be in [1, 1024]" in msg()
    assert fn(p, 1025, p, p, 1, p, p, 1 << 40, None) == -1 and "K must be in [1, 1024]" in msg()
    assert fn(p, 3, p, p, -1, p, p, need, None) == -1
    assert fn(p, 3, None, p, 1, p, p, need, None) == -1 and "null pointer" in msg()   # the centre
    assert fn(p, 3, None, p, 0, p, p, need, None) == -1 and "null pointer" in msg()   # ... even with no chunks
    assert fn(None, 3, p, p, 1, p, p, need, None) == -1 and "null pointer" in msg()
    assert fn(p, 3, p, p, 1, None, p, need, None) == -1 and "null pointer" in msg()
    assert fn(p, 3, p, None, 1, p, p, need, None) == -1 and "null pointer" in msg()
    assert fn(p, 3, p, p, 1, p, None, need, None) == -1 and "null pointer" in msg()
    assert fn(p, 3, p, p, 1, p, p, need - 1, None) == -1 and "workspace too small" in msg()
    assert fn(p, 3, p, p, 1, p, p, 0, None) == -1 and "workspace too small" in msg()
    assert fn(p, 200, p, p, 1, p, p, 10 * 4096 + 200 * 200 - 1, None) == -1 and "workspace too small" in msg()


def test_tier_lookup(monkeypatch):
    assert set(dfn.PAIRGRAM_WIDE_AUTO) == {256, 512, 1024}
    assert all(isinstance(v, bool) for v in dfn.PAIRGRAM_WIDE_AUTO.values())
    monkeypatch.setattr(dfn, "PAIRGRAM_WIDE_AUTO", {256: True, 512: False, 1024: True})
    for K, want in ((129, True), (200, True), (256, True), (257, False), (512, False), (513, True), (1024, True),
                    (1025, False), (5000, False)):
        assert dfn.pairgram_wide_auto(K) is want, K
    monkeypatch.setattr(dfn, "PAIRGRAM_WIDE_AUTO", {256: True, 512: True, 1024: True})
    assert dfn.pairgram_wide_auto(1025) is False


def test_gram_wide_rejects_more_than_1024_clients():
    """ValueError before any tensor is made or the library is called."""
    with pytest.raises(ValueError, match="at most 1024"):
        dfn.pairdist2_rows(None, 1025, None, 1, "cpu", "gram_wide", length=8)
    with pytest.raises(ValueError, match="length or a centre"):
        dfn.pairdist2_rows(None, 300, None, 1, "cpu", "gram_wide")
    with pytest.raises(ValueError, match="gram_wide"):
        dfn.pairdist2_rows(None, 300, None, 1, "cpu", "gram_tall")
    with pytest.raises(ValueError, match="at most 128"):
        dfn.pairdist2_rows(None, 129, None, 1, "cpu", "gram", length=8)


def _sym(K, seed):
    """Random symmetric D with a zero diagonal, exact ties inside rows and
    across rows, and one client at infinity."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.5, 2.0, (K, K)) ** 2
    D = np.triu(A, 1) + np.triu(A, 1).T
    t = min(K - 1, 3)
    D[0, 1:1 + t] = D[1:1 + t, 0] = 1.25            # a tie inside row 0
    D[K - 1, 1] = D[1, K - 1] = D[K - 2, 1] = D[1, K - 2] = 0.75   # ... and inside row 1
    D[2, :] = D[:, 2] = np.inf                       # an inf client
    D[2, 2] = 0.0
    if K > 20:
        D[7, 10:15] = D[10:15, 7] = 0.0              # distinct clients at distance 0
        # fp64 values that tie only after the fp32 root
        D[8, 11] = D[11, 8] = 1.0 + 2.0 ** -40
        D[8, 12] = D[12, 8] = 1.0
    return D


@pytest.mark.parametrize("K", [5, 129, 300])
def test_krum_scores_numpy_is_the_loop_bit_for_bit(K):
    for seed in (0, 1):
        D = _sym(K, 10 * K + seed)
        for f in sorted({0, 1, (K - 3) // 2, K - 3, K - 2, K - 1, K + 3}):
            want = dfn.krum_scores_loop(D, f)
            got = dfn.krum_scores_numpy(D, f)
            assert got is not None and len(got) == len(want) == K
            assert np.array_equal(np.asarray(got, np.float64).view(np.uint64),
                                  np.asarray(want, np.float64).view(np.uint64)), (K, f)
            if K > dfn.KRUM_SCORES_LOOP_MAX_CLIENTS:
                assert dfn.krum_scores(D, f) == got
            else:
                assert dfn.krum_scores(D, f) == want


def test_krum_scores_keeps_the_loop_for_nan():
    D = _sym(129, 3)
    D[4, 9] = D[9, 4] = float("nan")
    assert dfn.krum_scores_numpy(D, 5) is None
    a, b = dfn.krum_scores(D, 5), dfn.krum_scores_loop(D, 5)
    assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
