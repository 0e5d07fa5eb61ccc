"""fedagg_nearmedian_mean_wide_f32 without a GPU: the C entry's argument checks
(all made before any HIP call), its cap, the tier lookup of the dispatch, and
stage 1 of Bulyan (defense.bulyan_select, which above 256 clients sorts every
row of the distances once) bit for bit against the plain loops of
tests/bulyan_ref.py and against the sort per round."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import bulyan_ref as br
from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn


@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


def _caller(f):
    ok = (1, 300, 10, 200, 1, 0, None)  # src, K, N, keep, out, flags, stream (the pointers are never dereferenced)

    def call(**kw):
        a = dict(zip(("src", "K", "N", "keep", "out", "flags", "stream"), ok))
        a.update(kw)
        return f(*a.values())

    return call


def test_constants():
    assert nat.NEARMEDIAN_WIDE_MAX_CLIENTS == 1024 == dfn.NEARMEDIAN_WIDE_MAX_CLIENTS
    assert nat.NEARMEDIAN_MAX_CLIENTS == 128 == dfn.NEARMEDIAN_MAX_CLIENTS  # the narrow entry keeps its cap


def test_argument_checks_without_a_device(lib):
    call = _caller(lib.fedagg_nearmedian_mean_wide_f32)
    assert call(K=0) == -1  # FEDAGG_EINVAL
    assert b"fedagg_nearmedian_mean_wide_f32" in lib.fedagg_last_error() and b"K must be" in lib.fedagg_last_error()
    assert call(K=-3) == -1
    assert call(N=-1) == -1
    assert b"N >= 0" in lib.fedagg_last_error()
    assert call(keep=0) == -1
    assert b"keep must be" in lib.fedagg_last_error()
    assert call(keep=301) == -1  # keep = K + 1
    assert b"keep must be" in lib.fedagg_last_error()
    assert call(K=1, keep=2) == -1
    assert call(src=None) == -1
    assert b"null" in lib.fedagg_last_error()
    assert call(out=None) == -1
    assert b"null" in lib.fedagg_last_error()
    assert call(K=1025) == -2  # FEDAGG_ENOKERNEL
    msg = lib.fedagg_last_error()
    assert b"1024" in msg and b"1025" in msg
    assert call(K=1025, keep=1026) == -1  # an invalid keep is EINVAL whatever K is
    assert call(K=5000, keep=1, N=0) == -2
    for K, keep in ((1, 1), (128, 100), (129, 1), (300, 300), (512, 77), (1024, 1024)):
        assert call(K=K, keep=keep, N=0) == 0, (K, keep)  # FEDAGG_OK, nothing to launch


def test_grid_bound(lib):
    """A block holds 64 columns up to 512 rows and 32 above: the first N whose
    grid passes 2^31 - 1 blocks is refused, for every tier."""
    call = _caller(lib.fedagg_nearmedian_mean_wide_f32)
    for K, cols in ((1, 64), (300, 64), (512, 64), (513, 32), (1024, 32)):
        assert call(K=K, keep=1, N=(2 ** 31 - 1) * cols + 1) == -1, K
        assert b"N too large" in lib.fedagg_last_error()
    assert call(N=2 ** 62) == -1


def test_narrow_entry_keeps_its_cap(lib):
    call = _caller(lib.fedagg_nearmedian_mean_f32)
    assert call(K=129, keep=1) == -2
    assert b"128" in lib.fedagg_last_error()
    assert call(K=128, keep=1, N=0) == 0


def test_wide_auto(monkeypatch):
    """Every tier of the wide kernel has an entry, K finds its tier, and
    nothing above the cap is decided by the table."""
    assert sorted(dfn.NEARMEDIAN_WIDE_AUTO) == [256, 512, 1024]
    assert all(isinstance(v, bool) for v in dfn.NEARMEDIAN_WIDE_AUTO.values())
    for K, tier in ((129, 256), (256, 256), (257, 512), (512, 512), (513, 1024), (1024, 1024)):
        for on in (256, 512, 1024):  # the one tier that is True
            monkeypatch.setattr(dfn, "NEARMEDIAN_WIDE_AUTO", {t: t == on for t in (256, 512, 1024)})
            assert dfn.nearmedian_wide_auto(K) is (tier == on), (K, on)
    for table in ({256: True, 512: True, 1024: True}, {256: False, 512: False, 1024: False}):
        monkeypatch.setattr(dfn, "NEARMEDIAN_WIDE_AUTO", table)
        assert dfn.nearmedian_wide_auto(1025) is False and dfn.nearmedian_wide_auto(5000) is False


# ---- stage 1: bulyan_select ---------------------------------------------------

def _sym(K: int, rng) -> np.ndarray:
    a = rng.random((K, K))
    D = a + a.T
    np.fill_diagonal(D, 0.0)
    return D


def _inputs(K: int, f: int):
    """Random symmetric distances; one and then f clients whose row and column
    are NaN; a +inf client; two identical clients (an exact tie in every
    round); all zero."""
    rng = np.random.default_rng(100 * K + f)
    D = _sym(K, rng)
    yield "random", D
    for count in sorted({1, f}):
        N = D.copy()
        for i in rng.choice(K, size=count, replace=False):
            N[i, :], N[:, i] = np.nan, np.nan
        yield f"nan{count}", N
    I = D.copy()
    I[2, :], I[:, 2] = np.inf, np.inf
    I[2, 2] = 0.0
    yield "inf", I
    T = D.copy()
    T[4, :], T[:, 4] = T[1, :], T[:, 1]  # client 4 is client 1 again
    T[1, 4] = T[4, 1] = T[4, 4] = 0.0
    yield "twins", T
    yield "zero", np.zeros((K, K))


def _same(got, want, what):
    assert got[0] == want[0], what
    assert np.array_equal(np.array(got[1], dtype=np.float64).view(np.int64),
                          np.array(want[1], dtype=np.float64).view(np.int64)), what


@functools.lru_cache(maxsize=None)
def _select_cases(K: int):
    """[(f, name, D, bulyan_select_ref's answer)]: computed once, shared by the paths."""
    return [(f, name, D, br.bulyan_select_ref(D, f)) for f in sorted({1, (K - 3) // 4}) for name, D in _inputs(K, f)]


# "auto": the path bulyan_select takes by itself (up to BULYAN_PRESORT_ABOVE
# clients the sort per round); then the presorted rows at every K, compacted
# every 32 rounds as shipped, every 5 and after every round
@pytest.mark.parametrize("path", ["auto", "presorted", "presorted-compact5", "presorted-compact1"])
@pytest.mark.parametrize("K", [7, 23, 64, 140])
def test_bulyan_select_matches_the_plain_loops(K, path, monkeypatch):
    if path != "auto":
        monkeypatch.setattr(dfn, "BULYAN_PRESORT_ABOVE", 0)
        if "compact" in path:
            monkeypatch.setattr(dfn, "_BULYAN_COMPACT_EVERY", int(path.split("compact")[1]))
    for f, name, D, want in _select_cases(K):
        before = D.copy()
        got = dfn.bulyan_select(D, f)
        assert np.array_equal(D, before, equal_nan=True), "the distances are not modified"
        assert len(got[0]) == K - 2 * f == len(set(got[0])) == len(got[1])
        assert all(type(i) is int for i in got[0]) and all(type(s) is float for s in got[1])
        _same(got, want, f"K={K} f={f} {name} {path}")


def _select_by_sorting_every_round(D, f: int):
    """bulyan_select as it was before the presorted rows: every round
    re-sorts the n x n sub-matrix of the clients still in R."""
    D = np.asarray(D, dtype=np.float64)
    K = len(D)
    R = list(range(K))
    selected, scores = [], []
    for _ in range(K - 2 * f):
        n = len(R)
        sub = D[np.ix_(R, R)].copy()
        sub[np.arange(n), np.arange(n)] = np.nan
        c = min(max(1, n - f - 2), n - 1)
        if c < 1:
            sc = np.zeros(n)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                sc = np.cumsum(np.sort(sub, axis=1)[:, :c], axis=1)[:, c - 1]
        sc = np.where(np.isnan(sc), np.inf, sc)
        p = int(np.argmin(sc))
        selected.append(R[p])
        scores.append(float(sc[p]))
        del R[p]
    return selected, scores


def test_bulyan_select_at_300_clients():
    """bulyan_select_ref is too slow here: the per-round sort stands in.  300
    clients take the presorted rows by themselves."""
    K, f = 300, 5
    assert K > dfn.BULYAN_PRESORT_ABOVE
    for name, D in _inputs(K, f):
        _same(dfn.bulyan_select(D, f), _select_by_sorting_every_round(D, f), f"K={K} f={f} {name}")


def test_the_per_round_sort_is_the_plain_loops():
    """What stands in at 300 clients agrees with bulyan_select_ref where both run."""
    for K, f in ((23, 5), (64, 1)):
        for name, D in _inputs(K, f):
            _same(_select_by_sorting_every_round(D, f), br.bulyan_select_ref(D, f), f"K={K} f={f} {name}")
