"""The "wise_bulyan" defense without a GPU: the torch path of the
nearest-to-median mean against the two-pointer reference (tests/bulyan_ref.py),
stage 1's selection against plain loops, the C entry's argument checks and the
defense's host-side validation."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest
import torch

import bulyan_ref as br
import trimmed_mean_ref as tmr
from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn
from fedml_amd import server_aggregator as sa

INF, NAN = br.INF, br.NAN


@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


def _window_nans(K: int, keep: int) -> int:
    """With every non-NaN value equal, all distances tie and go left: the
    window is [max(0, r - keep + 1), .. + keep).  This many NaNs leave it one
    rank short of the first NaN; one more and it touches it."""
    r = (K - 1) // 2
    return K - (max(0, r - keep + 1) + keep)


def _plant(x: torch.Tensor, keep: int) -> torch.Tensor:
    """Specials in the last ten columns."""
    K = x.shape[0]
    r = (K - 1) // 2
    x = x.clone()
    x[0, -1] = NAN
    x[K // 2, -2] = -NAN
    n = _window_nans(K, keep)
    x[:, -3] = 0.25
    x[:n, -3] = NAN  # the window stops one rank short of the first NaN
    x[:, -4] = 0.25
    x[:min(K, n + 1), -4] = NAN  # ... and touches it
    x[0, -5] = INF
    x[K - 1, -6] = -INF
    x[0, -7], x[K - 1, -7] = INF, -INF
    x[:K - r, -8] = INF  # m = +inf
    x[:, -9] = 0.125
    x[:, -10] = -0.0
    return x


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 13, 130])
def test_torch_path_equals_reference(K):
    N = 257
    base = tmr.make_rows(K, N, torch.float32, seed=400 + K)
    for keep in br.keeps(K):
        x = _plant(base, keep)
        ref = br.nearmedian_mean_ref(x, keep)
        # the planted NaN edge, on the reference: short of the NaNs, then touching them
        assert not bool(torch.isnan(ref[-3])) and ref[-3].item() == 0.25
        assert bool(torch.isnan(ref[-4]))
        assert ref[-9].item() == 0.125
        assert ref[-10].item() == 0 and bool(torch.signbit(ref[-10]))
        got = dfn.nearmedian_mean_rows_torch(x, keep)
        tmr.assert_same(got, ref, f"K={K} keep={keep}")
        # a list of rows, in chunks that do not divide N
        got = dfn.nearmedian_mean_rows_torch([x[i] for i in range(K)], keep, chunk_cols=100)
        tmr.assert_same(got, ref, f"K={K} keep={keep} chunked")


def test_reference_basics():
    """The reference itself on columns worked by hand (K = 5, r = 2)."""
    x = torch.tensor([[1.0, 0.0, -0.0, NAN, INF, 1.0],
                      [2.0, 1.0, -0.0, 1.0, INF, 2.0],
                      [3.0, 2.0, -0.0, 2.0, INF, 3.0],
                      [10.0, 3.0, -0.0, NAN, -INF, 3.5],
                      [11.0, 4.0, -0.0, 3.0, 0.0, 9.0]])
    r3 = br.nearmedian_mean_ref(x, 3)
    assert r3[0].item() == 2.0  # 1 2 [3] 10 11: both left neighbours are nearer than 10
    assert r3[1].item() == 2.0  # symmetric: the tie goes left (1), then right (3): (1 + 2 + 3) / 3
    assert r3[2].item() == 0 and bool(torch.signbit(r3[2]))
    assert r3[3].item() == 2.0  # 1 2 [3] NaN NaN: a NaN is at +inf, the window stays left of it
    assert r3[4].item() == INF  # -inf 0 [inf] inf inf: m = +inf, d(+inf) = 0: the three +inf
    r2 = br.nearmedian_mean_ref(x, 2)
    assert r2[1].item() == 1.5  # the one tie: left
    assert r2[5].item() == 3.25  # 1 2 [3] 3.5 9: 3.5 is nearer than 2
    r4 = br.nearmedian_mean_ref(x, 4)
    assert bool(torch.isnan(r4[3]))  # four of 1 2 3 NaN NaN hold a NaN
    assert bool(torch.isnan(br.nearmedian_mean_ref(x[:, 4:5], 5)[0]))  # +inf with -inf


def test_reference_m_inf_window():
    # -inf 0 [inf] inf inf: the three +inf are at distance 0 and all kept
    x = torch.tensor([[INF], [INF], [INF], [-INF], [0.0]])
    assert br.nearmedian_mean_ref(x, 3)[0].item() == INF
    assert dfn.nearmedian_mean_rows_torch(x, 3)[0].item() == INF


@pytest.mark.parametrize("K", [1, 2, 5, 8, 13])
def test_keep_all_is_the_ascending_mean(K):
    x = _plant(tmr.make_rows(K, 257, torch.float32, seed=500 + K), K)
    want = tmr.trimmed_mean_ref(x, 0)
    tmr.assert_same(br.nearmedian_mean_ref(x, K), want, f"reference K={K}")
    tmr.assert_same(dfn.nearmedian_mean_rows_torch(x, K), want, f"torch K={K}")


@pytest.mark.parametrize("K", [5, 8, 13])
def test_row_order_does_not_matter(K):
    g = torch.Generator().manual_seed(K)
    for keep in br.keeps(K):
        x = _plant(tmr.make_rows(K, 257, torch.float32, seed=600 + K), keep)
        y = x[torch.randperm(K, generator=g)]
        a, b = dfn.nearmedian_mean_rows_torch(x, keep), dfn.nearmedian_mean_rows_torch(y, keep)
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        ok = torch.isnan(a) | (tmr.bits(a) == tmr.bits(b))
        assert bool(ok.all())
        tmr.assert_same(br.nearmedian_mean_ref(y, keep), br.nearmedian_mean_ref(x, keep), f"reference K={K}")


EXHAUSTIVE = [(K, "a9") for K in range(1, 7)] + [(7, "a5"), (8, "a5")]


@pytest.mark.parametrize("K,alphabet", EXHAUSTIVE, ids=[f"K{K}-{a}" for K, a in EXHAUSTIVE])
def test_exhaustive_small_columns(K, alphabet):
    """Every column of length K over the alphabet, at every keep."""
    x = br.all_columns(br.ALPHABET9 if alphabet == "a9" else br.ALPHABET5, K)
    assert x.shape == (K, (9 if alphabet == "a9" else 5) ** K)
    for keep in range(1, K + 1):
        tmr.assert_same(dfn.nearmedian_mean_rows_torch(x, keep), br.nearmedian_mean_ref(x, keep),
                        f"K={K} keep={keep}")


def test_torch_path_rejects_bad_arguments():
    x = torch.zeros((4, 3))
    for keep in (-1, 0, 5):
        with pytest.raises(ValueError):
            dfn.nearmedian_mean_rows_torch(x, keep)
    with pytest.raises(TypeError):
        dfn.nearmedian_mean_rows_torch(x.double(), 1)
    with pytest.raises(TypeError):
        dfn.nearmedian_mean_rows_torch(x.bfloat16(), 1)


# ---- stage 1 --------------------------------------------------------------------

def _random_d(K: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((K, 6))
    D = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    return D


def _same_selection(D, f):
    got, want = dfn.bulyan_select(D, f), br.bulyan_select_ref(D, f)
    assert got[0] == want[0], (got[0], want[0])
    assert len(got[1]) == len(want[1]) == len(D) - 2 * f
    for a, b in zip(got[1], want[1]):
        assert a == b or abs(a - b) <= 1e-12 * abs(b), (got[1], want[1])
    return got


@pytest.mark.parametrize("K,f", [(7, 1), (11, 2), (15, 3), (23, 5), (40, 3), (131, 2)])
def test_select_random(K, f):
    sel, _ = _same_selection(_random_d(K, 10 * K + f), f)
    assert len(set(sel)) == K - 2 * f


def test_select_equal_scores_go_to_the_lowest_index():
    K, f = 11, 2
    D = np.ones((K, K)) - np.eye(K)
    sel, scores = _same_selection(D, f)
    assert sel == list(range(K - 2 * f))
    # two mirror-image clients far from the rest: equal scores there too
    D = _random_d(K, 3)
    D[[4, 9]] = D[4]
    D[:, [4, 9]] = D[:, [4]]
    D[4, 9] = D[9, 4] = D[4, 4] = D[9, 9] = 0.0
    sel, _ = _same_selection(D, f)
    if 4 in sel and 9 in sel:
        assert sel.index(4) < sel.index(9)


def test_select_never_takes_nan_or_inf_clients():
    K, f = 11, 2
    D = _random_d(K, 5)
    D[3, :], D[:, 3] = np.nan, np.nan  # a client that sent NaN: its row and column
    D[7, :], D[:, 7] = np.inf, np.inf
    D[7, 7] = 0.0
    sel, scores = _same_selection(D, f)
    assert 3 not in sel and 7 not in sel and len(sel) == 7
    assert all(np.isfinite(s) for s in scores)
    # three of them are more than f: the last rounds have nothing else to take
    D[5, :], D[:, 5] = np.nan, np.nan
    sel, _ = _same_selection(D, 2)
    assert len(sel) == 7


def test_select_f0_takes_everyone_in_order():
    D = _random_d(9, 1)
    assert dfn.bulyan_select(D, 0) == (list(range(9)), [0.0] * 9)
    assert br.bulyan_select_ref(D, 0) == (list(range(9)), [0.0] * 9)
    assert dfn.bulyan_select(np.empty((9, 0)), 0)[0] == list(range(9))  # no distances are looked at


def test_select_single_neighbour_rounds():
    """f = 1 at K = 7: n - f - 2 reaches 0 in the last rounds, which score on
    the one nearest neighbour."""
    for seed in range(5):
        sel, _ = _same_selection(_random_d(7, 70 + seed), 1)
        assert len(sel) == 5


# ---- the defense's host-side validation -------------------------------------------

def _clients(K: int):
    return [(1, OrderedDict(a=torch.ones(3))) for _ in range(K)]


@pytest.mark.parametrize("K,f", [(2, 0), (6, 1), (10, 2), (5, -1), (20, -3)])
def test_bulyan_bounds(K, f):
    with pytest.raises(ValueError):
        dfn.bulyan(_clients(K), f)


class _Args:
    def __init__(self, **kw):
        self.federated_optimizer = "FedAvg"
        self.enable_defense = True
        self.__dict__.update(kw)


def test_check_flags_wants_byzantine_client_num():
    assert "wise_bulyan" in dfn.SUPPORTED and dfn.DEFENSE_WISE_BULYAN == "wise_bulyan"
    sa._check_flags(_Args(defense_type="wise_bulyan", byzantine_client_num=2))
    with pytest.raises(AttributeError):
        sa._check_flags(_Args(defense_type="wise_bulyan"))


def test_fedml_bulyan_stays_refused():
    assert "bulyan" not in dfn.SUPPORTED
    with pytest.raises(NotImplementedError):
        sa._check_flags(_Args(defense_type="bulyan", byzantine_client_num=2))


def test_abi_validation_without_gpu(lib):
    f = lib.fedagg_nearmedian_mean_f32
    ok = (1, 4, 10, 2, 1, 0, None)  # src, K, N, keep, out, flags, stream

    def call(**kw):
        a = dict(zip(("src", "K", "N", "keep", "out", "flags", "stream"), ok))
        a.update(kw)
        return f(*a.values())

    assert call(K=0) == -1
    assert b"fedagg_nearmedian_mean_f32" in lib.fedagg_last_error() and b"K must be" in lib.fedagg_last_error()
    assert call(K=-3) == -1
    assert call(N=-1) == -1
    assert call(keep=0) == -1
    assert b"keep" in lib.fedagg_last_error()
    assert call(keep=-1) == -1
    assert call(keep=5) == -1  # keep > K
    assert call(src=None) == -1
    assert b"null" in lib.fedagg_last_error()
    assert call(out=None) == -1
    assert call(K=129, keep=3) == -2  # FEDAGG_ENOKERNEL
    assert b"128" in lib.fedagg_last_error() and b"129" in lib.fedagg_last_error()
    assert call(K=129, keep=130) == -1  # an invalid keep is EINVAL whatever K is
    assert call(N=0) == 0
    assert call(K=1, keep=1, N=0) == 0
    assert call(K=128, keep=128, N=0) == 0
    assert nat.NEARMEDIAN_MAX_CLIENTS == 128 == dfn.NEARMEDIAN_MAX_CLIENTS
