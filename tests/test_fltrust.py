"""CPU checks of the "fltrust" defense (fedml_amd.defense.fltrust): the
coefficient rule, the two specifications in torch ops against the numpy
reference (fltrust_ref.py), the plugin surface, and the argument checks of
fedagg_dotnorm2_f32 / fedagg_wsum_diff_f32 that need no GPU.

Tolerances.  The rebuild is an fp32 chain with a fixed order: bit for bit.
The dots and norms are fp64 sums of exact products whose ORDER differs between
torch and math.fsum: any-order fp64 summation of n terms errs by at most
(n - 1) 2^-53 sum|terms|; the bound used, n 2^-52 sum|terms|, is the one the
device test uses (doubled for the kernel's wave- and group-level combines).
"""
from __future__ import annotations

from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fltrust_ref as ref
from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn

NAN, INF = float("nan"), float("inf")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


# ---- fltrust_coeffs ---------------------------------------------------------------

def test_relu_drops_negative_zero_nan_inf_and_unmoved_clients():
    #        negative zero  NaN  +inf  -inf  n2 = 0 (0/0)  n2 = 0 (1/0)  n2 = inf  n2 = NaN  honest
    dot = [-1.0,    0.0,  NAN, INF, -INF, 0.0,          1.0,          1.0,      1.0,      1.0]
    n2 = [1.0,      1.0,  1.0, 1.0, 1.0,  0.0,          0.0,          INF,      NAN,      4.0]
    trust, c = dfn.fltrust_coeffs(dot, n2, 1.0)
    assert trust.dtype == np.float64 and c.dtype == np.float64
    assert trust.tolist() == [0.0] * 9 + [0.5]
    assert c[:9].tolist() == [0.0] * 9
    assert c[9] == 0.5  # lr TS n_b / (n S) = 1 * 0.5 * 1 / (2 * 0.5)
    want = ref.coeffs(dot, n2, 1.0)
    assert want[1] == trust.tolist() and want[2] == c.tolist()


def test_no_trusted_client_gives_zero_coefficients():
    trust, c = dfn.fltrust_coeffs([-1.0, 0.0, NAN], [1.0, 1.0, 1.0], 2.0)
    assert trust.tolist() == [0.0, 0.0, 0.0] and c.tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("nb2", [0.0, NAN, INF])
def test_a_root_update_that_cannot_judge_is_refused(nb2):
    with pytest.raises(ValueError, match="root"):
        dfn.fltrust_coeffs([1.0], [1.0], nb2)
    with pytest.raises(ValueError):
        ref.coeffs([1.0], [1.0], nb2)


@pytest.mark.parametrize("K,lr", [(1, 1.0), (9, 1.0), (9, 0.3), (200, 2.5)])
def test_trusted_updates_sum_to_the_root_norm(K, lr):
    """sum_i c_i n_i = lr n_b.  Per term: sqrt for n_i, then lr TS n_b / (n_i S)
    is four roundings and c_i n_i a fifth, against an S with K - 1 roundings
    and a sum here with K - 1 more: within (2K + 4) 2^-53 relative."""
    rng = np.random.default_rng(K)
    n2 = rng.uniform(0.5, 2.0, K)
    nb2 = 1.7
    cos = rng.uniform(-1.0, 1.0, K)
    cos[0] = 0.9
    dot = cos * np.sqrt(n2) * np.sqrt(nb2)
    trust, c = dfn.fltrust_coeffs(dot, n2, nb2, lr)
    assert (trust > 0).sum() == (dot > 0).sum()
    total = 0.0
    for ci, ni in zip(c, np.sqrt(n2)):
        total += float(ci) * float(ni)
    want = lr * np.sqrt(nb2)
    assert abs(total - want) <= (2 * K + 4) * 2.0 ** -53 * want
    _, _, cr = ref.coeffs(dot.tolist(), n2.tolist(), nb2, lr)
    np.testing.assert_allclose(c, cr, rtol=4 * 2.0 ** -53, atol=0)


def test_trust_is_summed_left_to_right():
    """1 + 2^-53 + 2^-53 from the left is 1 (two ties to even); from the right,
    pairwise or exactly it is 1 + 2^-52.  c_0 = 1 / S tells them apart."""
    e = 2.0 ** -53
    trust, c = dfn.fltrust_coeffs([1.0, e, e], [1.0, 1.0, 1.0], 1.0)
    assert trust.tolist() == [1.0, e, e]
    assert c[0] == 1.0 and c[1] == e and c[2] == e
    assert 1.0 / (e + e + 1.0) != 1.0  # the other order would show


# ---- the specifications in torch ops, on the CPU -------------------------------------

def _rows(K, N, seed):
    rng = np.random.default_rng(seed)
    g = (0.05 * rng.standard_normal(N)).astype(np.float32)
    b = (0.01 * rng.standard_normal(N)).astype(np.float32)
    rows = (g[None, :] + b[None, :] + 0.01 * rng.standard_normal((K, N))).astype(np.float32)
    return rows, g, (g + b).astype(np.float32)


@pytest.mark.parametrize("K,N", [(1, 1), (3, 1000), (9, 4099)])
def test_dotnorm2_torch_against_fsum(K, N):
    rows, g, r = _rows(K, N, 10 * K + N)
    cols = np.sort(np.random.default_rng(N).choice(N, size=max(1, (2 * N) // 3), replace=False))
    for sel in (None, cols):
        n = N if sel is None else len(sel)
        both = np.concatenate([rows, r[None, :]])
        dot, n2 = dfn.dotnorm2_rows_torch(torch.from_numpy(both), torch.from_numpy(g), torch.from_numpy(r),
                                          None if sel is None else torch.from_numpy(sel))
        assert dot.dtype == torch.float64 and n2.dtype == torch.float64
        wd, wda, wn, wnb = ref.dot_norm(rows, g, r, sel)
        tol = n * 2.0 ** -52
        for i in range(K):
            assert abs(float(dot[i]) - wd[i]) <= tol * wda[i]
            assert abs(float(n2[i]) - wn[i]) <= tol * wn[i]
        assert abs(float(n2[K]) - wnb) <= tol * wnb
        assert float(dot[K]) == float(n2[K])  # the root as a row: its dot IS its squared norm


def fma_rows(K, N, seed):
    """Rows, g and coefficients (0.0, a subnormal and FMA_C among them) with
    the FMA-revealing column at 0 and at N - 1: for K >= 2 the chain's second
    step adds fl(c_1 d_1) to acc = FMA_ACC; for K == 1 the final g + acc does."""
    rng = np.random.default_rng(seed)
    g = (0.05 * rng.standard_normal(N)).astype(np.float32)
    rows = (g[None, :] + 0.01 * rng.standard_normal((max(K, 1), N))).astype(np.float32)[:K]
    c = [float(np.float32(v)) for v in rng.uniform(0.01, 0.3, K)]
    for j, v in enumerate([1.0, ref.FMA_C, 0.0, 1e-41][:K]):
        c[j] = float(np.float32(v))
    if K == 1:
        c[0] = ref.FMA_C
    for col in {0, N - 1}:
        if K == 1:
            g[col] = ref.FMA_ACC
            rows[0, col] = np.float32(-2.0 ** -12)  # x - g = FMA_D exactly
        elif K >= 2:
            g[col] = 0.0
            rows[:, col] = 0.0
            rows[0, col] = ref.FMA_ACC
            rows[1, col] = ref.FMA_D
    return rows, g, c


def check_fma_column(got_col, K):
    """The column holds fl(acc + fl(c d)) = 0, which the CPU shows to differ
    from the FMA's 2^-24."""
    if K == 0:
        return
    rounded = np.float32(ref.FMA_ACC + np.float32(np.float32(ref.FMA_C) * ref.FMA_D))
    fused = ref.fma_chain_value(ref.FMA_ACC, ref.FMA_C, ref.FMA_D)
    assert rounded == 0.0 and fused == np.float32(2.0 ** -24) and rounded != fused
    assert got_col == rounded


@pytest.mark.parametrize("K", [0, 1, 2, 3, 17])
@pytest.mark.parametrize("N", [1, 5, 2049])
def test_wsum_diff_torch_is_the_float32_chain(K, N):
    rows, g, c = fma_rows(K, N, 100 * K + N)
    want = ref.rebuild(rows, c, g)
    got = dfn.wsum_diff_rows_torch(torch.from_numpy(rows) if K else [], c, torch.from_numpy(g)).numpy()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    check_fma_column(got[0], K)
    check_fma_column(got[N - 1], K)
    if K == 0:
        assert np.array_equal(bits(got), bits(g))


def test_untrusted_rows_are_never_read_by_the_reference_rule():
    rows, g, r = _rows(5, 300, 3)
    rows[1] = g - 3 * (r - g)
    rows[3] = g - 3 * (r - g)
    rows[3, 17] = NAN
    out, cos, trust, c32, trusted = ref.fltrust(rows, g, r, np.arange(300))
    assert trusted == [0, 2, 4] and np.isnan(cos[3]) and cos[1] < -0.99
    assert np.isfinite(out).all()


# ---- flags and surface ---------------------------------------------------------------

def _args(**kw):
    return SimpleNamespace(federated_optimizer="FedAvg", enable_defense=True, defense_type="fltrust", **kw)


def test_fltrust_is_a_supported_defense_type():
    from fedml_amd.server_aggregator import _check_flags

    assert dfn.DEFENSE_FLTRUST == "fltrust" and "fltrust" in dfn.SUPPORTED
    _check_flags(_args())  # no required attribute
    with pytest.raises(NotImplementedError):
        _check_flags(SimpleNamespace(enable_defense=True, defense_type="foolsgold"))


def test_aggregate_without_a_root_model_raises_before_device_work():
    from fedml_amd.server_aggregator import MI355XServerAggregator

    agg = MI355XServerAggregator(torch.nn.Linear(3, 2), _args())
    sd = agg.get_model_params()
    with pytest.raises(RuntimeError, match="set_fltrust_root"):
        agg.aggregate([(1, sd), (2, sd)])


def test_the_root_model_serves_one_round(monkeypatch):
    from fedml_amd.server_aggregator import MI355XServerAggregator

    calls = []

    def fake(lst, g, root, lr, device):
        calls.append((lst, g, root, lr, device))
        return "aggregated"

    monkeypatch.setattr(dfn, "fltrust", fake)
    model = torch.nn.Linear(3, 2)
    agg = MI355XServerAggregator(model, _args(fltrust_lr=0.5, fedagg_device="cuda:0"))
    sd = agg.get_model_params()
    root = OrderedDict((k, v + 1) for k, v in sd.items())
    lst = [(1, sd), (2, sd)]
    agg.set_fltrust_root(root)
    assert agg.aggregate(lst) == "aggregated"
    (l0, g0, r0, lr0, d0), = calls
    assert l0 is lst and r0 is root and lr0 == 0.5 and d0 == "cuda:0" and list(g0) == list(sd)
    with pytest.raises(RuntimeError, match="set_fltrust_root"):
        agg.aggregate(lst)
    assert len(calls) == 1
    agg2 = MI355XServerAggregator(model, _args())  # the defaults: lr 1.0, no device
    agg2.set_fltrust_root(root)
    agg2.aggregate(lst)
    assert calls[1][3] == 1.0 and calls[1][4] is None


def test_fltrust_refuses_bad_inputs_before_device_work():
    d = OrderedDict(w=torch.ones(4), b=torch.ones(2))
    lst = [(1, d), (1, OrderedDict(d))]
    with pytest.raises(KeyError):
        dfn.fltrust(lst, OrderedDict(w=torch.ones(4)), d)
    with pytest.raises(KeyError):
        dfn.fltrust(lst, d, OrderedDict(b=torch.ones(2)))
    with pytest.raises(KeyError):
        dfn.fltrust([(1, d), (1, OrderedDict(w=torch.ones(4)))], d, d)
    with pytest.raises(ValueError):
        dfn.fltrust([], d, d)
    h = OrderedDict(w=torch.ones(4, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="fp32 models"):
        dfn.fltrust([(1, h)], h, h)


# ---- native argument checks, no GPU --------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


def test_dotnorm2_validates_without_gpu(lib):
    p = 64  # never dereferenced: every check stands before the first HIP call
    f = lib.fedagg_dotnorm2_f32
    for K in (0, -3):
        assert f(p, K, p, p, p, 1, p, p, 100, None) == -1
        assert b"fedagg_dotnorm2_f32: K must be >= 1" in lib.fedagg_last_error()
    assert f(p, 2, p, p, p, -1, p, p, 100, None) == -1
    assert b"n_chunks >= 0" in lib.fedagg_last_error()
    for args in ((None, 2, p, p, p, 1, p, p, 100), (p, 2, None, p, p, 1, p, p, 100), (p, 2, p, None, p, 1, p, p, 100),
                 (p, 2, p, p, None, 1, p, p, 100), (p, 2, p, p, p, 1, None, p, 100), (p, 2, p, p, p, 1, p, None, 100),
                 (p, 2, p, p, None, 0, None, None, 0)):
        lib.fedagg_wsum_f32(None, None, 0, 10, None, 0, None)  # another error in between
        assert f(*args, None) == -1, args
        assert b"fedagg_dotnorm2_f32: null pointer" in lib.fedagg_last_error()
    for K, wl in ((1, 1), (2, 3), (129, 257)):
        assert f(p, K, p, p, p, 5, p, p, wl, None) == -1
        assert b"2K doubles" in lib.fedagg_last_error()


def test_wsum_diff_validates_without_gpu(lib):
    p = 64
    f = lib.fedagg_wsum_diff_f32
    assert f(p, p, -1, p, 10, p, None) == -1
    assert b"fedagg_wsum_diff_f32: K must be >= 0" in lib.fedagg_last_error()
    assert f(p, p, 2, p, -1, p, None) == -1
    assert b"N >= 0" in lib.fedagg_last_error()
    for args in ((None, p, 2, p, 10, p), (p, None, 2, p, 10, p), (p, p, 2, None, 10, p), (p, p, 2, p, 10, None),
                 (None, None, 0, None, 10, p), (None, None, 0, p, 10, None)):
        lib.fedagg_wsum_f32(None, None, 0, 10, None, 0, None)
        assert f(*args, None) == -1, args
        assert b"fedagg_wsum_diff_f32: null pointer" in lib.fedagg_last_error()
    assert f(None, None, 0, p, 0, p, None) == 0  # K == 0 is a call (out = ref), N == 0 has nothing to launch
    assert f(p, p, 3, p, 0, p, None) == 0


def test_dotnorm2_work_len(lib):
    f = lib.fedagg_robust_work_len
    assert nat.WORK_DOTNORM2 == 5
    for K, n in ((1, 1), (3, 7), (9, 1024), (129, 1025), (1000, 25_011)):
        assert f(nat.WORK_DOTNORM2, K, n) == 2 * K * min(n, 1024)
    assert f(nat.WORK_DOTNORM2, 4, 0) == 0
    assert f(nat.WORK_DOTNORM2, 0, 5) == -1 and f(nat.WORK_DOTNORM2, 4, -1) == -1
    assert f(6, 4, 5) == -1 and f(99, 4, 5) == -1 and f(-1, 4, 5) == -1
    assert nat.WSUM_DIFF_TILE == 2048  # FEDAGG_WSUM_DIFF_TILE (include/fedagg.h), the kernel's kWdTile
