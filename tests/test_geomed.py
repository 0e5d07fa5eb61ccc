"""CPU checks of the "geomed" defense (fedml_amd.defense.geometric_median):
the specification in torch ops against the numpy reference (geomed_ref.py),
the Weiszfeld driver, its robustness, the lazy screen for non-finite clients,
and the argument checks of fedagg_wsum_dist2_f32 that need no GPU.

Tolerances.  z is an fp32 chain with a fixed order: bit for bit.  D is an fp64
sum of exact squares whose ORDER differs between torch and numpy: at most
N 2^-53 < 1e-12 relative for the N <= 4099 columns here (fedagg_dist2_f32's
tolerance).  The weights are a_i / sqrt(D_i) normalised, so a relative error
e in D moves them by about e / 2 per pass and the contraction does not
amplify it: 17 passes stay far inside 1e-9.
"""
from __future__ import annotations

import logging
from collections import OrderedDict

import numpy as np
import pytest
import torch

import geomed_ref as ref
from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def torch_step(rows, cols=None):
    t = torch.from_numpy(rows)
    c = None if cols is None else torch.from_numpy(np.asarray(cols))

    def step(w32):
        z, D = dfn.weiszfeld_step_torch(t, w32, c)
        return z.numpy(), D.numpy()
    return step


def weights_of(counts):
    total = 0
    for n in counts:
        total += n
    return [n / total for n in counts]


@pytest.fixture(scope="module")
def robust():
    """(rows, counts, corrupted, a, z, w, info) per robustness case, computed once."""
    out = {}
    for K, bad in ref.ROBUST_CASES:
        rows, counts, corrupted = ref.robust_clients(K, bad)
        a = weights_of(counts)
        z, w, info = dfn.geometric_median_loop(torch_step(rows), a, 1e-6, 16, 0.0)
        out[(K, bad)] = (rows, counts, corrupted, a, z, w, info)
    return out


@pytest.mark.parametrize("K,N", [(1, 5), (2, 64), (7, 1025), (33, 4099)])
def test_step_torch_matches_numpy(K, N):
    rng = np.random.default_rng(K)
    rows = (0.05 * rng.standard_normal((K, N))).astype(np.float32)
    rows[0, :3] = [0.0, -0.0, 1e-42]  # signed zeros and a denormal
    w = rng.random(K)
    w /= w.sum()
    cols = np.sort(rng.choice(N, size=max(1, N // 2), replace=False))
    z, D = dfn.weiszfeld_step_torch(torch.from_numpy(rows), w.tolist(), torch.from_numpy(cols))
    zr, Dr = ref.step(rows, w, cols)
    assert np.array_equal(bits(z.numpy()), bits(zr))
    np.testing.assert_allclose(D.numpy(), Dr, rtol=1e-12, atol=0)
    zl, Dl = dfn.weiszfeld_step_torch([torch.from_numpy(r) for r in rows], w.tolist())  # a list of rows, all columns
    assert np.array_equal(bits(zl.numpy()), bits(zr))
    np.testing.assert_allclose(Dl.numpy(), ref.dist2(rows, zr), rtol=1e-12, atol=0)


def test_geomed_weights_match_reference():
    rng = np.random.default_rng(3)
    for K in (1, 2, 9, 128):
        a = weights_of([int(v) for v in rng.integers(50, 150, K)])
        D = rng.random(K) * 10.0 ** rng.integers(-20, 6, K)
        D[0] = 0.0  # below nu
        for nu in (1e-6, 1e-3):
            w = dfn.geomed_weights(D, a, nu)
            assert w.dtype == np.float64
            assert np.array_equal(w, ref.weights(D, a, nu))
            assert abs(w.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("case", ref.ROBUST_CASES)
def test_loop_matches_reference(case, robust):
    rows, _, _, a, z, w, info = robust[case]
    zr, wr, fr = ref.loop(rows, a, 1e-6, 16, 0.0)
    assert info.iterations == 16 and len(info.objective) == 17 == len(fr)
    np.testing.assert_allclose(w, wr, rtol=1e-9, atol=0)
    np.testing.assert_allclose(info.objective, fr, rtol=1e-9, atol=0)
    # z with the reference's own weights is the reference's z, bit for bit
    assert np.array_equal(bits(ref.chain(rows, wr.astype(np.float32))), bits(zr))
    assert np.array_equal(bits(z), bits(ref.chain(rows, np.asarray(w).astype(np.float32))))


def test_loop_stops_on_ftol_and_counts_passes():
    rows, counts, _ = ref.robust_clients(9, 2)
    a = weights_of(counts)
    calls = []
    inner = torch_step(rows)

    def step(w32):
        calls.append(list(w32))
        return inner(w32)

    z, w, info = dfn.geometric_median_loop(step, a, 1e-6, 16, 1e-3)
    zr, wr, fr = ref.loop(rows, a, 1e-6, 16, 1e-3)
    assert info.iterations == len(fr) - 1 < 16 and len(calls) == info.iterations + 1
    assert all(isinstance(v, float) and v == float(np.float32(v)) for v in calls[-1])  # fl32(w) goes in
    np.testing.assert_allclose(w, wr, rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        dfn.geometric_median_loop(step, a, 1e-6, -1, 0.0)


def test_maxiter_zero_is_fedavg():
    rows, counts, _ = ref.robust_clients(16, 5)
    a = weights_of(counts)
    z, w, info = dfn.geometric_median_loop(torch_step(rows), a, 1e-6, 0, 1e-6)
    assert info.iterations == 0 and len(info.objective) == 1
    assert np.array_equal(w, np.array(a))
    assert np.array_equal(bits(z), bits(ref.chain(rows, np.array(a).astype(np.float32))))


def test_one_client_returns_its_own_bits():
    rows = (np.random.default_rng(5).standard_normal((1, 257)) * 1e3).astype(np.float32)
    rows[0, :4] = [0.0, -0.0, 1e-42, -3e38]
    z, w, info = dfn.geometric_median_loop(torch_step(rows), [1.0], 1e-6, 16, 0.0)
    assert np.array_equal(bits(z), bits(rows[0])) and w.tolist() == [1.0]


def test_identical_clients_keep_their_sample_weights():
    row = (0.05 * np.random.default_rng(6).standard_normal(257)).astype(np.float32)
    rows = np.stack([row] * 7)
    a = weights_of([3, 50, 7, 11, 120, 64, 1])
    z, w, info = dfn.geometric_median_loop(torch_step(rows), a, 1e-3, 8, 0.0)
    np.testing.assert_allclose(w, a, rtol=1e-14, atol=0)  # every distance is below nu: b_i = a_i / nu
    np.testing.assert_allclose(z, row, rtol=1e-6, atol=0)


@pytest.mark.parametrize("case", ref.ROBUST_CASES)
def test_objective_never_rises(case, robust):
    f = robust[case][6].objective
    for t in range(len(f) - 1):
        assert f[t + 1] <= f[t] * (1 + 1e-6), (t, f[t], f[t + 1])


@pytest.mark.parametrize("case", ref.ROBUST_CASES)
def test_robust_to_corrupted_clients(case, robust):
    rows, _, corrupted, a, z, w, _ = robust[case]
    got = ref.robust_check(z, w, rows, corrupted)
    print(case, got)
    assert got["ratio"] < 1.0
    assert got["corrupted_weight"] < 1e-4
    fedavg = ref.robust_check(ref.chain(rows, np.array(a).astype(np.float32)), a, rows, corrupted)
    assert fedavg["ratio"] > 1e2  # what the defense is for: the plain average is far outside


def _screen_setup(rows, cols=None):
    t = torch.from_numpy(rows)
    seen = []

    def make_step(alive):
        seen.append(list(alive))
        return torch_step(rows[alive], cols)

    def norms2():
        return ref.dist2(rows, np.zeros_like(rows[0]), cols)
    return make_step, norms2, seen


def test_screen_drops_non_finite_clients(caplog):
    rows, counts, _ = ref.robust_clients(9, 0)
    rows[2, 17] = np.nan
    rows[5, 100] = np.inf
    rows[7, :] = 3e38  # finite, but its differences could overflow fp32
    a = weights_of(counts)
    make_step, norms2, seen = _screen_setup(rows)
    with caplog.at_level(logging.WARNING):
        z, w, info, alive = dfn.geometric_median_screened(make_step, norms2, a, 1e-6, 16, 0.0)
    assert info.dropped == [2, 5, 7] == ref.screen(rows) and alive == [0, 1, 3, 4, 6, 8]
    assert seen == [list(range(9)), alive]  # one restart
    assert "[2, 5, 7]" in caplog.text
    assert w[[2, 5, 7]].tolist() == [0.0, 0.0, 0.0] and abs(w.sum() - 1.0) < 1e-12
    kept = 0.0
    for i in alive:
        kept += a[i]
    zr, wr, fr = ref.loop(rows[alive], [a[i] / kept for i in alive], 1e-6, 16, 0.0)
    np.testing.assert_allclose(w[alive], wr, rtol=1e-9, atol=0)
    assert np.all(np.isfinite(z))


def test_screen_costs_an_honest_round_nothing():
    rows, counts, _ = ref.robust_clients(9, 2)
    make_step, _, seen = _screen_setup(rows)

    def norms2():
        raise AssertionError("the screen ran on a finite round")
    z, w, info, alive = dfn.geometric_median_screened(make_step, norms2, weights_of(counts), 1e-6, 4, 0.0)
    assert info.dropped == [] and alive == list(range(9)) and len(seen) == 1


def test_screen_refuses_half_the_weight():
    rows, _, _ = ref.robust_clients(9, 0)
    rows = rows[:4]
    rows[1, 0] = np.nan
    rows[3, 5] = -np.inf
    make_step, norms2, _ = _screen_setup(rows)
    with pytest.raises(ValueError, match="half"):
        dfn.geometric_median_screened(make_step, norms2, weights_of([10, 10, 10, 10]), 1e-6, 16, 0.0)
    # just under half goes through
    z, w, info, alive = dfn.geometric_median_screened(make_step, norms2, weights_of([10, 10, 11, 9]), 1e-6, 16, 0.0)
    assert info.dropped == [1, 3]


def test_screen_reports_what_it_cannot_fix():
    rows, _, _ = ref.robust_clients(9, 0)
    make_step, norms2, _ = _screen_setup(rows)

    def nan_step(alive):
        return lambda w32: (rows[0], np.full(len(alive), np.nan))
    with pytest.raises(RuntimeError):  # non-finite D, every norm finite
        dfn.geometric_median_screened(nan_step, norms2, weights_of([1] * 9), 1e-6, 16, 0.0)


# ---- the C ABI and the plugin surface, without a GPU ----------------------------

@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


def test_wsum_dist2_argument_validation_without_gpu(lib):
    f = lib.fedagg_wsum_dist2_f32
    p = 64  # any non-null address: every case returns before a HIP call
    assert nat.GEOMED_MAX_CLIENTS == 128 and nat.WORK_WSUM_DIST2 == 3
    assert f(p, p, 0, p, 1, p, p, p, 1024, 0, None) == -1  # K < 1
    assert b"K must be" in lib.fedagg_last_error()
    assert f(p, p, 4, p, -1, p, p, p, 1024, 0, None) == -1  # n_chunks < 0
    for hole in (0, 1, 3, 5, 6, 7):  # d_src, d_w, d_chunks, d_z, d_dist2, d_work: a null pointer
        a = [p, p, 4, p, 1, p, p, p, 1024, 0, None]
        a[hole] = None
        assert f(*a) == -1, hole
        assert b"null pointer" in lib.fedagg_last_error()
    assert f(p, p, 4, p, 1, p, p, p, 3, 0, None) == -1  # a workspace shorter than K doubles
    assert b"workspace" in lib.fedagg_last_error()
    assert f(p, p, 129, p, 1, p, p, p, 1 << 20, 0, None) == -2  # FEDAGG_ENOKERNEL: callers run the pair
    assert b"128" in lib.fedagg_last_error()
    assert f(p, p, 4096, p, 1, p, p, p, 1 << 20, nat.FEDAGG_HOST_WEIGHTS, None) == -2


def test_wsum_dist2_work_len(lib):
    wl = lib.fedagg_robust_work_len
    assert wl(nat.WORK_WSUM_DIST2, 128, 0) == 0
    assert wl(nat.WORK_WSUM_DIST2, 128, 10) == 128 * 10  # one partial per client and block
    assert wl(nat.WORK_WSUM_DIST2, 5, 1) == 5
    assert 4 <= wl(nat.WORK_WSUM_DIST2, 4, 1 << 20) <= 4 * 4096  # the grid is capped
    assert wl(nat.WORK_WSUM_DIST2, 129, 1) == -1
    assert wl(nat.WORK_WSUM_DIST2, 0, 1) == -1 and wl(nat.WORK_WSUM_DIST2, 4, -1) == -1


def test_plugin_accepts_geomed_and_still_refuses_fedmls_names():
    from fedml_amd.server_aggregator import _check_flags

    assert dfn.DEFENSE_GEOMED == "geomed" and "geomed" in dfn.SUPPORTED
    A = type("A", (), {"enable_defense": True, "defense_type": "geomed"})
    _check_flags(A())
    for name in ("geometric_median", "RFA"):
        with pytest.raises(NotImplementedError):
            _check_flags(type("B", (), {"enable_defense": True, "defense_type": name})())


def test_auto_takes_the_pair_above_the_kernels_limit():
    assert dfn.GEOMED_MAX_CLIENTS == 128
    assert not dfn.geomed_auto_fused(129) and not dfn.geomed_auto_fused(4096)
    assert set(dfn.GEOMED_AUTO_FUSED) == {8, 16, 32, 64, 128}
    assert dfn.geomed_auto_fused(1) == dfn.GEOMED_AUTO_FUSED[8]
    assert dfn.geomed_auto_fused(33) == dfn.GEOMED_AUTO_FUSED[64]
    assert dfn.geomed_auto_fused(128) == dfn.GEOMED_AUTO_FUSED[128]


def test_host_side_errors_need_no_gpu():
    d = OrderedDict(w=torch.ones(3))
    with pytest.raises(ZeroDivisionError):
        dfn.geometric_median([(0, d), (0, d)])
    with pytest.raises(KeyError):
        dfn.geometric_median([(1, d), (1, OrderedDict(v=torch.ones(3)))])
    with pytest.raises(ValueError):
        dfn.geometric_median([(1, d)], method="fastest")
    with pytest.raises(ValueError):
        dfn.geometric_median([(1, d)] * 129, method="fused")
    h = OrderedDict(w=torch.ones(3, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError):
        dfn.geometric_median([(1, h), (1, h)])
    assert dfn.geometric_median([(1, OrderedDict()), (2, OrderedDict())]) == OrderedDict()
