"""LightSecAgg's mask decode on the GPU (fedagg_lcc_decode_i64, csrc/lccdecode.hip)
through fedml_amd.secagg, both kernels, every comparison exact.

Shapes sit at the kernels' edges: the matrix-core kernel pads U to 64 (one
MFMA's k) and R to 32, a block owns 64 columns and a wave 2 x 2 tiles of 16;
the exact kernel holds 16 rows per lane, takes the source rows in pairs (odd U:
a tail step) and its blocks span 256 columns."""
from __future__ import annotations

import copy
from collections import OrderedDict

import numpy as np
import pytest
import torch

import secagg_ref as ref
from fedml_amd import _native as nat
from fedml_amd import secagg

pytestmark = pytest.mark.gpu

P_MAX = 65269  # the largest prime <= FEDAGG_LCC_MFMA_MAX_PRIME = 65279
PRIMES = [3, 2 ** 15 - 19, P_MAX]
SHAPES = [(1, 1, 1), (63, 15, 63), (64, 17, 65), (65, 1, 131), (130, 17, 131), (3, 33, 259)]  # U, R, M
METHODS = ["valu", "mfma"]


def exact(C, F, p):
    """Σ in Python integers, then % p."""
    return np.array((C.astype(object).dot(F.astype(object)) % p).tolist(), dtype=np.int64)


def decode(C, F, p, method, **kw):
    return secagg.lcc_decode(list(F), C, p, method=method, **kw).cpu().numpy()


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("U,R,M", SHAPES)
@pytest.mark.parametrize("method", METHODS)
def test_field_data_against_python_integers(method, U, R, M, p):
    rng = np.random.default_rng(U * 1000 + R)
    C, F = rng.integers(0, p, (R, U)), rng.integers(0, p, (U, M))
    want = exact(C, F, p)
    assert np.array_equal(decode(C, F, p, method).reshape(R, M), want)
    # n_out ends mid-row (or mid-element of the only row): the guard behind it stays
    n_out = (R - 1) * M + M // 2
    buf = torch.full((R * M + 8,), -7, dtype=torch.int64, device="cuda")
    got = secagg.lcc_decode([torch.from_numpy(f).cuda() for f in F], C, p, n_out=n_out, method=method, out=buf)
    assert got.numel() == n_out and np.array_equal(got.cpu().numpy(), want.reshape(-1)[:n_out])
    assert bool((buf[n_out:] == -7).all())


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("method", METHODS)
def test_centring_boundary_and_digit_extremes(method, p):
    U, R, M = 65, 17, 65
    for a in (0, (p - 1) // 2, (p + 1) // 2, p - 1):
        for b in (0, (p - 1) // 2, (p + 1) // 2, p - 1):
            got = decode(np.full((R, U), a), np.full((U, M), b), p, method)
            assert np.array_equal(got, np.full(R * M, U * a * b % p)), (a, b)


@pytest.mark.parametrize("method", METHODS)
def test_int32_headroom_at_1024_rows(method):
    U, R, M, v = 1024, 17, 17, (P_MAX + 1) // 2
    got = decode(np.full((R, U), v), np.full((U, M), v), P_MAX, method)
    assert np.array_equal(got, np.full(R * M, U * v * v % P_MAX))


@pytest.mark.parametrize("method", METHODS)
def test_numpy_semantics_outside_the_field(method):
    """One column tile (64 .. 127) holds elements outside [0, p): the whole
    product is numpy's wrapping int64 (C.dot(F)) % p, the other tiles included;
    the same for one coefficient outside the field."""
    p, (U, R, M) = 2 ** 15 - 19, (65, 17, 131)
    rng = np.random.default_rng(5)
    C, F = rng.integers(0, p, (R, U)), rng.integers(0, p, (U, M))
    for k, v in enumerate([-1, p, 2 ** 63 - 1, -2 ** 63]):
        F[7 * k + 3, 70 + 11 * k] = v
    assert np.array_equal(decode(C, F, p, method).reshape(R, M), C.dot(F) % p)
    F = rng.integers(0, p, (U, M))
    for v in (-1, p, -2 ** 63):
        C2 = C.copy()
        C2[R - 1, U - 1] = v
        assert np.array_equal(decode(C2, F, p, method).reshape(R, M), C2.dot(F) % p)


@pytest.mark.parametrize("p", [m for m in ref.MODULI if m > nat.LCC_MFMA_MAX_PRIME])
@pytest.mark.parametrize("method", METHODS)
def test_moduli_above_the_byte_bound_take_the_exact_kernel(method, p):
    rng = np.random.default_rng(9)
    C, F = rng.integers(0, p, (17, 65)), rng.integers(0, p, (65, 67))
    F[1, 2], F[3, 66] = -2 ** 63, 2 ** 63 - 1
    assert np.array_equal(decode(C, F, p, method).reshape(17, 67), C.dot(F) % p)


@pytest.mark.parametrize("method", METHODS)
def test_mask_reconstruction_end_to_end(method):
    """N = 8 clients, U = 5, T = 2, d = 100 (no multiple of U - T = 3), three
    clients dropped: the decoded aggregate mask is Σ masks mod p, and
    model_reconstruction takes it from the device as from its numpy copy."""
    N, U, T, d, p, q = 8, 5, 2, 100, 2 ** 15 - 19, 8
    M = -(-d // (U - T))
    rng = np.random.default_rng(11)
    masks = rng.integers(0, p, (N, d))
    pieces = np.concatenate([np.pad(masks, ((0, 0), (0, (U - T) * M - d))).reshape(N, U - T, M),
                             rng.integers(0, p, (N, T, M))], axis=1)
    # client i's share for client j: its degree-(U-1) polynomial through (N+1+k, piece k), evaluated at j + 1
    W = secagg.lagrange_coeffs(range(1, N + 1), range(N + 1, N + U + 1), p)
    shares = [exact(W, pieces[i], p) for i in range(N)]
    active = [6, 0, 3, 7, 2]
    encoded = {j: sum(shares[i][j] for i in active) % p for j in active}
    d_mask = secagg.aggregate_mask_reconstruction(encoded, active, N, U, T, d, p, method=method)
    assert d_mask.is_cuda and d_mask.shape == (d, 1)
    assert np.array_equal(d_mask.cpu().numpy().reshape(-1), masks[active].sum(axis=0) % p)
    models = {c: OrderedDict(w=rng.integers(0, p, (7, 9)), b=rng.integers(0, p, 37)) for c in active}
    a = secagg.model_reconstruction(copy.deepcopy(models), active, d_mask, p, q)
    b = secagg.model_reconstruction(copy.deepcopy(models), active, d_mask.cpu().numpy(), p, q)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
