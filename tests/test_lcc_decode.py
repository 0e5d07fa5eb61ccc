"""The host side of the LightSecAgg mask decode: the Lagrange coefficients
(fedml_amd.secagg.lagrange_coeffs) and fedagg_lcc_decode_i64's argument checks,
which stand before any HIP call."""
from __future__ import annotations

import numpy as np
import pytest

from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import secagg


@pytest.mark.parametrize("U,p", [(1, 2), (3, 7), (5, 2 ** 15 - 19), (12, 65269), (9, 2 ** 31 - 1), (6, 2 ** 61 - 1)])
def test_lagrange_coeffs_recover_a_polynomial(U, p):
    rng = np.random.default_rng(U)
    poly = [int(c) for c in rng.integers(0, min(p, 2 ** 62), U)]  # degree U - 1
    value = lambda x: sum(c * pow(int(x), k, p) for k, c in enumerate(poly)) % p  # noqa: E731
    alpha = [int(a) for a in rng.choice(min(p, 1000), U, replace=False)]
    beta = list(range(1000, 1004))
    C = secagg.lagrange_coeffs(beta, alpha, p)
    assert C.dtype == np.int64 and C.shape == (4, U) and C.min() >= 0 and C.max() < p
    for t, b in enumerate(beta):
        assert sum(int(C[t, j]) * value(a) for j, a in enumerate(alpha)) % p == value(b)


def test_lagrange_coeffs_refuse_repeated_points_and_bad_moduli():
    with pytest.raises(ValueError):
        secagg.lagrange_coeffs([9], [1, 2, 1], 32749)
    with pytest.raises(ValueError):
        secagg.lagrange_coeffs([9], [1, 8], 7)  # equal mod p
    with pytest.raises(ValueError):
        secagg.lagrange_coeffs([9], [1, 2], 1)


def test_argument_validation_without_gpu():
    fbuild.build()
    lib, a = nat.lib(), 64  # a: never dereferenced
    call = lambda U, M, R, p, n_out, method, src=a, work=a, nbytes=1 << 30: lib.fedagg_lcc_decode_i64(  # noqa: E731
        src, U, M, a, R, p, a, n_out, method, work, nbytes, None)
    for args, msg in [((0, 10, 3, 7, 30, 0), b"U and R must be"), ((3, 10, 0, 7, 0, 0), b"U and R must be"),
                      ((3, -1, 3, 7, 0, 0), b"M >= 0"), ((3, 10, 3, 0, 30, 0), b"prime must be positive"),
                      ((3, 10, 3, 7, 31, 0), b"n_out"), ((3, 10, 3, 7, -1, 1), b"n_out"),
                      ((3, 10, 3, 7, 30, 2), b"method"), ((3, 10, 3, 7, 30, 0, None), b"null pointer"),
                      ((3, 10, 3, 7, 30, 1, a, None), b"d_work"), ((3, 10, 3, 7, 30, 1, a, a, 100), b"d_work"),
                      ((3, 10, 3, 7, 30, 1, a, 72), b"16-byte aligned")]:
        assert call(*args) == -1, args
        err = lib.fedagg_last_error()
        assert err.startswith(b"fedagg_lcc_decode_i64: ") and msg in err, (args, err)
    assert call(1025, 10, 3, 7, 30, 0) == -2 and call(3, 10, 1025, 7, 30, 1) == -2  # FEDAGG_ENOKERNEL
    assert b"at most 1024" in lib.fedagg_last_error()
    assert call(3, 10, 3, 7, 0, 1) == 0 and call(3, 0, 3, 7, 0, 0) == 0  # nothing to write: no launch
    assert lib.fedagg_lcc_work_bytes(3, 3, 10) == 2 * 64 * 32 + 4 * 32 + 4
    assert lib.fedagg_lcc_work_bytes(1024, 1024, 129) == 2 * 1024 * 1024 + 4 * 1024 + 4 * 3
    assert lib.fedagg_lcc_work_bytes(1025, 3, 10) == -1 and lib.fedagg_lcc_work_bytes(3, 0, 10) == -1
