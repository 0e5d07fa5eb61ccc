"""fedagg_trimmed_mean_wide without a GPU: the C entry's argument checks (all
made before any HIP call), its cap, and the old entry's cap unchanged."""
from __future__ import annotations

import pytest

from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn


@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


def _caller(f):
    ok = (nat.DT_F32, 1, 300, 10, 30, 1, 0, None)  # dtype, src, K, N, trim, out, flags, stream

    def call(**kw):
        a = dict(zip(("dtype", "src", "K", "N", "trim", "out", "flags", "stream"), ok))
        a.update(kw)
        return f(*a.values())

    return call


def test_einval_cases(lib):
    call = _caller(lib.fedagg_trimmed_mean_wide)
    assert call(K=0) == -1
    assert b"K must be" in lib.fedagg_last_error()
    assert call(K=-5) == -1
    assert call(N=-1) == -1
    assert b"N >= 0" in lib.fedagg_last_error()
    assert call(trim=-1) == -1
    assert b"trim" in lib.fedagg_last_error()
    assert call(trim=150) == -1  # 2 * trim == K
    assert call(K=4, trim=2) == -1
    assert call(K=5, trim=3) == -1
    assert call(K=1, trim=1) == -1
    assert call(src=None) == -1
    assert b"null" in lib.fedagg_last_error()
    assert call(out=None) == -1
    assert b"null" in lib.fedagg_last_error()
    for dt in (nat.DT_F64, nat.DT_I64, nat.DT_I32, 99, -1):
        assert call(dtype=dt) == -1
        assert b"dtype" in lib.fedagg_last_error()


def test_grid_bound(lib):
    """A block holds 64 columns up to 512 clients and 32 above: the first N
    whose grid passes 2^31 - 1 blocks is refused, for every tier."""
    call = _caller(lib.fedagg_trimmed_mean_wide)
    for K, cols in ((1, 64), (300, 64), (512, 64), (513, 32), (1024, 32)):
        assert call(K=K, trim=0, N=(2 ** 31 - 1) * cols + 1) == -1, K
        assert b"N too large" in lib.fedagg_last_error()
    assert call(N=2 ** 62) == -1


def test_cap(lib):
    call = _caller(lib.fedagg_trimmed_mean_wide)
    assert call(K=1025, trim=1) == -2  # FEDAGG_ENOKERNEL
    msg = lib.fedagg_last_error()
    assert b"1024" in msg and b"1025" in msg
    assert call(K=1025, trim=600) == -1  # an invalid trim is EINVAL whatever K is
    assert call(K=1025, trim=-1) == -1
    assert call(K=5000, trim=0, N=0) == -2
    assert nat.TRIMMED_WIDE_MAX_CLIENTS == 1024 == dfn.TRIMMED_WIDE_MAX_CLIENTS


def test_no_columns_is_ok(lib):
    call = _caller(lib.fedagg_trimmed_mean_wide)
    for dt in (nat.DT_F32, nat.DT_BF16, nat.DT_F16):
        for K, trim in ((1, 0), (128, 12), (129, 12), (300, 30), (1024, 511)):
            assert call(dtype=dt, K=K, trim=trim, N=0) == 0


def test_old_entry_keeps_its_cap(lib):
    call = _caller(lib.fedagg_trimmed_mean)
    assert call(K=129, trim=1) == -2
    assert b"128" in lib.fedagg_last_error()
    assert call(K=128, trim=1, N=0) == 0
    assert nat.TRIMMED_MAX_CLIENTS == 128 == dfn.TRIMMED_MAX_CLIENTS


def test_dispatch_table():
    """Every tier of the wide kernel has an entry; nothing above the cap or at
    or below the old kernel's cap is decided by it."""
    assert sorted(dfn.TRIMMED_WIDE_AUTO) == [256, 512, 1024]
    assert all(isinstance(v, bool) for v in dfn.TRIMMED_WIDE_AUTO.values())
    for K, tier in ((129, 256), (256, 256), (257, 512), (512, 512), (513, 1024), (1024, 1024)):
        assert dfn.trimmed_wide_auto(K) is dfn.TRIMMED_WIDE_AUTO[tier]
    assert dfn.trimmed_wide_auto(1025) is False
