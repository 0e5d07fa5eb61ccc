"""The coordinate-wise trimmed mean without a GPU: the torch slow path against
the numpy reference (tests/trimmed_mean_ref.py), the C entry's argument
checks, and the defense's host-side validation."""
from __future__ import annotations

from collections import OrderedDict

import pytest
import torch

import trimmed_mean_ref as tmr
from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn
from fedml_amd import server_aggregator as sa

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


def _plant(x: torch.Tensor) -> torch.Tensor:
    """NaN (both signs), +-inf and an all-equal column in the last columns."""
    K = x.shape[0]
    x = x.clone()
    x[0, -1] = float("nan")
    x[K // 2, -2] = -float("nan")
    x[: (K + 1) // 2, -3] = float("nan")
    x[0, -4] = float("inf")
    x[K - 1, -5] = -float("inf")
    x[0, -6] = float("inf")
    x[K - 1, -6] = -float("inf")
    x[:, -7] = 0.125
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 9, 33, 128, 130, 200])
def test_torch_path_equals_reference(K, dtype):
    N = 257
    x = _plant(tmr.make_rows(K, N, dtype, seed=K))
    assert bool(torch.signbit(x[:, :16].float()).any()) and bool((x[:, :16] == 0).all())
    for trim in tmr.trims(K):
        ref = tmr.trimmed_mean_ref(x, trim)
        got = dfn.trimmed_mean_rows_torch(x, trim)
        tmr.assert_same(got, ref, f"K={K} trim={trim} {dtype}")
        # a list of rows, in chunks that do not divide N
        got = dfn.trimmed_mean_rows_torch([x[i] for i in range(K)], trim, chunk_cols=100)
        tmr.assert_same(got, ref, f"K={K} trim={trim} {dtype} chunked")


def test_reference_basics():
    """The reference itself on columns worked by hand."""
    x = torch.tensor([[1.0, -0.0, float("nan"), float("inf")],
                      [5.0, -0.0, 2.0, -float("inf")],
                      [2.0, -0.0, 4.0, 1.0],
                      [-7.0, -0.0, -float("nan"), 3.0],
                      [3.0, -0.0, 6.0, 2.0]])
    r1 = tmr.trimmed_mean_ref(x, 1)
    assert r1[0].item() == 2.0  # (1 + 2 + 3) / 3
    assert r1[1].item() == 0.0 and bool(torch.signbit(r1[1]))  # an all -0 column stays -0
    assert bool(torch.isnan(r1[2]))  # two NaNs, one trimmed
    assert r1[3].item() == 2.0  # both infinities trimmed
    r2 = tmr.trimmed_mean_ref(x, 2)
    assert r2[2].item() == 6.0  # NaNs rank above everything: sorted 2 4 6 NaN NaN
    r0 = tmr.trimmed_mean_ref(x, 0)
    assert bool(torch.isnan(r0[3]))  # +inf and -inf both kept


def test_torch_path_rejects_bad_trim():
    x = torch.zeros((4, 3))
    for trim in (-1, 2, 3):
        with pytest.raises(ValueError):
            dfn.trimmed_mean_rows_torch(x, trim)
    with pytest.raises(TypeError):
        dfn.trimmed_mean_rows_torch(x.double(), 1)


def test_abi_validation_without_gpu(lib):
    f = lib.fedagg_trimmed_mean
    ok = (nat.DT_F32, 1, 4, 10, 1, 1, 0, None)  # dtype, src, K, N, trim, out, flags, stream

    def call(**kw):
        a = dict(zip(("dtype", "src", "K", "N", "trim", "out", "flags", "stream"), ok))
        a.update(kw)
        return f(*a.values())

    assert call(K=0) == -1
    assert b"K must be" in lib.fedagg_last_error()
    assert call(N=-1) == -1
    assert call(trim=-1) == -1
    assert b"trim" in lib.fedagg_last_error()
    assert call(trim=2) == -1  # 2 * trim == K
    assert call(K=5, trim=3) == -1
    assert call(src=None) == -1
    assert b"null" in lib.fedagg_last_error()
    assert call(out=None) == -1
    for dt in (nat.DT_F64, nat.DT_I64, nat.DT_I32, 99, -1):
        assert call(dtype=dt) == -1
        assert b"dtype" in lib.fedagg_last_error()
    assert call(K=129, trim=1) == -2  # FEDAGG_ENOKERNEL
    assert b"128" in lib.fedagg_last_error()
    assert call(K=129, trim=70) == -1  # an invalid trim is EINVAL whatever K is
    for dt in (nat.DT_F32, nat.DT_BF16, nat.DT_F16):
        assert call(dtype=dt, N=0) == 0
    assert call(K=1, trim=0, N=0) == 0
    assert nat.TRIMMED_MAX_CLIENTS == 128 == dfn.TRIMMED_MAX_CLIENTS


class _Args:
    def __init__(self, **kw):
        self.federated_optimizer = "FedAvg"
        self.enable_defense = True
        self.__dict__.update(kw)


def test_check_flags_wants_beta():
    assert "wise_trimmed_mean" in dfn.SUPPORTED and dfn.DEFENSE_WISE_TRIMMED_MEAN == "wise_trimmed_mean"
    sa._check_flags(_Args(defense_type="wise_trimmed_mean", beta=0.2))
    with pytest.raises(AttributeError):
        sa._check_flags(_Args(defense_type="wise_trimmed_mean"))
    # FedML's per-client trimmed mean keeps its name and its meaning
    assert dfn.DEFENSE_TRIMMED_MEAN == "trimmed_mean"
    lst = [(n, OrderedDict(a=torch.full((2,), float(n)))) for n in (5, 1, 9, 3, 7)]
    kept = dfn.trimmed_mean_before_aggregation(lst, 0.2)
    assert [n for n, _ in kept] == [3, 5, 7]


@pytest.mark.parametrize("beta", [-0.1, 0.5, 0.6])
def test_beta_bounds(beta):
    lst = [(1, OrderedDict(a=torch.ones(3))) for _ in range(4)]
    with pytest.raises(ValueError):
        dfn.coordinate_wise_trimmed_mean(lst, beta)
