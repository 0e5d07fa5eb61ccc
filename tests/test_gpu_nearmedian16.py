"""fedagg_nearmedian_mean_16 / fedagg_nearmedian_mean_wide_16 (Bulyan's stage 2
on bf16 / f16 rows) and bulyan() on 16-bit models, bit for bit against the
two-pointer reference (tests/bulyan_ref.py) on the exactly widened rows,
rounded once to the rows' dtype on the CPU."""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bulyan_ref as br
import test_gpu_bulyan as tgb
import trimmed_mean_ref as tmr
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
offsets = pytest.mark.parametrize("offset", [0, 1], ids=["own", "offset1"])
INF, NAN = br.INF, br.NAN


def _ref(x: torch.Tensor, keep: int) -> torch.Tensor:
    return br.nearmedian_mean_ref(x.float(), keep).to(x.dtype)


class _Rows:
    """test_gpu_bulyan._Rows for 16-bit rows: every row its own allocation,
    `offset` elements into it, and the output likewise."""

    def __init__(self, x: torch.Tensor, dev, offset: int = 0):
        self.K, self.N = x.shape
        self.dev, self.offset, self.dtype = dev, offset, x.dtype
        xd = x.to(dev)
        self.rows = []
        for i in range(self.K):
            buf = torch.empty(self.N + offset, dtype=x.dtype, device=dev)
            buf[offset:] = xd[i]
            self.rows.append(buf[offset:])
        self.ptrs = kn.upload_i64([r.data_ptr() for r in self.rows], dev)

    def run(self, fn, keep: int, N: "int | None" = None) -> torch.Tensor:
        N = self.N if N is None else N
        out = torch.full((N + self.offset,), 7.0, dtype=self.dtype, device=self.dev)[self.offset:]
        fn(self.ptrs, self.K, N, keep, out)
        torch.cuda.synchronize(self.dev)
        return out.cpu()


@functools.lru_cache(maxsize=None)
def _case(K: int, N: int, dtype):
    """Rows with a NaN, +inf and -inf planted one per column, and the
    reference per keep; shared by both offsets."""
    x = tmr.make_rows(K, N, dtype, seed=7000 + K)
    if K >= 3:
        x[0, 50], x[1, 51], x[2, 52] = NAN, INF, -INF
    return x, {keep: _ref(x, keep) for keep in br.keeps(K)}


def _check_kernel(fn, K, NS, dtype, offset, dev):
    x, refs = _case(K, max(NS), dtype)
    rows = _Rows(x, dev, offset)
    for keep, ref in refs.items():
        for N in NS:  # columns are independent: a prefix of the rows gives a prefix
            tmr.assert_same(rows.run(fn, keep, N), ref[:N], f"K={K} keep={keep} N={N} offset={offset}")


@offsets
@dtypes
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 16, 17, 33, 64, 65, 97, 128])
def test_narrow_kernel(K, dtype, offset, cuda_device):
    _check_kernel(dfn.nearmedian_mean_rows16, K, [1, 63, 65, 4099], dtype, offset, cuda_device)


@offsets
@dtypes
@pytest.mark.parametrize("K", [129, 256, 257, 512, 513, 1024])
def test_wide_kernel(K, dtype, offset, cuda_device):
    _check_kernel(dfn.nearmedian_mean_rows_wide16, K, [1, 65, 4099], dtype, offset, cuda_device)


@dtypes
@pytest.mark.parametrize("K,alphabet", [(K, br.ALPHABET9) for K in range(1, 6)] + [(8, br.ALPHABET5)],
                         ids=[f"K{K}" for K in (1, 2, 3, 4, 5, 8)])
def test_exhaustive_small_columns(K, alphabet, dtype, cuda_device):
    x = br.all_columns(alphabet, K).to(dtype)
    rows = _Rows(x, cuda_device)
    for keep in range(1, K + 1):
        tmr.assert_same(rows.run(dfn.nearmedian_mean_rows16, keep), _ref(x, keep), f"K={K} keep={keep}")


@dtypes
@pytest.mark.parametrize("K", [9, 128])
def test_planted_fp32_distances(K, dtype, cuda_device):
    """keep = r + 1: after the r values equal to the median the last step
    chooses between rank 0 and rank r + 1 by their fp32 distances."""
    r = (K - 1) // 2
    keep = r + 1
    fi = torch.finfo(dtype)
    big, tiny = fi.max, fi.tiny * fi.eps  # the largest finite value, the smallest subnormal
    x = tmr.make_rows(K, 8, dtype, seed=377 + K)
    # -inf, r times -big (the median), +big: big - (-big) overflows fp32 for bf16
    # and ties with the -inf side, which is left; for f16 it is finite and wins
    x[:, 0] = big
    x[0, 0], x[1:r + 1, 0] = -INF, -big
    # -big, r times tiny (the median), +big: |-big - tiny| and |big - tiny| both
    # round to big in fp32, so the exactly nearer +big ties with -big: left
    x[:, 1] = big
    x[0, 1], x[1:r + 1, 1] = -big, tiny
    x[:, 2] = 0.0
    x[:r + 1, 2] = -0.0  # -0 == +0: every step ties, the window stays on the -0 side
    x[:K - r, 3] = INF  # the median is +inf
    x[:K - r, 4] = NAN  # the median is a NaN
    assert float(x[1, 1]) == tiny and float(x[2, 0]) == -big
    ref = _ref(x, keep)
    assert ref[0].item() == -INF if dtype == torch.bfloat16 else -big < ref[0].item() < 0
    assert -big < ref[1].item() < 0
    assert ref[2].item() == 0 and bool(torch.signbit(ref[2]))
    assert ref[3].item() == INF and bool(torch.isnan(ref[4]))
    tmr.assert_same(_Rows(x, cuda_device).run(dfn.nearmedian_mean_rows16, keep), ref, f"K={K}")
    tmr.assert_same(_Rows(x, cuda_device).run(dfn.nearmedian_mean_rows_wide16, keep), ref, f"K={K} wide")


# ---- bulyan() on a 16-bit model -------------------------------------------------

def _to16(d, dtype):
    return OrderedDict((k, t.to(dtype) if t.is_floating_point() else t) for k, t in d.items())


def _ref16(host, f, dtype):
    """bulyan_ref on the widened clients; float keys rounded once to dtype."""
    ref, selected, _, D = br.bulyan_ref(host, f)
    like = host[0][1]
    return OrderedDict((k, t.to(dtype) if like[k].is_floating_point() else t) for k, t in ref.items()), selected, D


@functools.lru_cache(maxsize=None)
def _e2e_reference(dtype):
    host = [(n, _to16(d, dtype)) for n, d in tgb._clients()]
    ref, selected, D = _ref16(host, tgb.F_E2E, dtype)
    gaps = []
    br.bulyan_select_ref(D, tgb.F_E2E, gaps)
    assert min(gaps) > 1e-4, gaps  # against the 16-bit Gram's 2e-6
    assert not set(selected) & set(tgb.BYZ) and len(selected) == tgb.K_E2E - 2 * tgb.F_E2E
    return host, ref, selected


def _check_result(out, ref, like, dtype):
    assert isinstance(out, OrderedDict) and list(out.keys()) == list(like.keys())
    for k, t in out.items():
        assert t.dtype == (dtype if like[k].is_floating_point() else torch.float32), k
        assert t.shape == like[k].shape and t.device == like[k].device, k
        tmr.assert_same(t.reshape(-1), ref[k].reshape(-1), k)


@pytest.mark.parametrize("device_inputs", [False, True], ids=["host", "device"])
@dtypes
def test_defense_end_to_end(dtype, device_inputs, cuda_device):
    host, ref, selected = _e2e_reference(dtype)
    raw = host
    if device_inputs:
        raw = [(n, OrderedDict((k, t.to(cuda_device)) for k, t in d.items())) for n, d in host]
    ids = [{k: id(t) for k, t in d.items()} for _, d in raw]
    before = [{k: t.clone() for k, t in d.items()} for _, d in raw]
    out, info = dfn.bulyan(raw, tgb.F_E2E, cuda_device, method="exact", return_info=True)
    assert info.selected == selected and (info.theta, info.beta) == (7, 3)
    _check_result(out, ref, raw[0][1], dtype)
    assert out["bn.num_batches_tracked"].dtype == torch.float32
    for (_, d), i, b in zip(raw, ids, before):  # no client dict is modified
        for k, t in d.items():
            assert id(t) == i[k] and t.dtype == b[k].dtype, k
            assert torch.equal(tmr.bits(t.float()), tmr.bits(b[k].float())), k
    out2, info2 = dfn.bulyan(raw, tgb.F_E2E, cuda_device, method="auto", return_info=True)
    assert set(info2.selected) == set(selected)
    _check_result(out2, ref, raw[0][1], dtype)


@dtypes
def test_above_128_selected_clients(dtype, cuda_device):
    """test_gpu_bulyan's K = 134, f = 2 construction in 16-bit rows: the wide
    kernel or the torch path, whichever NEARMEDIAN_WIDE16_AUTO picks."""
    K, f, N = 134, 2, 300
    spread = [0.05] * 130 + [0.15, 0.15, 5.0, 5.0]
    g = torch.Generator().manual_seed(7)
    centre = torch.randn(N, generator=g)
    x = torch.stack([centre + spread[i] * torch.randn(N, generator=g) for i in range(K)]).to(dtype)
    y = tmr.make_rows(K, 64, torch.float32, seed=8).to(dtype)
    y[5, 50], y[9, 51], y[11, 52] = NAN, INF, -INF
    y[20:26, 53] = NAN  # more than theta - beta of them: the window reaches a NaN
    host = [(1, OrderedDict([("w", x[i].clone()), ("bn.running_mean", y[i].clone())])) for i in range(K)]
    ref, selected, D = _ref16(host, f, dtype)
    assert set(selected) == set(range(130))
    e = np.random.default_rng(1).uniform(-1e-5, 1e-5, size=D.shape)
    assert set(br.bulyan_select_ref(D * (1 + np.triu(e, 1) + np.triu(e, 1).T), f)[0]) == set(selected)
    assert bool(torch.isnan(ref["bn.running_mean"][53])) and not bool(torch.isnan(ref["bn.running_mean"][50]))
    raw = [(n, OrderedDict((k, t.to(cuda_device)) for k, t in d.items())) for n, d in host]
    out, info = dfn.bulyan(raw, f, method="exact", return_info=True)
    assert set(info.selected) == set(selected) and (info.theta, info.beta) == (130, 126)
    for k, rows in (("w", x), ("bn.running_mean", y)):
        assert out[k].is_cuda and out[k].dtype == dtype
        tmr.assert_same(out[k], ref[k], f"K={K} {k}")
        got = dfn.nearmedian_mean_rows16_torch(rows[selected].to(cuda_device), 126, chunk_cols=100)
        tmr.assert_same(got, ref[k], f"K={K} {k} torch path")
