"""fedagg_trimmed_mean on the GPU against the numpy reference
(tests/trimmed_mean_ref.py), bit for bit: every K tier in its full and padded
form, planted NaN / inf / zero columns, the defense end to end and the torch
slow path above 128 clients."""
from __future__ import annotations

from collections import OrderedDict

import pytest
import torch

import trimmed_mean_ref as tmr
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn
from fedml_amd.server_aggregator import MI355XServerAggregator

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 7, 8, 9, 16, 17, 24, 31, 32, 33, 48, 64, 65, 96, 97, 127, 128]
KS_16BIT = [3, 8, 33, 96, 128]
NS = [1, 63, 64, 65, 4099]
DT_IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
KERNEL_CASES = [(K, torch.float32) for K in KS] + [(K, dt) for dt in (torch.bfloat16, torch.float16)
                                                   for K in KS_16BIT]


def _launch(x: torch.Tensor, trim: int, dev, offset: int = 0) -> torch.Tensor:
    """The kernel on the rows of CPU tensor x (K, N): every row its own
    allocation, `offset` elements into it (1: rows and output that are not
    aligned to anything beyond their element)."""
    K, N = x.shape
    rows = []
    for i in range(K):
        buf = torch.empty(N + offset, dtype=x.dtype, device=dev)
        buf[offset:] = x[i].to(dev)
        rows.append(buf[offset:])
    ptrs = kn.upload_i64([r.data_ptr() for r in rows], dev)
    out = torch.full((N + offset,), 7.0, dtype=x.dtype, device=dev)[offset:]
    dfn.trimmed_mean_rows(ptrs, K, N, trim, out)
    torch.cuda.synchronize(dev)
    return out.cpu()


@pytest.mark.parametrize("offset", [0, 1], ids=["own", "offset1"])
@pytest.mark.parametrize("K,dtype", KERNEL_CASES, ids=[f"K{K}-{DT_IDS[dt]}" for K, dt in KERNEL_CASES])
def test_kernel_matches_reference(K, dtype, offset, cuda_device):
    x = tmr.make_rows(K, max(NS), dtype, seed=1000 + K)
    if K >= 3:  # a NaN, an inf of each sign: one per column, trimmed or not by trim
        x[0, 50], x[1, 51], x[2, 52] = float("nan"), float("inf"), -float("inf")
    for trim in tmr.trims(K, extra=(K // 4,)):
        ref = tmr.trimmed_mean_ref(x, trim)  # columns are independent: a prefix of the rows gives a prefix
        for N in NS:
            got = _launch(x[:, :N].contiguous(), trim, cuda_device, offset)
            tmr.assert_same(got, ref[:N], f"K={K} trim={trim} N={N} {dtype} offset={offset}")


def _neg_nan(dtype) -> torch.Tensor:
    v = torch.tensor([-1], dtype=torch.int32 if dtype == torch.float32 else torch.int16).view(dtype)[0]
    assert bool(torch.isnan(v)) and int(tmr.bits(v.reshape(1))[0]) < 0
    return v


@pytest.mark.parametrize("dtype", list(DT_IDS), ids=list(DT_IDS.values()))
@pytest.mark.parametrize("K", [9, 128])
def test_planted_specials(K, dtype, cuda_device):
    trim, N, c0 = 2, 128, 100
    x = tmr.make_rows(K, N, dtype, seed=77 + K)
    inf = float("inf")
    x[1:1 + trim, c0] = float("nan")  # exactly trim NaNs: all trimmed
    x[1:2 + trim, c0 + 1] = float("nan")  # trim + 1 NaNs: NaN
    x[K - 1, c0 + 2] = _neg_nan(dtype)  # a negative-sign NaN ranks above +inf too
    x[0:trim, c0 + 3], x[K - trim:K, c0 + 3] = inf, -inf  # trimmed at both ends
    x[0:trim + 1, c0 + 4], x[K - trim - 1:K, c0 + 4] = inf, -inf  # one of each kept: inf - inf
    x[:, c0 + 5] = -0.0
    x[:, c0 + 6] = 0.3
    ref = tmr.trimmed_mean_ref(x, trim)
    # the NaN carve-out of assert_same covers exactly the two planted columns
    assert torch.nonzero(torch.isnan(ref)).flatten().tolist() == [c0 + 1, c0 + 4]
    assert ref[c0 + 5].item() == 0 and bool(torch.signbit(ref[c0 + 5]))
    assert bool(torch.isfinite(ref[[c0, c0 + 2, c0 + 3]].float()).all())
    got = _launch(x, trim, cuda_device)
    tmr.assert_same(got, ref, f"K={K} {dtype}")
    assert int(tmr.bits(got)[c0 + 5]) == int(tmr.bits(torch.tensor([-0.0], dtype=dtype))[0])


@pytest.mark.parametrize("dtype", list(DT_IDS), ids=list(DT_IDS.values()))
def test_trim_zero_is_the_ascending_mean(dtype, cuda_device):
    K, N = 12, 200
    x = tmr.make_rows(K, N, dtype, seed=5)
    s = torch.sort(x.float(), dim=0).values  # no NaN here; +-0 order cannot change a sum that starts from a value
    acc = s[0].clone()
    for r in range(1, K):
        acc = acc + s[r]
    want = (acc / torch.full((1,), float(K))).to(dtype)
    got = _launch(x, 0, cuda_device)
    nz = want.float() != 0  # a zero's sign follows the total order, which torch.sort does not keep
    assert torch.equal(tmr.bits(got)[nz], tmr.bits(want)[nz])
    tmr.assert_same(got, tmr.trimmed_mean_ref(x, 0), f"trim=0 {dtype}")


@pytest.mark.parametrize("dtype", list(DT_IDS), ids=list(DT_IDS.values()))
def test_one_client_is_the_identity(dtype, cuda_device):
    x = tmr.make_rows(1, 300, dtype, seed=6)
    x[0, 60], x[0, 61], x[0, 62] = float("inf"), -float("inf"), float("nan")
    got = _launch(x, 0, cuda_device, offset=1)
    assert bool(torch.isnan(got[62]))
    keep = torch.arange(300) != 62
    assert torch.equal(tmr.bits(got)[keep], tmr.bits(x[0])[keep])


# ---- the defense end to end ---------------------------------------------------

class _Agg(MI355XServerAggregator):
    def __init__(self, args):
        super().__init__(torch.nn.Linear(1, 1), args)


class _Args:
    federated_optimizer = "FedAvg"
    enable_defense = True
    defense_type = "wise_trimmed_mean"
    beta = 0.2


def _model(seed: int, dtype) -> "OrderedDict[str, torch.Tensor]":
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (0.05 * torch.randn(*s, generator=g)).to(dtype)
    return OrderedDict([
        ("conv.weight", r(4, 3, 3, 3)), ("bn.weight", 1 + r(4)), ("bn.bias", r(4)),
        ("bn.running_mean", r(4)), ("bn.running_var", 1 + r(4).abs()),
        ("bn.num_batches_tracked", torch.tensor(100 + seed, dtype=torch.int64)), ("fc.weight", r(10, 36))])


def _clients(K: int, dtype):
    raw = []
    for i in range(K):
        d = _model(i, dtype)
        if i == 3:  # one client scaled far away
            d = OrderedDict((k, t * 1e6 if t.is_floating_point() else t * 1000) for k, t in d.items())
        if i == 6:  # one client all NaN (its counter: absurd)
            d = OrderedDict((k, torch.full_like(t, float("nan")) if t.is_floating_point() else t * 0 + 10 ** 9)
                            for k, t in d.items())
        raw.append((10 + i, d))
    return raw


@pytest.mark.parametrize("device_inputs", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_defense_end_to_end(dtype, device_inputs, cuda_device):
    K = 10
    host = _clients(K, dtype)
    raw = host
    if device_inputs:
        raw = [(n, OrderedDict((k, t.to(cuda_device)) for k, t in d.items())) for n, d in host]
    first = raw[0][1]
    ids = {k: id(t) for k, t in first.items()}
    before = {k: t.clone() for k, t in first.items()}
    out = _Agg(_Args()).aggregate(raw)
    assert isinstance(out, OrderedDict) and out is not first
    assert list(out.keys()) == list(first.keys())
    trim = int(_Args.beta * K)
    assert trim == 2
    for k, t in out.items():
        stack = torch.stack([d[k].reshape(-1) for _, d in host])
        is_int = not stack.is_floating_point()
        ref = tmr.trimmed_mean_ref(stack.float() if is_int else stack, trim)
        assert t.dtype == (torch.float32 if is_int else dtype), k
        assert t.shape == first[k].shape, k
        assert t.device == first[k].device, k
        assert bool(torch.isfinite(t.float()).all()), k
        tmr.assert_same(t.reshape(-1), ref, k)
    assert out["bn.num_batches_tracked"].dtype == torch.float32
    # client 0's dict: the same tensors, the same values
    assert list(first.keys()) == list(ids)
    for k, t in first.items():
        assert id(t) == ids[k] and torch.equal(t, before[k]), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_slow_path_above_128_clients(dtype, cuda_device):
    K, N = 130, 1000
    x = tmr.make_rows(K, N, dtype, seed=9)
    x[5, 70], x[6, 71], x[7, 72] = float("nan"), float("inf"), -float("inf")
    raw = [(1, OrderedDict(w=x[i].to(cuda_device))) for i in range(K)]
    out = dfn.coordinate_wise_trimmed_mean(raw, 0.1)
    assert out["w"].is_cuda and out["w"].dtype == dtype
    tmr.assert_same(out["w"], tmr.trimmed_mean_ref(x, int(0.1 * K)), f"K={K} {dtype}")
