"""fedagg_nearmedian_mean_f32 and the "wise_bulyan" defense on the GPU against
the two-pointer reference (tests/bulyan_ref.py), bit for bit: every K tier in
its full and padded form, planted NaN / inf / tie columns, every small column
over a small alphabet, the defense end to end and the torch path above 128
selected clients.  The offset variant of the kernel (the launches past 2^30
columns) runs in tests/test_gpu_col_chunks.py, at every tier, on launches of
130 columns; a launch at the true 2^30 boundary is run by no test."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest
import torch

import bulyan_ref as br
import trimmed_mean_ref as tmr
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn
from fedml_amd.server_aggregator import MI355XServerAggregator

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 7, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 127, 128]
NS = [1, 63, 64, 65, 4099]
INF, NAN = br.INF, br.NAN


class _Rows:
    """The rows of CPU tensor x (K, N) on the device: every row its own
    allocation, `offset` elements into it (1: rows and output that are not
    aligned to anything beyond their element)."""

    def __init__(self, x: torch.Tensor, dev, offset: int = 0):
        self.K, self.N = x.shape
        self.dev, self.offset = dev, offset
        self.rows = []
        for i in range(self.K):
            buf = torch.empty(self.N + offset, dtype=torch.float32, device=dev)
            buf[offset:] = x[i].to(dev)
            self.rows.append(buf[offset:])
        self.ptrs = self.table(range(self.K))

    def table(self, order):
        return kn.upload_i64([self.rows[i].data_ptr() for i in order], self.dev)

    def out(self, N):
        return torch.full((N + self.offset,), 7.0, dtype=torch.float32, device=self.dev)[self.offset:]

    def run(self, keep: int, N: "int | None" = None, ptrs=None) -> torch.Tensor:
        """The kernel over the first N columns (columns are independent)."""
        N = self.N if N is None else N
        out = self.out(N)
        dfn.nearmedian_mean_rows(self.ptrs if ptrs is None else ptrs, self.K, N, keep, out)
        torch.cuda.synchronize(self.dev)
        return out.cpu()


@pytest.mark.parametrize("offset", [0, 1], ids=["own", "offset1"])
@pytest.mark.parametrize("K", KS)
def test_kernel_matches_reference(K, offset, cuda_device):
    x = tmr.make_rows(K, max(NS), torch.float32, seed=2000 + K)
    if K >= 3:  # a NaN, an inf of each sign: one per column
        x[0, 50], x[1, 51], x[2, 52] = NAN, INF, -INF
    rows = _Rows(x, cuda_device, offset)
    for keep in br.keeps(K):
        ref = br.nearmedian_mean_ref(x, keep)  # columns are independent: a prefix of the rows gives a prefix
        for N in NS:
            tmr.assert_same(rows.run(keep, N), ref[:N], f"K={K} keep={keep} N={N} offset={offset}")


@pytest.mark.parametrize("K,keep", [(9, 6), (9, 7), (128, 66), (128, 126)])
def test_planted_specials(K, keep, cuda_device):
    N, c0 = 128, 100
    r = (K - 1) // 2
    assert r + 2 <= keep <= K - 2 and keep // 2 <= r
    x = tmr.make_rows(K, N, torch.float32, seed=177 + K)
    # all other values equal: every distance ties, the window goes left first
    n = K - (max(0, r - keep + 1) + keep)
    assert n >= 1
    x[:, c0], x[:, c0 + 1] = 0.25, 0.25
    x[1:1 + n, c0] = NAN  # the window stops one rank short of the first NaN
    x[1:2 + n, c0 + 1] = NAN  # one more: it touches it
    x[:K - r, c0 + 2] = INF  # m = +inf
    x[:K - r, c0 + 3] = NAN  # m a NaN
    # -inf, keep - 2 ones (m among them), K - keep + 1 +inf: the ones go first,
    # then the tie of the two infinities goes left, then right is all that is left
    x[:, c0 + 4] = 1.0
    x[0, c0 + 4] = -INF
    x[keep - 1:, c0 + 4] = INF
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    x[:, c0 + 5] = perm.float() - r  # the integers -r .. K-1-r: symmetric about m = 0
    x[:, c0 + 6] = -0.0
    x[:, c0 + 7] = 0.3
    x[3:3 + n, c0 + 8] = NAN  # the same two NaN counts among random values
    x[3:4 + n, c0 + 9] = NAN
    ref = br.nearmedian_mean_ref(x, keep)
    # the NaN carve-out of assert_same covers the planted columns it should
    assert ref[c0].item() == 0.25 and bool(torch.isnan(ref[c0 + 1]))
    assert ref[c0 + 2].item() == INF
    assert bool(torch.isnan(ref[c0 + 3])) and bool(torch.isnan(ref[c0 + 4]))
    # symmetric about m: with an even keep the odd last step is a tie, which goes left
    assert ref[c0 + 5].item() == (-0.5 if keep % 2 == 0 else 0.0)
    assert ref[c0 + 6].item() == 0 and bool(torch.signbit(ref[c0 + 6]))
    assert ref[c0 + 7].item() == pytest.approx(0.3, rel=1e-4)  # a chain of up to 126 fp32 adds
    assert bool(torch.isnan(ref[c0 + 9]))
    assert torch.nonzero(torch.isnan(ref[:c0])).numel() == 0
    got = _Rows(x, cuda_device).run(keep)
    tmr.assert_same(got, ref, f"K={K} keep={keep}")
    assert int(tmr.bits(got)[c0 + 6]) == int(tmr.bits(torch.tensor([-0.0]))[0])


EXHAUSTIVE = [(K, "a9") for K in range(1, 7)] + [(8, "a5"), (9, "a4")]


@pytest.mark.parametrize("K,alphabet", EXHAUSTIVE, ids=[f"K{K}-{a}" for K, a in EXHAUSTIVE])
def test_exhaustive_small_columns(K, alphabet, cuda_device):
    """Every column of length K over the alphabet at every keep: K = 1..6 on
    the padded tier-8 kernel, K = 8 on the full one, K = 9 on the padded
    tier-16 kernel."""
    x = br.all_columns({"a9": br.ALPHABET9, "a5": br.ALPHABET5, "a4": br.ALPHABET4}[alphabet], K)
    rows = _Rows(x, cuda_device)
    for keep in range(1, K + 1):
        tmr.assert_same(rows.run(keep), br.nearmedian_mean_ref(x, keep), f"K={K} keep={keep}")


@pytest.mark.parametrize("K", [1, 5, 8, 33, 128])
def test_keep_all_is_the_trimmed_mean_at_trim_zero(K, cuda_device):
    x = tmr.make_rows(K, 300, torch.float32, seed=40 + K)
    if K >= 3:
        x[0, 60], x[1, 61], x[2, 62] = NAN, INF, -INF
        x[0, 63], x[1, 63] = INF, -INF
    rows = _Rows(x, cuda_device)
    got = rows.run(K)
    want = rows.out(300)
    dfn.trimmed_mean_rows(rows.ptrs, K, 300, 0, want)
    torch.cuda.synchronize(cuda_device)
    tmr.assert_same(got, want.cpu(), f"K={K}")
    tmr.assert_same(got, tmr.trimmed_mean_ref(x, 0), f"K={K} reference")


@pytest.mark.parametrize("K", [9, 48, 100])
def test_row_order_does_not_matter(K, cuda_device):
    x = tmr.make_rows(K, 300, torch.float32, seed=60 + K)
    x[0, 60], x[1, 61], x[2, 62] = NAN, INF, -INF
    rows = _Rows(x, cuda_device)
    g = torch.Generator().manual_seed(K)
    for keep in br.keeps(K):
        a = rows.run(keep)
        b = rows.run(keep, ptrs=rows.table(torch.randperm(K, generator=g).tolist()))
        tmr.assert_same(b, a, f"K={K} keep={keep}")


# ---- the defense end to end ---------------------------------------------------

K_E2E, F_E2E, BYZ = 11, 2, (3, 6)


def _model(g, centre=None) -> "OrderedDict[str, torch.Tensor]":
    r = lambda *s: 0.05 * torch.randn(*s, generator=g)
    d = OrderedDict([
        ("conv.weight", r(4, 3, 3, 3)), ("bn.weight", 1 + r(4)), ("bn.bias", r(4)),
        ("bn.running_mean", r(4)), ("bn.running_var", 1 + r(4).abs()),
        ("bn.num_batches_tracked", torch.tensor(100, dtype=torch.int64)), ("fc.weight", r(10, 36))])
    if centre is not None:
        d = OrderedDict((k, centre[k] + t if t.is_floating_point() else t) for k, t in d.items())
    return d


def _clients():
    """Nine honest clients 0.05 * randn around a common point, client 3 scaled
    x 100, client 6 with a NaN in a weight key."""
    g = torch.Generator().manual_seed(2024)
    centre = _model(g)
    raw = []
    for i in range(K_E2E):
        d = _model(g, centre)
        d["bn.num_batches_tracked"] = torch.tensor(100 + i, dtype=torch.int64)
        if i == BYZ[0]:
            d = OrderedDict((k, t * 100) for k, t in d.items())
        if i == BYZ[1]:
            d["fc.weight"][2, 5] = NAN
        raw.append((10 + i, d))
    return raw


@pytest.fixture(scope="module")
def e2e_reference():
    host = _clients()
    gaps = []
    ref, selected, scores, D = br.bulyan_ref(host, F_E2E)
    br.bulyan_select_ref(D, F_E2E, gaps)
    # every round's pick is far from going the other way: the kernel's
    # distances (relative error ~1e-7) cannot change the selection
    assert min(gaps) > 1e-4, gaps
    assert not set(selected) & set(BYZ) and len(selected) == K_E2E - 2 * F_E2E
    return host, ref, selected


def _check_result(out, host, ref, like):
    assert isinstance(out, OrderedDict)
    assert list(out.keys()) == list(host[0][1].keys())
    for k, t in out.items():
        assert t.dtype == torch.float32 and t.shape == host[0][1][k].shape, k
        assert t.device == like[k].device, k
        assert bool(torch.isfinite(t).all()), k
        tmr.assert_same(t.reshape(-1), ref[k].reshape(-1), k)


@pytest.mark.parametrize("device_inputs", [False, True], ids=["host", "device"])
def test_defense_end_to_end(device_inputs, e2e_reference, cuda_device):
    host, ref, selected = e2e_reference
    raw = host
    if device_inputs:
        raw = [(n, OrderedDict((k, t.to(cuda_device)) for k, t in d.items())) for n, d in host]
    ids = [{k: id(t) for k, t in d.items()} for _, d in raw]
    before = [{k: t.clone() for k, t in d.items()} for _, d in raw]
    out, info = dfn.bulyan(raw, F_E2E, cuda_device, method="exact", return_info=True)
    assert set(info.selected) == set(selected) and not set(info.selected) & set(BYZ)
    assert info.selected == selected  # the gaps assert the order too
    assert (info.theta, info.beta, info.method) == (7, 3, "exact") and len(info.scores) == 7
    assert all(out is not d for _, d in raw)
    _check_result(out, host, ref, raw[0][1])
    assert out["bn.num_batches_tracked"].dtype == torch.float32
    # no client dict is modified: the same tensors, the same values (NaN included)
    for (_, d), i, b in zip(raw, ids, before):
        assert list(d.keys()) == list(i)
        for k, t in d.items():
            assert id(t) == i[k] and torch.equal(tmr.bits(t.float()), tmr.bits(b[k].float())), k
    out2, info2 = dfn.bulyan(raw, F_E2E, cuda_device, method="auto", return_info=True)
    assert set(info2.selected) == set(selected)
    _check_result(out2, host, ref, raw[0][1])


class _Agg(MI355XServerAggregator):
    def __init__(self, args):
        super().__init__(torch.nn.Linear(1, 1), args)


class _Args:
    federated_optimizer = "FedAvg"
    enable_defense = True
    defense_type = "wise_bulyan"
    byzantine_client_num = F_E2E


def test_server_aggregator_routes_to_bulyan(e2e_reference, cuda_device):
    host, ref, _ = e2e_reference
    agg = _Agg(_Args())
    raw, idxs = agg.on_before_aggregation(host)
    assert raw is host and idxs == list(range(K_E2E))  # nothing happens before aggregation
    out = agg.on_after_aggregation(agg.aggregate(raw))
    _check_result(out, host, ref, host[0][1])


def test_torch_path_above_128_selected_clients(cuda_device):
    """K = 134, f = 2: theta = 130 rows, beta = 126.  With 130 rounds over
    i.i.d. clients some round's two lowest scores are bound to be close, so
    the pick ORDER is not pinned here; the selected SET is: the last four
    clients (two far away, two at three times the others' spread) score worse
    than any other client in every round, and the window does not depend on
    the order of the rows."""
    K, f, N = 134, 2, 300
    spread = [0.05] * 130 + [0.15, 0.15, 5.0, 5.0]
    g = torch.Generator().manual_seed(7)
    centre = torch.randn(N, generator=g)
    x = torch.stack([centre + spread[i] * torch.randn(N, generator=g) for i in range(K)])
    # NaN and infinities where the distances do not look: a BatchNorm statistic
    y = tmr.make_rows(K, 64, torch.float32, seed=8)
    y[5, 50], y[9, 51], y[11, 52] = NAN, INF, -INF
    y[20:26, 53] = NAN  # more than theta - beta of them: the window reaches a NaN
    host = [(1, OrderedDict([("w", x[i].clone()), ("bn.running_mean", y[i].clone())])) for i in range(K)]
    ref, selected, _, D = br.bulyan_ref(host, f)
    assert set(selected) == set(range(130)) and len(selected) == 130 > dfn.NEARMEDIAN_MAX_CLIENTS
    # the set survives distances moved by 1e-5 relative, a hundred times the
    # kernel's error (symmetric, as the kernel's matrix is)
    rng = np.random.default_rng(1)
    for _ in range(2):
        e = rng.uniform(-1e-5, 1e-5, size=D.shape)
        assert set(br.bulyan_select_ref(D * (1 + np.triu(e, 1) + np.triu(e, 1).T), f)[0]) == set(selected)
    assert bool(torch.isnan(ref["bn.running_mean"][53])) and not bool(torch.isnan(ref["bn.running_mean"][50]))
    raw = [(n, OrderedDict((k, t.to(cuda_device)) for k, t in d.items())) for n, d in host]
    out, info = dfn.bulyan(raw, f, method="exact", return_info=True)
    assert set(info.selected) == set(selected) and (info.theta, info.beta) == (130, 126)
    for k in ("w", "bn.running_mean"):
        assert out[k].is_cuda and out[k].dtype == torch.float32
        tmr.assert_same(out[k], ref[k], f"K={K} {k}")
