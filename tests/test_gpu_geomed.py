"""GPU checks of the fused Weiszfeld step (fedagg_wsum_dist2_f32,
csrc/geomed.hip) and of the "geomed" defense built on it.

Kernel: z bit for bit against fedagg_wsum_f32 and the numpy chain, columns
outside the chunk table untouched, D within 1e-12 relative of numpy's fp64 sum
over the kernel's own z (fedagg_dist2_f32's tolerance: exact squares, only the
fp64 summation order differs, N 2^-53 for N <= 7,300 columns) and bit-identical
from call to call.  End to end: the fused and the unfused path differ only
through that summation order, which moves a weight a_i / sqrt(D_i) by about
5e-13 relative per pass; the fp32 weight it rounds to can flip its last bit
and the contraction does not amplify it, so final weights agree within 1e-6
(16 fp32 ulp) with each other and with the CPU reference.
"""
from __future__ import annotations

import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

import geomed_ref as ref
from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn
from fedml_amd.server_aggregator import MI355XServerAggregator

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128]
NUMELS = [1, 63, 64, 65, 1023, 1024, 1025, 4099]
GUARD = 123.5


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def key_layout():
    """A row of weight keys with the numels above, gaps of 1 .. 3 columns
    between them (starts of every alignment) and a BatchNorm buffer in the
    middle that the chunk table leaves out."""
    keys, offsets, numels, off = [], [], [], 2
    for j, n in enumerate(NUMELS):
        keys.append(f"l{j}.weight")
        offsets.append(off)
        numels.append(n)
        off += n + 1 + j % 3
        if j == 3:
            keys.append("bn.running_mean")
            offsets.append(off)
            numels.append(7)
            off += 7
    return types.SimpleNamespace(keys=keys, offsets=offsets, numels=numels, length=off)


@pytest.fixture(scope="module")
def table(cuda_device):
    g = key_layout()
    chunks, n_chunks = dfn.weight_chunks(g, nat.DIST_CHUNK, cuda_device)
    cols = np.concatenate([np.arange(o, o + n) for k, o, n in zip(g.keys, g.offsets, g.numels)
                           if dfn.is_weight_param(k)])
    tab = chunks.cpu().numpy().reshape(-1, 2)
    assert n_chunks == len(tab) and tab[:, 1].max() == 1024 and tab[:, 1].min() >= 1
    assert np.array_equal(np.concatenate([np.arange(s, s + n) for s, n in tab]), cols)
    return g, chunks, n_chunks, cols


def client_rows(K, L, seed):
    rng = np.random.default_rng(seed)
    rows = (0.05 * rng.standard_normal((K, L))).astype(np.float32)
    rows[:, 5] = -0.0          # a column of -0: the chain must return -0
    rows[0, 6:9] = [0.0, -0.0, 1e-42]
    rows[K - 1, 9:11] = [-1e-45, 3e-39]  # denormals
    w = rng.random(K) + 0.1
    return rows, (w / w.sum()).astype(np.float32)


def run_fused(rows_np, w32, chunks, n_chunks, dev, shift=0, host_w=False):
    """-> (z with guards (numpy), D (numpy), D of a second call): rows and z
    start `shift` elements past a 256-byte boundary."""
    K, L = rows_np.shape
    buf = torch.zeros((K, (L + 127) // 64 * 64), dtype=torch.float32, device=dev)  # rows 256 bytes apart
    buf[:, shift:shift + L] = torch.from_numpy(rows_np).to(dev)
    ptrs = kn.upload_i64([buf[i, shift:].data_ptr() for i in range(K)], dev)
    zbuf = torch.full((L + 64,), GUARD, dtype=torch.float32, device=dev)
    z = zbuf[shift:shift + L]
    d_w = kn.HostWeights([float(v) for v in w32]) if host_w else torch.from_numpy(np.asarray(w32)).to(dev)
    D1 = dfn.wsum_dist2_rows(ptrs, d_w, K, chunks, n_chunks, z, dev).cpu().numpy()
    D2 = dfn.wsum_dist2_rows(ptrs, d_w, K, chunks, n_chunks, z, dev).cpu().numpy()
    zz = torch.empty(L + 64, dtype=torch.float32, device=dev)  # fedagg_wsum_f32 on the same inputs
    kn.wsum_ptrs(torch.float32, ptrs, d_w, K, L, zz[shift:shift + L], shift == 0)
    return zbuf.cpu().numpy(), D1, D2, zz[shift:shift + L].cpu().numpy()


@pytest.mark.parametrize("K", KS)
def test_kernel_matches_wsum_and_numpy(K, table, cuda_device):
    g, chunks, n_chunks, cols = table
    rows, w32 = client_rows(K, g.length, K)
    outside = np.setdiff1d(np.arange(g.length), cols)
    zr = ref.chain(rows, w32)
    for shift, host_w in ((0, False), (1, False), (0, True), (1, True)):
        zbuf, D1, D2, zw = run_fused(rows, w32, chunks, n_chunks, cuda_device, shift, host_w)
        z = zbuf[shift:shift + g.length]
        what = f"K={K} shift={shift} host_w={host_w}"
        assert np.array_equal(bits(z[cols]), bits(zw[cols])), what   # fedagg_wsum_f32
        assert np.array_equal(bits(z[cols]), bits(zr[cols])), what   # the numpy chain
        assert bits(z[5:6])[0] == 0x80000000, what
        assert (z[outside] == GUARD).all() and (zbuf[:shift] == GUARD).all() and \
            (zbuf[shift + g.length:] == GUARD).all(), what
        Dr = ref.dist2(rows, z, cols)
        np.testing.assert_allclose(D1, Dr, rtol=1e-12, atol=0, err_msg=what)
        assert np.array_equal(D1.view(np.uint64), D2.view(np.uint64)), what


@pytest.mark.parametrize("K", [3, 16, 100, 128])
def test_kernel_matches_the_unfused_pair(K, table, cuda_device):
    g, chunks, n_chunks, cols = table
    dev = cuda_device
    rows, w32 = client_rows(K, g.length, 100 + K)
    t = torch.zeros((K, (g.length + 127) // 64 * 64), dtype=torch.float32, device=dev)  # 16-byte aligned rows
    t[:, :g.length] = torch.from_numpy(rows).to(dev)
    ptrs = kn.upload_i64([t[i].data_ptr() for i in range(K)], dev)
    d_w = torch.from_numpy(w32).to(dev)
    z1 = torch.zeros(g.length + 64, dtype=torch.float32, device=dev)
    z2 = torch.zeros_like(z1)
    D1 = dfn.wsum_dist2_rows(ptrs, d_w, K, chunks, n_chunks, z1, dev)
    D2 = dfn.weiszfeld_step_unfused(ptrs, d_w, K, g.length, chunks, n_chunks, z2, dev, aligned=True)
    assert np.array_equal(bits(z1.cpu().numpy()[cols]), bits(z2.cpu().numpy()[cols]))
    np.testing.assert_allclose(D1.cpu().numpy(), D2.cpu().numpy(), rtol=1e-12, atol=0)
    # and the specification in torch ops, on the device
    z3, D3 = dfn.weiszfeld_step_torch(t[:, :g.length], w32.tolist(), torch.from_numpy(cols).to(dev))
    assert np.array_equal(bits(z3.cpu().numpy()[cols]), bits(z1.cpu().numpy()[cols]))
    np.testing.assert_allclose(D3.cpu().numpy(), D1.cpu().numpy(), rtol=1e-12, atol=0)


def test_empty_table_and_kernel_limit(table, cuda_device):
    dev = cuda_device
    rows, w32 = client_rows(4, 256, 1)
    t = torch.from_numpy(rows).to(dev)
    ptrs = kn.upload_i64([t[i].data_ptr() for i in range(4)], dev)
    z = torch.full((256,), GUARD, dtype=torch.float32, device=dev)
    empty = torch.zeros(2, dtype=torch.int64, device=dev)
    D = dfn.wsum_dist2_rows(ptrs, torch.from_numpy(w32).to(dev), 4, empty, 0, z, dev)
    assert D.cpu().tolist() == [0.0] * 4 and (z == GUARD).all()
    with pytest.raises(nat.FedAggNativeError):  # fedagg_robust_work_len: no fused kernel above 128 clients
        dfn.wsum_dist2_rows(ptrs, torch.from_numpy(w32).to(dev), 129, empty, 1, z, dev)


@pytest.mark.parametrize("K", [9, 128])
def test_non_finite_clients_give_non_finite_distances(K, table, cuda_device):
    g, chunks, n_chunks, cols = table
    rows, w32 = client_rows(K, g.length, 7)
    rows[1, cols[40]] = np.nan
    rows[K - 1, cols[-1]] = np.inf
    zbuf, D1, D2, zw = run_fused(rows, w32, chunks, n_chunks, cuda_device)
    z = zbuf[:g.length]
    assert np.isnan(z[cols[40]]) and np.isinf(z[cols[-1]])
    assert not np.isfinite(D1).any()  # every client is a NaN or an inf away from such a z
    ok = np.ones(g.length, dtype=bool)
    ok[[cols[40], cols[-1]]] = False
    assert np.array_equal(bits(z[cols][ok[cols]]), bits(zw[cols][ok[cols]]))
    # a client that is only huge: finite distances
    rows, w32 = client_rows(K, g.length, 8)
    rows[0, cols] = 1e30
    zbuf, D1, D2, zw = run_fused(rows, w32, chunks, n_chunks, cuda_device)
    assert np.isfinite(D1).all()
    np.testing.assert_allclose(D1, ref.dist2(rows, zbuf[:g.length], cols), rtol=1e-12, atol=0)


# ---- geometric_median end to end -------------------------------------------------

SPLIT = [("fc.weight", (40, 100)), ("fc.bias", (99,))]  # 4099 columns


def as_dicts(rows, counts, dev=None, extra=None):
    raw = []
    for i, (r, n) in enumerate(zip(rows, counts)):
        d, o = OrderedDict(), 0
        for k, shp in SPLIT:
            m = int(np.prod(shp))
            t = torch.from_numpy(r[o:o + m].copy()).view(shp)
            d[k] = t.to(dev) if dev is not None else t
            o += m
        if extra is not None:
            for k, t in extra(i).items():
                d[k] = t.to(dev) if dev is not None else t
        raw.append((n, d))
    return raw


def flat(d):
    return np.concatenate([d[k].detach().cpu().numpy().reshape(-1) for k, _ in SPLIT])


@pytest.fixture(scope="module")
def reference():
    """The CPU reference of every robustness case, computed once: maxiter 16
    and the fixed maxiter 6 of the path comparison."""
    out = {}
    for K, bad in ref.ROBUST_CASES:
        rows, counts, corrupted = ref.robust_clients(K, bad)
        total = 0
        for n in counts:
            total += n
        a = [n / total for n in counts]
        out[(K, bad)] = (rows, counts, corrupted, a, ref.loop(rows, a, 1e-6, 16, 0.0), ref.loop(rows, a, 1e-6, 6, 0.0))
    return out


@pytest.mark.parametrize("case", ref.ROBUST_CASES)
def test_fused_and_unfused_agree_with_each_other_and_the_reference(case, reference, cuda_device):
    rows, counts, corrupted, a, _, (zr, wr, fr) = reference[case]
    raw = as_dicts(rows, counts, cuda_device)
    before = [flat(d) for _, d in raw]
    res = {}
    for method in ("fused", "unfused"):
        out, info = dfn.geometric_median(raw, nu=1e-6, maxiter=6, ftol=0.0, method=method, return_info=True)
        assert info.method == method and info.iterations == 6 and info.dropped == []
        assert list(out.keys()) == [k for k, _ in SPLIT] and all(t.is_cuda for t in out.values())
        res[method] = (flat(out), info)
        np.testing.assert_allclose(info.weights, wr, rtol=1e-6, atol=0, err_msg=method)
        np.testing.assert_allclose(info.objective, fr, rtol=1e-9, atol=0, err_msg=method)
        # the result IS fedagg_wsum_f32 with the returned weights
        t = torch.from_numpy(rows).to(cuda_device)
        L = rows.shape[1]
        buf = torch.zeros((len(rows), (L + 127) // 64 * 64), dtype=torch.float32, device=cuda_device)
        buf[:, :L] = t
        ptrs = kn.upload_i64([buf[i].data_ptr() for i in range(len(rows))], cuda_device)
        zz = torch.empty(L + 64, dtype=torch.float32, device=cuda_device)
        w32 = [float(np.float32(v)) for v in info.weights]
        kn.wsum_ptrs(torch.float32, ptrs, kn.weights_for(w32, torch.float32, cuda_device), len(rows), L, zz, True)
        assert np.array_equal(bits(res[method][0]), bits(zz[:L].cpu().numpy())), method
    np.testing.assert_allclose(res["fused"][1].weights, res["unfused"][1].weights, rtol=1e-6, atol=0)
    for b, (_, d) in zip(before, raw):
        assert np.array_equal(bits(b), bits(flat(d)))  # no client dict is modified


@pytest.mark.parametrize("method", ["fused", "unfused"])
@pytest.mark.parametrize("case", ref.ROBUST_CASES)
def test_robust_on_the_device(case, method, reference, cuda_device):
    rows, counts, corrupted, a, (zr, wr, fr), _ = reference[case]
    out, info = dfn.geometric_median(as_dicts(rows, counts, cuda_device), nu=1e-6, maxiter=16, ftol=0.0,
                                     method=method, return_info=True)
    got = ref.robust_check(flat(out), info.weights, rows, corrupted)
    print(case, method, got)
    assert got["ratio"] < 1.0
    assert got["corrupted_weight"] < 1e-4
    f = info.objective
    assert all(f[t + 1] <= f[t] * (1 + 1e-6) for t in range(len(f) - 1))
    np.testing.assert_allclose(info.weights, wr, rtol=1e-6, atol=0)


def bn_extra(i):
    rng = np.random.default_rng(50 + i)
    return OrderedDict([("bn.weight", torch.from_numpy(rng.standard_normal(5).astype(np.float32))),
                        ("bn.running_mean", torch.from_numpy(rng.standard_normal(5).astype(np.float32))),
                        ("bn.running_var", torch.from_numpy(rng.random(5).astype(np.float32))),
                        ("bn.num_batches_tracked", torch.tensor(100 + 7 * i, dtype=torch.int64))])


@pytest.mark.parametrize("method", ["fused", "unfused"])
def test_batchnorm_buffers_take_the_final_weights(method, reference, cuda_device):
    rows, counts, corrupted, a, _, _ = reference[(9, 2)]
    raw = as_dicts(rows, counts, cuda_device, bn_extra)
    out, info = dfn.geometric_median(raw, maxiter=5, ftol=0.0, method=method, return_info=True)
    assert list(out.keys()) == list(raw[0][1].keys())
    w32 = np.asarray(info.weights).astype(np.float32)
    for k in ("bn.weight", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"):
        stack = np.stack([d[k].cpu().numpy().astype(np.float32).reshape(-1) for _, d in raw])  # integers as fl32(v)
        assert out[k].dtype == torch.float32 and out[k].shape == raw[0][1][k].shape
        assert np.array_equal(bits(out[k].cpu().numpy().reshape(-1)), bits(ref.chain(stack, w32))), k
    assert np.array_equal(bits(flat(out)), bits(ref.chain(rows, w32)))
    # the distances ran over the weight keys only: bn.weight counts, the buffers do not
    plain = dfn.geometric_median(as_dicts(rows, counts, cuda_device, lambda i: OrderedDict(
        [("bn.weight", bn_extra(i)["bn.weight"])])), maxiter=5, ftol=0.0, method=method, return_info=True)[1]
    np.testing.assert_allclose(plain.weights, info.weights, rtol=1e-6, atol=0)  # another chunking, another sum order


def test_host_clients_get_host_tensors_back(reference, cuda_device):
    rows, counts, _, _, _, _ = reference[(9, 2)]
    host = dfn.geometric_median(as_dicts(rows, counts), maxiter=4, ftol=0.0, device=cuda_device, method="fused")
    devr = dfn.geometric_median(as_dicts(rows, counts, cuda_device), maxiter=4, ftol=0.0, method="fused")
    assert all(not t.is_cuda for t in host.values()) and all(t.is_cuda for t in devr.values())
    assert np.array_equal(bits(flat(host)), bits(flat(devr)))


def test_more_clients_than_the_kernel_holds_take_the_pair(cuda_device):
    rng = np.random.default_rng(130)
    K, N = 130, 4099
    rows = (rng.standard_normal(N) + 0.05 * rng.standard_normal((K, N))).astype(np.float32)
    rows[3] = (1e4 * rng.standard_normal(N)).astype(np.float32)
    counts = [int(v) for v in rng.integers(50, 150, K)]
    out, info = dfn.geometric_median(as_dicts(rows, counts, cuda_device), maxiter=6, ftol=0.0, return_info=True)
    assert info.method == "unfused"
    total = sum(counts)
    zr, wr, fr = ref.loop(rows, [n / total for n in counts], 1e-6, 6, 0.0)
    np.testing.assert_allclose(info.weights, wr, rtol=1e-6, atol=0)
    assert info.weights[3] < 1e-4
    with pytest.raises(ValueError):
        dfn.geometric_median(as_dicts(rows, counts, cuda_device), method="fused")


def test_auto_follows_the_measured_table(reference, cuda_device):
    for case in ((9, 2), (128, 40)):
        rows, counts, _, _, _, _ = reference[case]
        info = dfn.geometric_median(as_dicts(rows, counts, cuda_device), maxiter=1, return_info=True)[1]
        assert info.method == ("fused" if dfn.geomed_auto_fused(case[0]) else "unfused")


class _Agg(MI355XServerAggregator):
    def __init__(self, args):
        super().__init__(torch.nn.Linear(1, 1), args)


def test_plugin_path_gives_the_same_result(reference, cuda_device):
    rows, counts, _, _, _, _ = reference[(16, 5)]
    args = types.SimpleNamespace(federated_optimizer="FedAvg", enable_defense=True, defense_type="geomed",
                                 geomed_maxiter=7, geomed_ftol=0.0, geomed_nu=1e-5)
    agg = _Agg(args)
    raw = as_dicts(rows, counts, cuda_device)
    lst, idxs = agg.on_before_aggregation(raw)
    assert lst is raw and idxs == list(range(16))
    got = agg.on_after_aggregation(agg.aggregate(lst))
    want = dfn.geometric_median(raw, nu=1e-5, maxiter=7, ftol=0.0)
    assert list(got.keys()) == list(want.keys())
    assert np.array_equal(bits(flat(got)), bits(flat(want)))
    # the defaults: nu 1e-6, maxiter 16, ftol 1e-6
    agg2 = _Agg(types.SimpleNamespace(federated_optimizer="FedAvg", enable_defense=True, defense_type="geomed"))
    assert np.array_equal(bits(flat(agg2.aggregate(raw))), bits(flat(dfn.geometric_median(raw))))


@pytest.mark.parametrize("method", ["fused", "unfused"])
def test_screening_on_the_device(method, reference, cuda_device, caplog):
    rows, counts, _, _, _, _ = reference[(9, 2)]
    rows = ref.robust_clients(9, 0)[0].copy()
    rows[2, 17] = np.nan
    rows[5, 100] = np.inf
    rows[7, :] = 3e38
    out, info = dfn.geometric_median(as_dicts(rows, counts, cuda_device), maxiter=6, ftol=0.0, method=method,
                                     return_info=True)
    assert info.dropped == [2, 5, 7] == ref.screen(rows)
    assert "[2, 5, 7]" in caplog.text
    alive = [0, 1, 3, 4, 6, 8]
    kept = 0.0
    total = sum(counts)
    for i in alive:
        kept += counts[i] / total
    zr, wr, fr = ref.loop(rows[alive], [counts[i] / total / kept for i in alive], 1e-6, 6, 0.0)
    np.testing.assert_allclose(info.weights[alive], wr, rtol=1e-6, atol=0)
    assert info.weights[[2, 5, 7]].tolist() == [0.0] * 3
    z = flat(out)
    assert np.isfinite(z).all()
    assert np.array_equal(bits(z), bits(ref.chain(rows[alive], info.weights[alive].astype(np.float32))))
    # half of the weight: the breakdown point
    four = rows[[0, 2, 1, 5]]
    with pytest.raises(ValueError, match="half"):
        dfn.geometric_median(as_dicts(four, [10, 10, 10, 10], cuda_device), method=method)
    # a NaN in a BatchNorm buffer is not screened: it passes through into that key only
    good = ref.robust_clients(9, 0)[0]

    def extra(i):
        e = bn_extra(i)
        if i == 4:
            e["bn.running_mean"] = torch.full((5,), float("nan"))
        return e
    out, info = dfn.geometric_median(as_dicts(good, counts, cuda_device, extra), maxiter=3, ftol=0.0, method=method,
                                     return_info=True)
    assert info.dropped == [] and torch.isnan(out["bn.running_mean"]).all()
    assert np.isfinite(flat(out)).all() and torch.isfinite(out["bn.running_var"]).all()
