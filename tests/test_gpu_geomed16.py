"""GPU checks of the 16-bit fused Weiszfeld step (fedagg_wsum_dist2_16,
csrc/geomed16.hip) and of the "geomed" defense on bf16 / f16 models.

Kernel: z bit for bit against the numpy chain on the exactly widened rows and
against fedagg_wsum_dist2_f32 on the widened copy, at every K tier edge, in the
dword form (aligned rows, even starts) and the element form (odd starts, rows
misaligned by one element), columns outside the table and guards untouched.
D within 1e-12 relative of numpy's fp64 sum over the kernel's own z: exact
squares, only the fp64 summation order differs, at most N 2^-53 = 8.6e-13 for
the N = 7,748 table columns of this layout; bit-identical from call to call.
End to end: the iterate is fp32 in both runs, so the 16-bit run and the run on
clients widened by the test differ only through that summation order (weights
within 1e-6, as test_gpu_geomed.py derives), and a rounded output element by
at most one ulp of the model's dtype.
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

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128]
NUMELS = [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4099]
GUARD = 123.5
DTS = {"bf16": (torch.bfloat16, nat.DT_BF16, 0x7F7F), "f16": (torch.float16, nat.DT_F16, 0x7BFF)}  # largest finite


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def table(cuda_device):
    """test_gpu_geomed.py's row: weight keys of NUMELS with gaps of 1 .. 3
    columns (even and odd starts) and a BatchNorm buffer the table leaves out."""
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
    g = types.SimpleNamespace(keys=keys, offsets=offsets, numels=numels, length=off)
    chunks, n_chunks = dfn.weight_chunks(g, nat.DIST_CHUNK, cuda_device)
    cols = np.concatenate([np.arange(o, o + n) for k, o, n in zip(keys, offsets, numels) if dfn.is_weight_param(k)])
    starts = chunks.cpu().numpy().reshape(-1, 2)[:, 0]
    assert (starts % 2 == 0).any() and (starts % 2 == 1).any()
    return g, chunks, n_chunks, cols


def client_rows(K, L, dt, big, seed):
    """-> (raw 16-bit rows as int16, their exact fp32 widening, fp32 weights)"""
    rng = np.random.default_rng(seed)
    raw = torch.from_numpy((0.05 * rng.standard_normal((K, L))).astype(np.float32)).to(dt).view(torch.int16)
    raw[:, 5] = -0x8000                                         # a column of -0
    raw[0, 6:9] = torch.tensor([0, -0x8000, 0], dtype=torch.int16)
    raw[K - 1, 9:11] = torch.tensor([1, -0x7FFF], dtype=torch.int16)  # +- the smallest subnormal
    raw[0, 11] = big
    w = rng.random(K) + 0.1
    return raw, raw.view(dt).float().numpy(), (w / w.sum()).astype(np.float32)


def place(rows, shift, dev):
    """Rows 256 bytes apart, starting `shift` elements past a 256-byte boundary."""
    K, L = rows.shape
    buf = torch.zeros((K, (L + 255) // 128 * 128), dtype=rows.dtype, device=dev)
    buf[:, shift:shift + L] = rows.to(dev)
    return buf, kn.upload_i64([buf[i, shift:].data_ptr() for i in range(K)], dev)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTS)
def test_kernel_matches_the_chain_and_the_fp32_kernel(name, K, table, cuda_device):
    dt, _, big = DTS[name]
    dev = cuda_device
    g, chunks, n_chunks, cols = table
    raw, wide, w32 = client_rows(K, g.length, dt, big, K)
    outside = np.setdiff1d(np.arange(g.length), cols)
    zr = ref.chain(wide, w32)
    assert np.isfinite(zr).all() and np.isfinite(ref.dist2(wide, zr, cols)).all()
    keep32, p32 = place(torch.from_numpy(wide), 0, dev)
    z32 = torch.zeros(g.length, dtype=torch.float32, device=dev)
    dfn.wsum_dist2_rows(p32, torch.from_numpy(w32).to(dev), K, chunks, n_chunks, z32, dev)
    z32 = z32.cpu().numpy()
    for shift, zshift, host_w in ((0, 0, False), (0, 1, True), (1, 0, True), (1, 1, False)):
        keep, ptrs = place(raw.view(dt), shift, dev)
        zbuf = torch.full((g.length + 64,), GUARD, dtype=torch.float32, device=dev)
        zv = zbuf[zshift:zshift + g.length]
        d_w = kn.HostWeights([float(v) for v in w32]) if host_w else torch.from_numpy(w32).to(dev)
        D1 = dfn.wsum_dist2_rows(ptrs, d_w, K, chunks, n_chunks, zv, dev, dtype=dt).cpu().numpy()
        D2 = dfn.wsum_dist2_rows(ptrs, d_w, K, chunks, n_chunks, zv, dev, dtype=dt).cpu().numpy()
        zb = zbuf.cpu().numpy()
        z = zb[zshift:zshift + g.length]
        what = f"{name} K={K} shift={shift} zshift={zshift} host_w={host_w}"
        assert np.array_equal(bits(z[cols]), bits(zr[cols])), what    # the numpy chain
        assert np.array_equal(bits(z[cols]), bits(z32[cols])), what   # fedagg_wsum_dist2_f32 on the widened copy
        assert bits(z[5:6])[0] == 0x80000000, what
        assert (z[outside] == GUARD).all() and (zb[:zshift] == GUARD).all() and \
            (zb[zshift + g.length:] == GUARD).all(), what
        Dr = ref.dist2(wide, z, cols)
        print(what, "max rel D error", float(np.max(np.abs(D1 - Dr) / np.maximum(Dr, 1e-300))))
        np.testing.assert_allclose(D1, Dr, rtol=1e-12, atol=0, err_msg=what)
        assert np.array_equal(D1.view(np.uint64), D2.view(np.uint64)), what


@pytest.mark.parametrize("case", ["empty", "k129", "f32", "short_work"])
@pytest.mark.parametrize("name", DTS)
def test_abi_edges(name, case, cuda_device):
    dt, code, _ = DTS[name]
    dev = cuda_device
    K = 129 if case == "k129" else 4
    keep, ptrs = place(torch.ones((K, 256), dtype=dt), 0, dev)
    w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
    z = torch.full((256,), GUARD, dtype=torch.float32, device=dev)
    D = torch.full((K,), 7.0, dtype=torch.float64, device=dev)
    work = torch.zeros(K, dtype=torch.float64, device=dev)
    tab = kn.upload_i64([0, 256], dev)
    rc = nat.lib().fedagg_wsum_dist2_16(nat.DT_F32 if case == "f32" else code, ptrs.data_ptr(), w.data_ptr(), K,
                                        tab.data_ptr(), 0 if case == "empty" else 1, z.data_ptr(), D.data_ptr(),
                                        work.data_ptr(), K - 1 if case == "short_work" else K, 0, nat.stream_handle())
    assert rc == {"empty": 0, "k129": -2, "f32": -1, "short_work": -1}[case]  # FEDAGG_OK, _ENOKERNEL, _EINVAL
    assert (z == GUARD).all()
    assert D.cpu().tolist() == [0.0 if case == "empty" else 7.0] * K


# ---- geometric_median end to end ---------------------------------------------------

def clients(K, dt, dev):
    """A small model of two weight keys (odd numels), a BatchNorm running_mean
    in the 16-bit dtype and an int64 counter; honest rows around a common
    point, client 1 far away; unequal sample counts that sum to a power of two
    (n_i / sum n is then exact, with or without a dropped client)."""
    rng = np.random.default_rng(7 * K)
    shapes = [("fc.weight", (11, 13)), ("fc.bias", (17,)), ("bn.running_mean", (5,))]
    base = {k: rng.standard_normal(s) for k, s in shapes}
    counts = [64 + (37 * i) % 64 for i in range(K)]
    counts[0] += (1 << int(np.ceil(np.log2(sum(counts))))) - sum(counts)
    raw = []
    for i in range(K):
        d = OrderedDict((k, torch.from_numpy((100.0 * (i == 1) + base[k] + 0.05 * rng.standard_normal(s))
                                             .astype(np.float32)).to(dt).to(dev)) for k, s in shapes)
        d["bn.num_batches_tracked"] = torch.tensor(100 + 7 * i, dtype=torch.int64, device=dev)
        raw.append((counts[i], d))
    return raw


def widened(raw):
    return [(n, OrderedDict((k, t.float() if t.is_floating_point() else t) for k, t in d.items())) for n, d in raw]


def ordered(t):
    """16-bit patterns as integers whose order is the values' order."""
    b = t.contiguous().view(torch.int16).cpu().numpy().astype(np.int64).reshape(-1)
    return np.where(b >= 0, b, -(b & 0x7FFF))


@pytest.mark.parametrize("K", [5, 128, 130])
@pytest.mark.parametrize("name", DTS)
def test_defense_on_16_bit_models(name, K, cuda_device, caplog):
    dt = DTS[name][0]
    raw = clients(K, dt, cuda_device)
    total = sum(n for n, _ in raw)
    a32 = np.array([n / total for n, _ in raw], dtype=np.float64).astype(np.float32)
    methods = ("auto",) if K > dfn.GEOMED_MAX_CLIENTS else ("fused", "unfused", "auto")
    for method in methods:  # maxiter = 0 is FedAvg: the fp32 chain rounded once
        out, info = dfn.geometric_median(raw, maxiter=0, method=method, return_info=True)
        assert list(out.keys()) == list(raw[0][1].keys())
        for k, t in out.items():
            stack = np.stack([d[k].float().cpu().numpy().reshape(-1) for _, d in raw])
            want = torch.from_numpy(ref.chain(stack, a32))
            if k.endswith("num_batches_tracked"):
                assert t.dtype == torch.float32 and np.array_equal(bits(t.cpu().numpy()), bits(want.numpy())), k
            else:
                assert t.dtype == dt and t.shape == raw[0][1][k].shape
                assert torch.equal(t.cpu().view(torch.int16).reshape(-1), want.to(dt).view(torch.int16)), (method, k)
    if K > dfn.GEOMED_MAX_CLIENTS:
        out, info = dfn.geometric_median(raw, return_info=True)
        assert info.method == "unfused" and info.weights[1] < 1e-3
    else:
        out, info = dfn.geometric_median(raw, ftol=0.0, method="fused", return_info=True)
        out32, info32 = dfn.geometric_median(widened(raw), ftol=0.0, method="fused", return_info=True)
        assert info.method == "fused" and info.iterations == info32.iterations == 16
        np.testing.assert_allclose(info.weights, info32.weights, rtol=1e-6, atol=0)
        for k, t in out.items():
            if t.dtype == dt:
                assert np.abs(ordered(t) - ordered(out32[k].to(dt))).max() <= 1, k
    # a client poisoned with inf is dropped: the result is the run without it
    bad = [(n, OrderedDict(d)) for n, d in raw]
    bad[2][1]["fc.bias"] = torch.full((17,), float("inf"), dtype=dt, device=cuda_device)
    method = "auto" if K > dfn.GEOMED_MAX_CLIENTS else "fused"
    out, info = dfn.geometric_median(bad, maxiter=3, ftol=0.0, method=method, return_info=True)
    rest = raw[:2] + raw[3:]
    outr, infor = dfn.geometric_median(rest, maxiter=3, ftol=0.0, method=method, return_info=True)
    assert info.dropped == [2] and "[2]" in caplog.text and info.weights[2] == 0.0
    assert np.array_equal(np.delete(info.weights, 2), infor.weights)
    for k in out:
        assert torch.equal(out[k], outr[k]), k
    with pytest.raises(NotImplementedError):  # host dicts of a 16-bit model stay refused
        dfn.geometric_median([(n, OrderedDict((k, t.cpu()) for k, t in d.items())) for n, d in raw[:2]])
