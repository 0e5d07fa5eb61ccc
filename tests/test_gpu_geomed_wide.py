"""GPU checks of the fused Weiszfeld step for 129 to 1024 clients
(fedagg_wsum_dist2_wide_f32 / _16, csrc/geomed_wide.hip) and of
geometric_median(method="fused_wide").

Kernel: at each tier's first, padded and full K, z bit for bit against the
numpy chain and fedagg_wsum_f32 on the (widened) rows, guards untouched; D
within 1e-12 relative of numpy's fp64 sum over the kernel's own z (exact
squares, only the fp64 summation order differs: at most N 2^-53 = 3.3e-13 for
this table's N = 2,974 columns, and twice that between two kernels' orders),
bit-identical from call to call.  End to end: test_gpu_geomed16.py's
tolerances, for the same arithmetic.
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
from test_gpu_geomed16 import DTS, GUARD, bits, client_rows, clients, ordered, place, widened

pytestmark = pytest.mark.gpu

NAMES = ["f32", "bf16", "f16"]
KS = [129, 200, 256, 257, 512, 513, 700, 1024]
NUMELS = [1, 63, 64, 65, 127, 129, 1025, 1500]  # 1025 and 1500: a whole chunk, then partial groups


def dtype_of(name):
    return torch.float32 if name == "f32" else DTS[name][0]


@pytest.fixture(scope="module")
def table(cuda_device):
    """Weight keys of NUMELS with gaps of 1 .. 3 columns (even and odd starts)."""
    offsets, off = [], 2
    for j, n in enumerate(NUMELS):
        offsets.append(off)
        off += n + 1 + j % 3
    g = types.SimpleNamespace(keys=[f"l{j}.weight" for j in range(len(NUMELS))], offsets=offsets, numels=NUMELS,
                              length=off)
    chunks, n_chunks = dfn.weight_chunks(g, nat.DIST_CHUNK, cuda_device)
    cols = np.concatenate([np.arange(o, o + n) for o, n in zip(offsets, NUMELS)])
    starts = chunks.cpu().numpy().reshape(-1, 2)[:, 0]
    assert (starts % 2 == 0).any() and (starts % 2 == 1).any()
    return g, chunks, n_chunks, cols


def rows_of(name, K, L):
    """-> (rows in their dtype, their exact fp32 widening, fp32 weights): test_gpu_geomed16.py's rows (a -0
    column, subnormals, one large value: f16's largest, and 65,280 in bf16, so that no single column decides a
    distance and D checks the whole sum); fp32 rows keep the bf16 specials (a bf16 subnormal is an fp32 one)
    among full-width mantissas."""
    dt = DTS["bf16" if name == "f32" else name][0]
    raw, wide, w32 = client_rows(K, L, dt, 0x7BFF if name == "f16" else 0x477F, K)
    if name != "f32":
        return raw.view(dt), wide, w32
    full = (0.05 * np.random.default_rng(K).standard_normal((K, L))).astype(np.float32)
    full[:, 5:12] = wide[:, 5:12]
    return torch.from_numpy(full), full, w32


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_chain_and_the_two_pass_path(name, K, table, cuda_device):
    dev, dt = cuda_device, dtype_of(name)
    g, chunks, n_chunks, cols = table
    rows, wide, w32 = rows_of(name, K, g.length)
    outside = np.setdiff1d(np.arange(g.length), cols)
    zr = ref.chain(wide, w32)
    Dr = ref.dist2(wide, zr, cols)
    assert np.isfinite(zr).all() and np.isfinite(Dr).all()
    d_w = torch.from_numpy(w32).to(dev)
    keep32, p32 = place(torch.from_numpy(wide), 0, dev)
    z32 = torch.zeros(g.length, dtype=torch.float32, device=dev)
    D32 = dfn.weiszfeld_step_unfused(p32, d_w, K, g.length, chunks, n_chunks, z32, dev).cpu().numpy()
    z32 = z32.cpu().numpy()  # fedagg_wsum_f32 on the widened rows
    for shift, zshift in ((0, 0), (0, 1), (1, 0), (1, 1)):
        keep, ptrs = place(rows, shift, dev)
        zbuf = torch.full((g.length + 64,), GUARD, dtype=torch.float32, device=dev)
        zv = zbuf[zshift:zshift + g.length]
        # the wrapper uploads kernel-argument weights (they hold up to 256)
        w = kn.HostWeights([float(v) for v in w32]) if shift and K <= kn.INLINE_MAX_K else d_w
        D1 = dfn.wsum_dist2_rows_wide(ptrs, w, K, chunks, n_chunks, zv, dev, dtype=dt).cpu().numpy()
        D2 = dfn.wsum_dist2_rows_wide(ptrs, w, K, chunks, n_chunks, zv, dev, dtype=dt).cpu().numpy()
        zb = zbuf.cpu().numpy()
        z = zb[zshift:zshift + g.length]
        what = f"{name} K={K} shift={shift} zshift={zshift}"
        assert np.array_equal(bits(z[cols]), bits(zr[cols])), what
        assert np.array_equal(bits(z[cols]), bits(z32[cols])), what
        assert bits(z[5:6])[0] == 0x80000000, what
        assert (z[outside] == GUARD).all() and (zb[:zshift] == GUARD).all() and \
            (zb[zshift + g.length:] == GUARD).all(), what
        print(what, "max rel D error", float(np.max(np.abs(D1 - Dr) / Dr)), "against the pair",
              float(np.max(np.abs(D1 - D32) / D32)))
        np.testing.assert_allclose(D1, Dr, rtol=1e-12, atol=0, err_msg=what)  # z is zr, bit for bit
        assert np.array_equal(D1.view(np.uint64), D2.view(np.uint64)), what
        np.testing.assert_allclose(D1, D32, rtol=1e-12, atol=0, err_msg=what)


@pytest.mark.parametrize("name,case", [(n, c) for n in NAMES for c in ("empty", "k1025", "short_work", "host_w")] +
                         [("bf16", "dtype"), ("f16", "dtype")])
def test_abi_edges(name, case, cuda_device):
    dev = cuda_device
    K = 1025 if case == "k1025" else 130
    keep, ptrs = place(torch.ones((K, 256), dtype=dtype_of(name)), 0, dev)
    w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
    z = torch.full((256,), GUARD, dtype=torch.float32, device=dev)
    D = torch.full((K,), 7.0, dtype=torch.float64, device=dev)
    work = torch.zeros(K, dtype=torch.float64, device=dev)
    tab = kn.upload_i64([0, 256], dev)
    a = (ptrs.data_ptr(), w.data_ptr(), K, tab.data_ptr(), 0 if case == "empty" else 1, z.data_ptr(), D.data_ptr(),
         work.data_ptr(), K - 1 if case == "short_work" else K, nat.FEDAGG_HOST_WEIGHTS if case == "host_w" else 0,
         nat.stream_handle())
    if name == "f32":
        rc = nat.lib().fedagg_wsum_dist2_wide_f32(*a)
    else:
        rc = nat.lib().fedagg_wsum_dist2_wide_16(nat.DT_F32 if case == "dtype" else DTS[name][1], *a)
    assert rc == (0 if case == "empty" else -2 if case == "k1025" else -1)  # FEDAGG_OK, _ENOKERNEL, _EINVAL
    assert (z == GUARD).all()
    assert D.cpu().tolist() == [0.0 if case == "empty" else 7.0] * K


@pytest.mark.parametrize("K", [129, 130, 300])  # 129: the screen leaves 128, and the narrow kernel takes over
@pytest.mark.parametrize("name", NAMES)
def test_defense_fused_wide(name, K, cuda_device, caplog):
    dt = dtype_of(name)
    raw = clients(K, dt, cuda_device)
    wide = widened(raw)
    total = sum(n for n, _ in raw)
    a32 = np.array([n / total for n, _ in raw], dtype=np.float64).astype(np.float32)
    out, info = dfn.geometric_median(raw, maxiter=0, method="fused_wide", return_info=True)
    assert list(out.keys()) == list(raw[0][1].keys()) and info.method == "fused_wide"
    for k, t in out.items():  # maxiter = 0 is FedAvg: the fp32 chain rounded once
        want = torch.from_numpy(ref.chain(np.stack([d[k].float().cpu().numpy().reshape(-1) for _, d in raw]), a32))
        want = want if k.endswith("num_batches_tracked") else want.to(dt)
        assert t.dtype == want.dtype and torch.equal(t.cpu().reshape(-1).view(torch.uint8), want.view(torch.uint8)), k
    out, info = dfn.geometric_median(raw, ftol=0.0, method="fused_wide", return_info=True)
    out32, info32 = dfn.geometric_median(wide, ftol=0.0, method="unfused", return_info=True)
    assert info.method == "fused_wide" and info.iterations == info32.iterations == 16
    np.testing.assert_allclose(info.weights, info32.weights, rtol=1e-6, atol=0)
    for k, t in out.items():
        if name != "f32" and t.dtype == dt:
            assert np.abs(ordered(t) - ordered(out32[k].to(dt))).max() <= 1, k
    # a client poisoned with inf is dropped: the result is the run without it
    bad = [(n, OrderedDict(d)) for n, d in raw]
    bad[2][1]["fc.bias"] = torch.full((17,), float("inf"), dtype=dt, device=cuda_device)
    out, info = dfn.geometric_median(bad, maxiter=3, ftol=0.0, method="fused_wide", return_info=True)
    outr, infor = dfn.geometric_median(raw[:2] + raw[3:], maxiter=3, ftol=0.0, method="fused_wide", return_info=True)
    assert info.dropped == [2] and "[2]" in caplog.text and info.weights[2] == 0.0
    assert np.array_equal(np.delete(info.weights, 2), infor.weights)
    for k in out:
        assert torch.equal(out[k], outr[k]), k
    with pytest.raises(ValueError):
        dfn.geometric_median(raw * 8, method="fused_wide")  # more than 1024 clients


@pytest.mark.parametrize("K", [130, 300])
@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_16_bit_model_allocates_less_than_a_widened_copy(name, K, cuda_device):
    """Peak above the clients' own tensors.  An fp32 bucket of this model is 768 bytes a client on its own (rows
    padded to 64 elements); the 16-bit rows take 384, the integer counter 16."""
    raw = clients(K, DTS[name][0], cuda_device)
    floats = sum(t.numel() for t in raw[0][1].values() if t.is_floating_point())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dfn.geometric_median(raw, ftol=0.0, method="fused_wide")
    peak = torch.cuda.max_memory_allocated() - before
    print(f"{name} K={K}: {peak} bytes above the clients at the call's peak, an fp32 copy of them is {K * floats * 4}")
    assert peak < K * floats * 4
