"""Krum's pair distances from bf16 / f16 rows (csrc/robust16.hip) against the
float64 distances of the exactly widened rows."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
RAGGED = [(0, 1), (3, 700), (704, 1), (960, 2500), (4000, 999)]  # odd starts, partial stages, the element path


def _rows(K, L, dev, seed, dtype, kind="close"):
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.randn(L, generator=g, device=dev) * 0.05
    rows = base + 0.01 * torch.randn((K, L), generator=g, device=dev)
    if kind == "scattered":  # no common exponent: c = x - r needs all three planes
        rows = rows * torch.exp2(torch.randint(-12, 13, (K, L), generator=g, device=dev).float())
    rows = rows.to(dtype)
    if kind == "one_outlier":  # one element, in the second 64-column stage of a fold of four
        rows[K // 2, 960 + 70] = (rows[K // 2, 960 + 70].float() * 300.0).to(dtype)
    return rows


def _run(rows, segs, method):
    K, dev = rows.shape[0], rows.device
    tab = [v for off, n in segs for s in range(off, off + n, nat.PAIR_CHUNK)
           for v in (s, min(nat.PAIR_CHUNK, off + n - s))]
    chunks = kn.upload_i64(tab, dev)
    ptrs = kn.upload_i64([rows[i].data_ptr() for i in range(K)], dev)
    return dfn.pairdist2_rows(ptrs, K, chunks, len(tab) // 2, dev, method, dtype=rows.dtype).cpu().numpy()


def _ref(rows, segs):
    """D_ref (float64 differences), D_ref16 (fp32-rounded differences) and
    scale = |C_i|^2 + |C_j|^2 about the centre mean_fp64(x).to(dtype)."""
    cols = np.concatenate([np.arange(o, o + n) for o, n in segs])
    X = rows.cpu().double().numpy()[:, cols]
    D, D16 = np.zeros((len(X), len(X))), np.zeros((len(X), len(X)))
    for i in range(len(X)):
        d = X[i][None, :] - X
        d32 = d.astype(np.float32).astype(np.float64)
        D[i], D16[i] = (d * d).sum(axis=1), (d32 * d32).sum(axis=1)
    cen = torch.from_numpy(X.mean(axis=0)).to(rows.dtype).double().numpy()
    nrm = ((X - cen) ** 2).sum(axis=1)
    return D, D16, nrm[:, None] + nrm[None, :]


def _check_gram(rows, segs):
    D = _run(rows, segs, "gram")
    want, _, scale = _ref(rows, segs)
    ratio = float((np.abs(D - want) / (scale + 1e-300)).max())
    print(f"gram16 {rows.dtype} K={rows.shape[0]}: max |D - D_ref| / scale = {ratio:.3e}")
    assert (np.abs(D - want) <= 2e-6 * scale + 1e-300).all(), ratio
    assert (np.diag(D) == 0).all() and (D >= 0).all()
    np.testing.assert_array_equal(D, D.T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 33, 64, 65, 100, 113, 128])
def test_gram16_vs_float64(K, dtype, cuda_device):
    _check_gram(_rows(K, 5000, cuda_device, 300 + K, dtype), RAGGED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["close", "scattered", "one_outlier"])
@pytest.mark.parametrize("K", [17, 128])
def test_gram16_every_plane_count(K, kind, dtype, cuda_device):
    _check_gram(_rows(K, 5000, cuda_device, 400 + K, dtype, kind), RAGGED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("segs", [[(0, 4096)], [(8, 1000)]])
@pytest.mark.parametrize("K", [16, 128])
def test_gram16_aligned_vector_path(K, segs, dtype, cuda_device):
    rows = _rows(K, 4096, cuda_device, 500 + K, dtype)  # rows 8192 bytes apart: 16-byte aligned
    assert all(rows[i].data_ptr() % 16 == 0 for i in range(K))
    _check_gram(rows, segs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 2, 3, 63, 64, 65, 128, 129, 200])
def test_exact16_vs_float64(K, dtype, cuda_device):
    rows = _rows(K, 5000, cuda_device, 600 + K, dtype)
    D = _run(rows, RAGGED, "exact")
    np.testing.assert_allclose(D, _ref(rows, RAGGED)[1], rtol=1e-5)
    assert (np.diag(D) == 0).all()
    np.testing.assert_array_equal(D, D.T)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_element_reaches_the_result(bad, cuda_device):
    K = 24
    rows = _rows(K, 5000, cuda_device, 700, torch.bfloat16)
    rows[5, 1000] = bad
    D = _run(rows, RAGGED, "gram")
    off = np.arange(K) != 5
    assert not np.isfinite(D[5, off]).any() and not np.isfinite(D[off, 5]).any()
    assert dfn.gram_condition(D) == float("inf")
    np.testing.assert_array_equal(_run(rows, RAGGED, "auto"), _run(rows, RAGGED, "exact"))


def _model(dtype, lin_dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    base = torch.Generator().manual_seed(1)
    b = lambda *s: torch.randn(*s, generator=base) * 0.05
    d = OrderedDict()
    d["conv.weight"] = ((b(6, 3, 3, 3) + 0.01 * r(6, 3, 3, 3)) * scale).to(dtype)
    d["bn.weight"] = ((b(6) + 0.01 * r(6)) * scale).to(dtype)
    d["bn.bias"] = ((b(6) + 0.01 * r(6)) * scale).to(dtype)
    d["bn.running_mean"] = r(6).to(dtype)
    d["bn.running_var"] = r(6).abs().to(dtype)
    d["bn.num_batches_tracked"] = torch.tensor(7)
    d["fc.weight"] = ((b(10, 54) + 0.01 * r(10, 54)) * scale).to(lin_dtype)
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 3])
def test_krum_on_a_16bit_model(m, dtype, cuda_device):
    K, f, bad = 20, 3, (2, 9, 15)
    raw = [(10.0 + i, _model(dtype, dtype, 50 + i, 3.0 if i in bad else 1.0)) for i in range(K)]
    X = torch.stack([torch.cat([d[k].double().ravel() for k in d if dfn.is_weight_param(k)]) for _, d in raw]).numpy()
    D_ref = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    order = torch.argsort(torch.Tensor(dfn.krum_scores(D_ref, f))).tolist()[:m]
    for method in ("auto", "gram", "exact"):
        got = dfn.krum_before_aggregation(raw, f, m, device=cuda_device, method=method)
        assert [id(t) for t in got] == [id(raw[i]) for i in order]
    assert not set(order) & set(bad)


def test_krum_on_a_mixed_width_model(cuda_device):
    K, f = 20, 3
    mixed = [(1.0, _model(torch.bfloat16, torch.float32, 50 + i, 3.0 if i in (2, 9, 15) else 1.0)) for i in range(K)]
    wide = [(n, OrderedDict((k, v.float() if v.is_floating_point() else v) for k, v in d.items())) for n, d in mixed]
    got = dfn.krum_before_aggregation(mixed, f, 3, device=cuda_device)
    want = dfn.krum_before_aggregation(wide, f, 3, device=cuda_device)
    assert [[id(x) for x in mixed].index(id(t)) for t in got] == [[id(x) for x in wide].index(id(t)) for t in want]
