"""fedagg_pairgram2_wide_16 (csrc/pairgram_wide16.hip) and pairdist2_rows'
"gram_wide" on bf16 / f16 rows, 129 to 1024 clients, against the float64
distances of the exactly widened rows.

Bound: |D - D_ref| <= 2e-6 (|c_i|^2 + |c_j|^2) with c about the centre row that
was passed, the project's bound for both parent kernels (the fp32 wide Gram and
the narrow 16-bit Gram measured 4.3e-7 and 4.2e-7 against it).  Integer rows
whose c fits 8 bits: c = h, every fp32 accumulator is an exact integer, so D
equals the integer reference bit for bit at every chunk-group count.

Largest measured ratio on an MI355X (the tests print WIDE16_RATIO lines):
see DESIGN.md 5c.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import bulyan_ref as br
import chunk_groups as cg
from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn
from test_gpu_pair16 import DTYPES, RAGGED, _model, _ref, _rows
from test_gpu_pairgram_wide import SEGS_1200, _assert_matrix, _chunks, _cols, _group_cap, _scale, _tiles

pytestmark = pytest.mark.gpu

NAN = float("nan")
ALL_ON = {dt: {256: True, 512: True, 1024: True} for dt in DTYPES}


def _shifted(rows):
    """Row i of a 16-bit (K, L) device tensor, i mod 4 elements past a 256-byte
    boundary: every wave meets a row that is not 8-byte aligned (the element
    path).  -> (keep-alive, views, pointer table)"""
    K, L = rows.shape
    buf = torch.zeros((K, (L + 4 + 127) // 128 * 128), dtype=rows.dtype, device=rows.device)
    assert buf.data_ptr() % 256 == 0
    views = [buf[i, i % 4:i % 4 + L] for i in range(K)]
    for v, r in zip(views, rows):
        v.copy_(r)
    assert all(v.data_ptr() % 256 == 2 * (i % 4) for i, v in enumerate(views))
    return buf, views, kn.upload_i64([v.data_ptr() for v in views], rows.device)


def _np(t):
    return t.float().cpu().numpy()


def _abi(dt, ptrs, K, centre, d_chunks, n, dev, G=None):
    """The C entry with a NaN-filled workspace of work_len + 64 doubles; G: the
    chunk-group count forced through work_len (None: the default workspace)."""
    per = _tiles(K) * 4096
    wl = int(nat.lib().fedagg_robust_work_len(nat.WORK_PAIRGRAM_WIDE, K, n)) if G is None else per * G + K * K
    work = torch.full((wl + 64,), NAN, dtype=torch.float64, device=dev)
    out = torch.full((K, K), NAN, dtype=torch.float64, device=dev)
    nat.check(nat.lib().fedagg_pairgram2_wide_16(dfn._PAIR16_DT[dt], ptrs.data_ptr(), K, centre.data_ptr(),
                                                 d_chunks.data_ptr(), n, out.data_ptr(), work.data_ptr(), wl,
                                                 nat.stream_handle()), "wide16")
    return out.cpu().numpy(), work.cpu().numpy(), wl, per


def _check(D, want, scale, what):
    ratio = float((np.abs(D - want) / (scale + 1e-300)).max())
    print(f"WIDE16_RATIO {what} {ratio:.3e}")
    assert (np.abs(D - want) <= 2e-6 * scale + 1e-300).all(), (what, ratio)
    _assert_matrix(D, what)
    return float(np.abs(D - want).max())


def _against_float64(rows, segs, dev, what, aligned=False, forced_G=None):
    """"gram_wide" about the rounded client mean, through pairdist2_rows (and
    through the C entry at G = forced_G), against _ref's float64 distances."""
    K, L = rows.shape
    dt = rows.dtype
    if aligned:
        keep, views = rows, [rows[i] for i in range(K)]
        ptrs = kn.upload_i64([v.data_ptr() for v in views], dev)
    else:
        keep, views, ptrs = _shifted(rows)
    d_chunks, n = _chunks(segs, nat.PAIR_CHUNK, dev)
    centre = dfn.client_mean_row(ptrs, K, L, dev, aligned, dt)
    if aligned:  # the 8-byte path: every row, the centre and every stage start
        assert all(v.data_ptr() % 8 == 0 for v in views) and centre.data_ptr() % 8 == 0
        assert all(off % 8 == 0 for off, _ in segs) and nat.PAIR_CHUNK % 64 == 0
    if K < 1000:
        want = _ref(rows, segs)[0]
    else:  # _ref's loop takes 7 s here; the same float64 distances from the float64 Gram (1e-15 |x|^2: 1e-8 of the bound)
        X = rows.double().cpu().numpy()[:, _cols(segs)]
        n2 = (X * X).sum(axis=1)
        want = n2[:, None] + n2[None, :] - 2.0 * (X @ X.T)
    scale = _scale(_np(rows), _cols(segs), _np(centre))
    D = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", center=centre, dtype=dt).cpu().numpy()
    _check(D, want, scale, what)
    if forced_G:
        D, work, wl, _ = _abi(dt, ptrs, K, centre, d_chunks, n, dev, G=forced_G)
        _check(D, want, scale, f"{what} G={forced_G}")
        assert np.isnan(work[wl:]).all(), "written past work_len"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [129, 192, 193, 256, 1000])
def test_wide16_vs_float64(K, dt, cuda_device):
    """Last tiles of 1, 64 and 1 clients, an odd tile count, a near-full grid.
    K = 1000 also runs G = 2: a block streams more than four stages (a
    mid-stream fold)."""
    segs, L = (RAGGED, 5000) if K < 1000 else (SEGS_1200, 1300)
    _against_float64(_rows(K, L, cuda_device, 800 + K, dt), segs, cuda_device, f"{dt} K={K}",
                     forced_G=2 if K == 1000 else None)


@pytest.mark.parametrize("dt", DTYPES)
def test_wide16_aligned_8_byte_path(dt, cuda_device):
    _against_float64(_rows(256, 4096, cuda_device, 801, dt), [(0, 2048), (2056, 1000)], cuda_device,
                     f"{dt} K=256 aligned", aligned=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["close", "scattered", "one_outlier"])
def test_wide16_every_plane_count(kind, dt, cuda_device):
    """K = 193: mostly P = 1 for "close", P = 3 for "scattered"; the outlier
    (client 96, the second tile) lifts only that tile's pairs in its stage."""
    _against_float64(_rows(193, 5000, cuda_device, 900, dt, kind), RAGGED, cuda_device, f"{dt} {kind}")


def test_wide16_f16_two_planes(cuda_device):
    """f16 rows and centre in one binade, [2^-5, 2^-4): c is a multiple of 2^-15
    below 2^-5, at most 10 bits, and more than 8 wherever |c| >= 2^-7: every
    stage runs P = 2 (m != 0, l == 0, asserted here on the values)."""
    dev = cuda_device
    g = torch.Generator(device=dev).manual_seed(901)
    rows = 0.047 + 0.004 * torch.randn(5000, generator=g, device=dev) + 0.004 * torch.randn((193, 5000), generator=g,
                                                                                            device=dev)
    rows = rows.clamp(2.0 ** -5, 0.062).half()
    c = rows.float() - rows.double().mean(dim=0).half().float()
    m = c - c.bfloat16().float()
    assert bool((m != 0).any()) and bool((m == m.bfloat16().float()).all())
    _against_float64(rows, RAGGED, dev, "f16 P=2")


@pytest.fixture(scope="module")
def tiny_table(cuda_device):
    tab, cols = cg.tiny_chunk_table(nat.PAIR_CHUNK, 700, 0)
    return tab, cols, kn.upload_i64(tab.reshape(-1).tolist(), cuda_device), int(cols[-1]) + 4


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [65, 200])
def test_wide16_exact_on_small_integers(K, dt, tiny_table, cuda_device):
    """(i) rows in {-1, 0, 1} about a zero centre row; (ii) rows in [-8, 8]
    about an integer centre in [-4, 4]: |c| <= 12 fits 8 bits.  G = 1, 2, 3,
    the cap and the default workspace, which is NaN before every call."""
    dev = cuda_device
    tab, cols, d_chunks, L = tiny_table
    cap = _group_cap(K)
    for lo, hi, clo, chi in ((-1, 1, 0, 0), (-8, 8, -4, 4)):
        rows = cg.integer_rows(K, L, 300 + K, lo, hi)
        centre = cg.integer_rows(1, L, 7, clo, chi)[0]
        want = cg.int_pair(rows, cols)
        # a fold sums kSplitFold = 4 stages of 64 columns in fp32: exact below 2^24
        assert int(np.abs(rows - centre[None, :]).max()) ** 2 * 256 < 2 ** 24
        keep, views, ptrs = _shifted(torch.from_numpy(rows).to(dev).to(dt))
        d_centre = torch.from_numpy(centre).to(dev).to(dt)
        for G in (1, 2, 3, cap, None):
            what = f"wide16 exact {dt} K={K} G={G} rows [{lo}, {hi}]"
            D, work, wl, per = _abi(dt, ptrs, K, d_centre, d_chunks, len(tab), dev, G=G)
            G = cap if G is None else G
            assert np.array_equal(D.view(np.uint64), want.view(np.uint64)), (what, np.argwhere(D != want)[:8].tolist())
            assert wl == G * per + K * K
            assert not np.isnan(work[(G - 1) * per:G * per]).all(), f"{what}: the last group wrote nothing"
            assert not np.isnan(work[G * per:wl]).any(), f"{what}: the K x K matrix has unwritten entries"
            assert np.isnan(work[wl:]).all(), f"{what}: written past work_len"


@pytest.mark.parametrize("dt", DTYPES)
def test_wide16_centre_is_live_and_typed(dt, cuda_device):
    """K = 150 about the rounded mean, client 0's row and the zero row: each
    within the bound about its own centre.  The rows sit 0.05 from the origin
    and 0.01 from one another, so |c|^2 about zero is ~26 times |c|^2 about the
    mean (checked below on the reference, at least 20) and the error, which
    scales with it, must be at least 3 times larger: the argument is read."""
    dev = cuda_device
    K, L = 150, 5000
    rows = _rows(K, L, dev, 77, dt)
    keep, views, ptrs = _shifted(rows)
    d_chunks, n = _chunks(RAGGED, nat.PAIR_CHUNK, dev)
    cols, want = _cols(RAGGED), _ref(rows, RAGGED)[0]
    mean = dfn.client_mean_row(ptrs, K, L, dev, False, dt)
    errs, scales, Ds = {}, {}, {}
    for name, centre in (("mean", mean), ("client0", rows[0].clone()), ("zero", torch.zeros_like(mean))):
        Ds[name] = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", center=centre, dtype=dt).cpu().numpy()
        scales[name] = _scale(_np(rows), cols, _np(centre))
        errs[name] = _check(Ds[name], want, scales[name], f"{dt} centre {name}")
    assert np.median(scales["zero"] / scales["mean"]) > 20
    assert errs["zero"] >= 3 * errs["mean"], errs
    with pytest.raises(TypeError):
        dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", center=mean.float(), dtype=dt)
    D = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", length=L, dtype=dt).cpu().numpy()
    np.testing.assert_array_equal(D, Ds["mean"])


@pytest.mark.parametrize("dt", DTYPES)
def test_wide16_non_finite_input(dt, monkeypatch, cuda_device):
    dev = cuda_device
    K, L = 150, 5000
    rows = _rows(K, L, dev, 78, dt)
    rows[70, 1000], rows[70, 3000] = NAN, float("inf")
    keep, views, ptrs = _shifted(rows)
    d_chunks, n = _chunks(RAGGED, nat.PAIR_CHUNK, dev)
    Dw = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", length=L, dtype=dt).cpu().numpy()
    assert dfn.gram_condition(Dw) == float("inf") and not np.isfinite(Dw).all()
    monkeypatch.setattr(dfn, "PAIRGRAM_WIDE16_AUTO", ALL_ON)
    Da = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "auto", length=L, dtype=dt).cpu().numpy()
    np.testing.assert_array_equal(Da, dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "exact", dtype=dt).cpu().numpy())


@pytest.mark.parametrize("dt", DTYPES)
def test_wide16_defenses_end_to_end(dt, monkeypatch, cuda_device):
    """K = 140 clients of test_gpu_pair16's 16-bit model, 10 attackers scaled by
    3 as in test_krum_on_a_16bit_model: every method picks what the float64
    reference on the widened rows picks, and never an attacker.  Client i's
    update about the clients' mean is rescaled to an RMS of 0.01 sqrt(1 + 0.4 i)
    over the weight keys, so the scores are spaced by radius and not by
    chance.  A distance is within 2e-6 (|c_i|^2 + |c_j|^2) <= 2e-6 condition
    D_ij of the truth, so a score (a sum of distances) is within 2e-6 condition
    of its own: two scores further apart than twice that keep their order
    under every kernel, which the reference must show before it is relied on."""
    K, f = 140, 10
    bad = set(range(3, K, 14))
    assert len(bad) == f
    plain = [_model(dt, dt, 50 + i) for i in range(K)]
    wk = [k for k in plain[0] if dfn.is_weight_param(k)]
    cen = {k: torch.stack([d[k].double() for d in plain]).mean(dim=0) for k in wk}
    raw = []
    for i, d in enumerate(plain):
        u = {k: d[k].double() - cen[k] for k in wk}
        s = 0.01 * float(np.sqrt(1.0 + 0.4 * i)) / float(torch.cat([t.ravel() for t in u.values()]).pow(2).mean().sqrt())
        raw.append((10.0 + i, type(d)((k, ((cen[k] + s * u[k]) * (3.0 if i in bad else 1.0)).to(dt) if k in u else t)
                                      for k, t in d.items())))
    X = torch.stack([torch.cat([d[k].double().ravel() for k in wk]) for _, d in raw]).numpy()
    n2 = (X * X).sum(axis=1)
    D_ref = np.maximum(n2[:, None] + n2[None, :] - 2.0 * (X @ X.T), 0.0)
    np.fill_diagonal(D_ref, 0.0)
    ks = np.asarray(dfn.krum_scores(D_ref, f))
    order = torch.argsort(torch.Tensor(ks)).tolist()
    gaps = []
    selected, _ = br.bulyan_select_ref(D_ref, f, gaps)
    margin = 2 * 2e-6 * dfn.gram_condition(D_ref)
    assert min(gaps) > margin and (np.diff(ks[order[:4]]) / ks[order[:3]]).min() > margin, (min(gaps), margin)
    assert not set(order[:3]) & bad and not set(selected) & bad
    monkeypatch.setattr(dfn, "PAIRGRAM_WIDE16_AUTO", ALL_ON)
    for method in ("gram_wide", "auto", "exact"):
        for m in (1, 3):
            got = dfn.krum_before_aggregation(raw, f, m, device=cuda_device, method=method)
            assert [id(t) for t in got] == [id(raw[i]) for i in order[:m]], (method, m)
        out, info = dfn.bulyan(raw, f, cuda_device, method=method, return_info=True)
        assert info.selected == selected, method
        assert all(t.dtype == dt for k, t in out.items() if raw[0][1][k].dtype == dt)
    assert all(d[k].dtype == dt for _, d in raw for k in d if d[k].is_floating_point())
