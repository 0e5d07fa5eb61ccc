"""fedagg_pairgram2_wide_f32 (csrc/robust.hip) and pairdist2_rows' "gram_wide"
on the GPU: the split Gram by 64-client tile pairs, 129 to 1024 clients (and
below, beside the narrow kernel).

Bounds.  Against numpy the bound is test_pairgram2_vs_numpy's, taken over
because the error model is the same (one fp32 rounding of x - r, the split's
dropped terms, fp32 over at most four stages): |D - D_exact| <= 2e-6 (|c_i|^2
+ |c_j|^2) with c centred on the centre used (the column mean unless a test
says otherwise), and rtol 1e-5 on D for these rows.  Rows in {-1, 0, 1} with a
zero centre: c = x = h (m = l = 0), every fp32 accumulator over <= 256 columns
and every fp64 sum is an exact integer, so D equals the integer reference bit
for bit at every chunk-group count G.

Rows of one call start 0 .. 3 elements past a 256-byte boundary
(chunk_groups.shifted_rows), and explicit centre rows 1 element past one.

Largest measured ratio |D - D_exact| / (|c_i|^2 + |c_j|^2) on an MI355X:
1.7e-7 to 2.0e-7 for K = 129 .. 320, 3.7e-7 at K = 1000 and 4.3e-7 at K = 1024
(the tests print WIDE_RATIO lines), a fifth of the 2e-6 bound.  The module
takes about 7 s there.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pytest
import torch

import bulyan_ref as br
import chunk_groups as cg
from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEGS_5000 = [(0, 1), (3, 700), (704, 1), (960, 2500), (4000, 999)]  # test_gpu_dist_defenses.py's: ragged, partial stages
SEGS_1200 = [(0, 1), (3, 300), (304, 1), (400, 601), (1010, 289)]   # the same features in 1,192 columns


def _chunks(segs, chunk, dev):
    tab = []
    for off, n in segs:
        for s in range(off, off + n, chunk):
            tab += [s, min(chunk, off + n - s)]
    return kn.upload_i64(tab, dev), len(tab) // 2


def _cols(segs):
    return np.concatenate([np.arange(o, o + n) for o, n in segs])


def _np_pair(rows_np, segs):
    X = rows_np[:, _cols(segs)]
    K = X.shape[0]
    D = np.zeros((K, K))
    for i in range(K):
        d = (X[i][None, :] - X).astype(np.float32).astype(np.float64)
        D[i] = (d * d).sum(axis=1)
    return D


def _scale(rows_np, cols, centre=None):
    """|c_i|^2 + |c_j|^2 about `centre` (a row; default: the column mean)"""
    X = rows_np[:, cols].astype(np.float64)
    r = X.mean(axis=0) if centre is None else centre[cols].astype(np.float64)
    C = X - r[None, :]
    nrm = (C * C).sum(axis=1)
    return nrm[:, None] + nrm[None, :]


def _device_rows(rows_np, dev):
    """rows at mixed alignment in one call -> (keep-alive, pointer table)"""
    buf, views = cg.shifted_rows(rows_np, [i % 4 for i in range(len(rows_np))], dev)
    return (buf, views), kn.upload_i64([v.data_ptr() for v in views], dev)


def _device_centre(row_np, dev):
    """a centre row 4 bytes past a 256-byte boundary: not 16-byte aligned"""
    buf, (v,) = cg.shifted_rows(row_np[None, :], [1], dev)
    assert v.data_ptr() % 16 == 4
    return buf, v


def _tiles(K):
    return cg.pair_tiles(K)


def _group_cap(K):
    return -(-4096 // (2 * _tiles(K)))


def _wide_abi(ptrs, K, centre, d_chunks, n, dev, G=None):
    """The C entry point with a NaN-filled workspace of work_len + 64 doubles;
    G: the chunk-group count forced through work_len (None: the default
    workspace).  -> (D, workspace on the host, work_len, per-group doubles)"""
    per = _tiles(K) * 4096
    wl = int(nat.lib().fedagg_robust_work_len(nat.WORK_PAIRGRAM_WIDE, K, n)) if G is None else per * G + K * K
    work = torch.full((wl + 64,), NAN, dtype=torch.float64, device=dev)
    out = torch.full((K, K), NAN, dtype=torch.float64, device=dev)
    nat.check(nat.lib().fedagg_pairgram2_wide_f32(ptrs.data_ptr(), K, centre.data_ptr(), d_chunks.data_ptr(), n,
                                                  out.data_ptr(), work.data_ptr(), wl, nat.stream_handle()), "wide")
    return out.cpu().numpy(), work.cpu().numpy(), wl, per


def _assert_matrix(D, what):
    assert (np.diag(D) == 0).all() and (D >= 0).all(), what
    np.testing.assert_array_equal(D, D.T, err_msg=what)


# ---- against numpy ----------------------------------------------------------------

@pytest.mark.parametrize("K", [129, 130, 191, 192, 193, 256, 320, 1000, 1024])
def test_gram_wide_vs_numpy(K, cuda_device):
    """A last tile of 1, 2, 63 and 64 clients, an empty and a one-client fourth
    tile, an odd tile count, and the full 16 x 16 tile grid.  Through
    pairdist2_rows: the centre is the client mean the FedAvg kernel computes.
    K >= 1000 also runs G = 2, where a block streams 4 or 5 chunks (more than
    four stages, a mid-stream fold)."""
    dev = cuda_device
    segs, L = (SEGS_5000, 5000) if K < 1000 else (SEGS_1200, 1300)
    rows = cg.gaussian_rows(K, L, 100 + K, outliers=[0])
    keep, ptrs = _device_rows(rows, dev)
    d_chunks, n = _chunks(segs, nat.PAIR_CHUNK, dev)
    want = _np_pair(rows, segs)
    scale = _scale(rows, _cols(segs))
    Ds = [dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", length=L).cpu().numpy()]
    if K >= 1000:
        centre = dfn.client_mean_row(ptrs, K, L, dev)
        Ds.append(_wide_abi(ptrs, K, centre, d_chunks, n, dev, G=2)[0])
    worst = 0.0
    for D in Ds:
        worst = max(worst, float((np.abs(D - want) / scale).max()))
        print(f"WIDE_RATIO K={K} {worst:.3e}")
        assert (np.abs(D - want) <= 2e-6 * scale + 1e-300).all(), (K, worst)
        np.testing.assert_allclose(D, want, rtol=1e-5)
        _assert_matrix(D, f"K={K}")


def test_gram_wide_empty_chunk_table(cuda_device):
    rows = cg.gaussian_rows(130, 64, 1)
    keep, ptrs = _device_rows(rows, cuda_device)
    empty = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    D = dfn.pairdist2_rows(ptrs, 130, empty, 0, cuda_device, "gram_wide", length=64)
    assert D.shape == (130, 130) and bool((D == 0).all())


# ---- bit-exact on {-1, 0, 1} at forced chunk-group counts --------------------------

EXACT_CHUNKS = 700   # at least K = 65's largest group count (683)


@pytest.fixture(scope="module")
def tiny_table(cuda_device):
    tab, cols = cg.tiny_chunk_table(nat.PAIR_CHUNK, EXACT_CHUNKS, 0)
    assert len(cols) <= cg.MAX_TABLE_COLUMNS
    return tab, cols, kn.upload_i64(tab.reshape(-1).tolist(), cuda_device), int(cols[-1]) + 4


@pytest.mark.parametrize("K", [65, 200])
def test_gram_wide_exact_on_small_integers(K, tiny_table, cuda_device):
    """K = 65: a two-tile grid whose second tile holds one client; K = 200:
    four tiles, the last of 8 clients.  G = 1 streams the whole table through
    one block per tile pair; the largest G gives most blocks one tiny chunk.
    The workspace is NaN before the call: D finite and exact shows every
    partial slot that is read was written, the last group's slots show that G
    groups ran, and the 64 doubles past work_len are still NaN."""
    dev = cuda_device
    tab, cols, d_chunks, L = tiny_table
    rows = cg.integer_rows(K, L, 300 + K, -1, 1)
    keep, ptrs = _device_rows(rows, dev)
    zbuf, zero = _device_centre(np.zeros(L, np.float32), dev)
    want = cg.int_pair(rows, cols)
    cap = _group_cap(K)
    assert cap <= EXACT_CHUNKS
    for G in (1, 2, 3, cap):
        what = f"gram_wide exact K={K} G={G}"
        D, work, wl, per = _wide_abi(ptrs, K, zero, d_chunks, len(tab), dev, G=G)
        assert np.array_equal(D.view(np.uint64), want.view(np.uint64)), (what, np.argwhere(D != want)[:8].tolist())
        assert wl == G * per + K * K
        assert not np.isnan(work[(G - 1) * per:G * per]).all(), f"{what}: group {G - 1} wrote nothing"
        assert not np.isnan(work[G * per:wl]).any(), f"{what}: the K x K matrix has unwritten entries"
        assert np.isnan(work[wl:]).all(), f"{what}: written past work_len"
    # the default workspace runs the largest G
    D, work, wl, per = _wide_abi(ptrs, K, zero, d_chunks, len(tab), dev)
    assert wl == cap * per + K * K and np.array_equal(D.view(np.uint64), want.view(np.uint64))
    assert np.isnan(work[wl:]).all()


# ---- the centre argument -----------------------------------------------------------

def test_centre_invariance(cuda_device):
    """K = 150, centre = the client mean, client 0's row and the zero row: D is
    translation invariant, so each is within the bound about ITS centre.  These
    rows sit 0.05 from the origin and 0.01 from one another, so |c|^2 about 0 is
    26 times |c|^2 about the mean and the zero centre's error must show it (at
    least 3 x here): the argument is live."""
    dev = cuda_device
    K, L = 150, 5000
    rows = cg.gaussian_rows(K, L, 77)
    keep, ptrs = _device_rows(rows, dev)
    d_chunks, n = _chunks(SEGS_5000, nat.PAIR_CHUNK, dev)
    cols = _cols(SEGS_5000)
    want = _np_pair(rows, SEGS_5000)
    mean = rows.astype(np.float64).mean(axis=0).astype(np.float32)
    errs = {}
    for name, centre in (("mean", mean), ("client0", rows[0].copy()), ("zero", np.zeros(L, np.float32))):
        cbuf, d_centre = _device_centre(centre, dev)
        D = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", center=d_centre).cpu().numpy()
        scale = _scale(rows, cols, centre)
        err = np.abs(D - want)
        print(f"WIDE_CENTRE {name} ratio {float((err / np.maximum(scale, 1e-300)).max()):.3e} abs {err.max():.3e}")
        assert (err <= 2e-6 * scale + 1e-300).all(), name
        _assert_matrix(D, name)
        errs[name] = float(err.max())
    assert errs["zero"] > 3 * errs["mean"], errs
    # no centre given: the mean of the rows' first `length` columns
    D = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", length=L).cpu().numpy()
    assert (np.abs(D - want) <= 2e-6 * _scale(rows, cols) + 1e-300).all()


@pytest.mark.parametrize("K", [100, 128])
def test_gram_wide_beside_the_narrow_kernel(K, cuda_device):
    """Both Grams within their bound of the exact distances, so within the sum
    of the two bounds of each other."""
    dev = cuda_device
    rows = cg.gaussian_rows(K, 5000, 500 + K, outliers=[0])
    keep, ptrs = _device_rows(rows, dev)
    d_chunks, n = _chunks(SEGS_5000, nat.PAIR_CHUNK, dev)
    Dw = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", length=5000).cpu().numpy()
    Dg = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram").cpu().numpy()
    scale = _scale(rows, _cols(SEGS_5000))
    assert (np.abs(Dw - Dg) <= 2 * 2e-6 * scale + 1e-300).all(), float((np.abs(Dw - Dg) / scale).max())
    _assert_matrix(Dw, f"K={K}")


# ---- "auto" ------------------------------------------------------------------------

ALL_ON = {256: True, 512: True, 1024: True}


def test_auto_runs_the_wide_gram_in_a_winning_tier(monkeypatch, cuda_device):
    dev = cuda_device
    K, L = 150, 5000
    rows = cg.gaussian_rows(K, L, 78)
    keep, ptrs = _device_rows(rows, dev)
    d_chunks, n = _chunks(SEGS_5000, nat.PAIR_CHUNK, dev)
    De = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "exact").cpu().numpy()
    Dw = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", length=L).cpu().numpy()
    assert not np.array_equal(De, Dw)
    assert dfn.gram_condition(Dw) < dfn.GRAM_MAX_CONDITION
    monkeypatch.setattr(dfn, "PAIRGRAM_WIDE_AUTO", ALL_ON)
    np.testing.assert_array_equal(dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "auto", length=L).cpu().numpy(), Dw)
    # without a length or a centre "auto" has nothing to centre on: the exact kernel
    np.testing.assert_array_equal(dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "auto").cpu().numpy(), De)
    monkeypatch.setattr(dfn, "PAIRGRAM_WIDE_AUTO", {256: False, 512: False, 1024: False})
    np.testing.assert_array_equal(dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "auto", length=L).cpu().numpy(), De)


@pytest.mark.parametrize("bad", ["inf", "nan", "1e30"])
def test_auto_falls_back_for_a_non_finite_or_far_client(bad, monkeypatch, cuda_device):
    """K = 140 with an inf element, a NaN element or a client scaled by 1e30
    (fp32 squares overflow): the wide Gram passes the non-finite values on,
    gram_condition is inf, and "auto" in a tier that is on returns the exact
    kernel's distances bit for bit."""
    dev = cuda_device
    K, L = 140, 3000
    rows = cg.gaussian_rows(K, L, 11)
    if bad == "inf":
        rows[5, 123] = np.inf
    elif bad == "nan":
        rows[70, 77] = np.nan
    else:
        rows[133] *= np.float32(1e30)
    keep, ptrs = _device_rows(rows, dev)
    d_chunks, n = _chunks([(0, L)], nat.PAIR_CHUNK, dev)
    Dw = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "gram_wide", length=L).cpu().numpy()
    De = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "exact").cpu().numpy()
    assert dfn.gram_condition(Dw) == float("inf")
    assert not np.isfinite(Dw).all()
    monkeypatch.setattr(dfn, "PAIRGRAM_WIDE_AUTO", ALL_ON)
    Da = dfn.pairdist2_rows(ptrs, K, d_chunks, n, dev, "auto", length=L).cpu().numpy()
    np.testing.assert_array_equal(Da, De)


# ---- the defenses end to end -------------------------------------------------------

K_E2E, F_E2E, M_E2E = 140, 10, 5


def _model(g, fc=1000):
    r = lambda *s: 0.05 * torch.randn(*s, generator=g)  # noqa: E731
    return OrderedDict([
        ("conv.weight", r(4, 3, 3, 3)), ("bn.weight", r(4)), ("bn.bias", r(4)),
        ("bn.running_mean", r(4)), ("bn.running_var", 1 + r(4).abs()),
        ("bn.num_batches_tracked", torch.tensor(100, dtype=torch.int64)), ("fc.weight", r(10, fc))])


def _clients():
    """test_gpu_bulyan.py's model around a common point; client i's update is
    scaled to an RMS of exactly 0.05 sqrt(1 + 0.1 i) over the weight keys, so
    every round's scores are spaced by the clients' radii and not by chance."""
    g = torch.Generator().manual_seed(1)
    centre = _model(g)
    raw = []
    for i in range(K_E2E):
        d = _model(g)
        w = torch.cat([t.reshape(-1) for k, t in d.items() if br.is_weight_key(k)])
        s = float(np.sqrt(1.0 + 0.1 * i)) * 0.05 / float(w.double().pow(2).mean().sqrt())
        raw.append((10 + i, OrderedDict((k, centre[k] + s * t if t.is_floating_point() else t)
                                        for k, t in d.items())))
    return raw


@pytest.fixture(scope="module")
def e2e_reference():
    """The selections on the CPU and their margins: the two lowest scores of
    every Bulyan round, and neighbouring Krum scores among the lowest M + 1,
    are more than 1e-4 apart relative (measured when this was written: 3.8e-4
    and 1.0e-2), a thousand times the Gram's error for these well-conditioned
    rows, so every kernel must select the same clients in the same order."""
    host = _clients()
    _, selected, _, D = br.bulyan_ref(host, F_E2E)
    gaps = []
    br.bulyan_select_ref(D, F_E2E, gaps)
    assert min(gaps) > 1e-4, min(gaps)
    ks = np.asarray(dfn.krum_scores_loop(D, F_E2E))
    order = np.argsort(ks, kind="stable")
    low = ks[order[:M_E2E + 1]]
    assert (np.diff(low) / low[:-1]).min() > 1e-4
    return host, selected, order[:M_E2E].tolist()


@pytest.mark.parametrize("device_inputs", [False, True], ids=["host", "device"])
def test_defenses_select_what_the_exact_kernel_selects(device_inputs, e2e_reference, cuda_device):
    host, selected, krum_order = e2e_reference
    raw = host
    if device_inputs:
        raw = [(n, OrderedDict((k, t.to(cuda_device)) for k, t in d.items())) for n, d in host]
    outs = {}
    for method in ("exact", "gram_wide"):
        out, info = dfn.bulyan(raw, F_E2E, cuda_device, method=method, return_info=True)
        assert info.selected == selected and info.method == method
        assert (info.theta, info.beta) == (K_E2E - 2 * F_E2E, K_E2E - 4 * F_E2E)
        outs[method] = out
        got = dfn.krum_before_aggregation(raw, F_E2E, M_E2E, cuda_device, method=method)
        assert [next(i for i, item in enumerate(raw) if item is s) for s in got] == krum_order, method
    for k, t in outs["exact"].items():  # the same rows selected: the same stage 2, bit for bit
        assert torch.equal(t.view(torch.int32), outs["gram_wide"][k].view(torch.int32)), k
