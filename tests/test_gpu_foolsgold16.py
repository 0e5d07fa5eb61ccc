"""fedagg_histgram_16 (csrc/histgram16.hip) against the fp64 reference on the
exactly widened rows, and the "foolsgold_cos" rule on bf16 / f16 models end to
end, on the device.  The chunk table, the models and the rounds are
test_gpu_foolsgold.py's.

Measured on an MI355X: the largest HISTGRAM16_RATIO over the cases of
test_gram_and_history and test_all_rows_aligned is 1.09e-7 (bf16, K = 113,
with a history; the bound, 1e-6, is not tightened to it).
"""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import test_gpu_foolsgold as tgf
from chunk_groups import gaussian_rows, integer_rows
from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn

pytestmark = pytest.mark.gpu

L, TABLE, COLS = tgf.L, tgf.TABLE, tgf.COLS
DTS = [torch.bfloat16, torch.float16]
DT = {torch.bfloat16: nat.DT_BF16, torch.float16: nat.DT_F16}


def _place(rows, shifts, dev, fill=0.0):
    """(buffer, views): row i of the (K, L) tensor `rows` starts shifts[i] elements past a 256-byte boundary."""
    buf = torch.full((rows.shape[0], (L + 127) // 64 * 64), fill, dtype=rows.dtype, device=dev)
    views = [buf[i, s:s + L] for i, s in enumerate(shifts)]
    for v, row, s in zip(views, rows, shifts):
        v.copy_(row)
        assert v.data_ptr() % 256 == s * rows.element_size()
    return buf, views


def _call(dt, views, K, ref, hviews, dev, work=None, groups=0):
    """One fedagg_histgram_16 call on row views; groups > 0 forces that many chunk groups."""
    chunks = kn.upload_i64(TABLE.ravel().tolist(), dev)
    if work is None:
        work = torch.empty(tgf._per(K) * groups if groups else
                           int(nat.lib().fedagg_robust_work_len(nat.WORK_HISTGRAM, K, len(TABLE))),
                           dtype=torch.float64, device=dev)
    out = torch.empty((K, K), dtype=torch.float64, device=dev)
    ptrs = kn.upload_i64([v.data_ptr() for v in views[:K]], dev)
    hp = kn.upload_i64([v.data_ptr() for v in hviews[:K]], dev) if hviews is not None else None
    nat.check(nat.lib().fedagg_histgram_16(DT[dt], ptrs.data_ptr(), K, ref.data_ptr(),
                                           hp.data_ptr() if hp is not None else None, chunks.data_ptr(), len(TABLE),
                                           out.data_ptr(), work.data_ptr(),
                                           tgf._per(K) * groups if groups else work.numel(), nat.stream_handle()),
              "histgram_16")
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gauss(dt, K):
    """16-bit inputs and the references of histgram_rows_torch on the CPU, with and without history."""
    x, r = torch.from_numpy(gaussian_rows(K, L, 10 + K)).to(dt), torch.from_numpy(gaussian_rows(1, L, 7)).to(dt)
    h = torch.from_numpy(gaussian_rows(K + 1, L, 20 + K))  # one history row more than clients: it must stay untouched
    cols = torch.from_numpy(COLS)
    hnew = h.clone()
    G_h = dfn.histgram_rows_torch(x.float(), r[0].float(), hnew[:K], cols).numpy()
    G_0 = dfn.histgram_rows_torch(x.float(), r[0].float(), None, cols).numpy()
    return x, r, h, hnew.numpy(), G_h, G_0


def _check(dt, K, hist, groups, xshift, rshift, hshift):
    dev = torch.device("cuda", 0)
    x, r, h, hnew, G_h, G_0 = _gauss(dt, K)
    _, xv = _place(x, xshift, dev)
    _, rv = _place(r, [rshift], dev)
    hbuf, hv = _place(h, hshift, dev, fill=-7.0)
    G = _call(dt, xv, K, rv[0], hv if hist else None, dev, groups=groups)
    ref = G_h if hist else G_0
    n = np.diag(ref)
    ratio = (np.abs(G - ref) / (n[:, None] + n[None, :])).max()
    print(f"HISTGRAM16_RATIO {dt} K={K} hist={hist} groups={groups} {ratio:.3e}")
    assert (np.abs(G - ref) <= 1e-6 * (n[:, None] + n[None, :]) + 1e-300).all()
    assert np.array_equal(G, G.T)
    want = np.full(tuple(hbuf.shape), -7.0, dtype=np.float32)
    for i, s in enumerate(hshift):
        want[i, s:s + L] = hnew[i] if hist else h[i].numpy()  # hnew: updated on COLS only, row K not at all
    assert np.array_equal(hbuf.cpu().numpy(), want)


@pytest.mark.parametrize("groups", [0, 3])  # the default workspace; 3 groups: ~20 stages a block, folds mid-stream
@pytest.mark.parametrize("hist", [True, False])
@pytest.mark.parametrize("K", [1, 16, 17, 113, 128])
@pytest.mark.parametrize("dt", DTS)
def test_gram_and_history(dt, K, hist, groups):
    # rows at shifts 1 .. 3 are not 8-byte aligned: their waves load by element
    _check(dt, K, hist, groups, [i % 4 for i in range(K)], 1, [(i + 1) % 4 for i in range(K + 1)])


@pytest.mark.parametrize("dt", DTS)
def test_all_rows_aligned(dt):
    _check(dt, 128, True, 0, [0] * 128, 0, [0] * 129)  # every load of a full stage at a multiple of 4 is the vector form


@pytest.mark.parametrize("K", [16, 113, 128])
@pytest.mark.parametrize("dt", DTS)
def test_exact_integers(dt, K):
    dev = torch.device("cuda", 0)
    x, h = integer_rows(K, L, K, -1, 1), integer_rows(K, L, K + 1, -1, 1)
    r = integer_rows(1, L, 3, -1, 1)
    A = (x.astype(np.int64) - r.astype(np.int64) + h.astype(np.int64))[:, COLS]
    want = (A @ A.T).astype(np.float64)
    _, xv = _place(torch.from_numpy(x).to(dt), [0] * K, dev)
    _, rv = _place(torch.from_numpy(r).to(dt), [0], dev)
    n_def = int(nat.lib().fedagg_robust_work_len(nat.WORK_HISTGRAM, K, len(TABLE)))
    for groups, poisoned in ((0, False), (1, False), (2, False), (0, True)):
        _, hv = _place(torch.from_numpy(h), [0] * K, dev)
        work = torch.full((n_def + 64,), float("nan"), dtype=torch.float64, device=dev) if poisoned else None
        G = _call(dt, xv, K, rv[0], hv, dev, work=work[:n_def] if poisoned else None, groups=groups)
        assert np.array_equal(G, want), (groups, poisoned)
        if poisoned:
            assert torch.isnan(work[n_def:]).all()


# ---- the rule ---------------------------------------------------------------------

def _cast(d, dt, i=0):
    """A model of test_gpu_foolsgold.py as a device-resident `dt` model with an int64 counter."""
    out = OrderedDict((k, v.to(dt).cuda()) for k, v in d.items())
    out["bn.num_batches_tracked"] = torch.tensor(3 + i, dtype=torch.int64).cuda()
    return out


@functools.lru_cache(maxsize=None)
def _two_rounds(dt, K, method):
    g32 = tgf._model(np.random.default_rng(5))
    g, state = _cast(g32, dt), dfn.FoolsGoldState()
    for rnd in range(2):
        clients = [(n, _cast(d, dt, i)) for i, (n, d) in enumerate(tgf._round(K, 100 * rnd + K, g32))]
        out, info = dfn.foolsgold(clients, g, state, method=method, return_info=True)
    return g, clients, out, info


@pytest.mark.parametrize("K,method", [(8, "fused"), (8, "composed"), (130, "composed")])
@pytest.mark.parametrize("dt", DTS)
def test_rule_two_rounds(dt, K, method):
    g, clients, out, info = _two_rounds(dt, K, method)
    assert info.method == method
    assert all(info.alpha[i] == 0 for i in tgf.SYBILS)
    assert all(info.alpha[i] > 0 for i in range(K) if i not in tgf.SYBILS)
    if K == 8:
        other = _two_rounds(dt, K, "composed" if method == "fused" else "fused")[3]
        assert np.abs(info.alpha - other.alpha).max() <= 1e-9
    incl = [i for i in range(K) if info.alpha[i] > 0]
    assert list(out.keys()) == list(g.keys())
    for k in g:
        wide = (lambda t: t.flatten()) if g[k].is_floating_point() else (lambda t: t.flatten().float())
        want = dfn.wsum_diff_rows_torch([wide(clients[i][1][k]) for i in incl], info.coeffs[incl], wide(g[k]))
        assert out[k].dtype == (dt if g[k].is_floating_point() else torch.float32)
        assert torch.equal(out[k].flatten(), want), k


@pytest.mark.parametrize("method", ["fused", "composed"])
@pytest.mark.parametrize("dt", DTS)
def test_nan_client(dt, method):
    g32 = tgf._model(np.random.default_rng(5))
    state = dfn.FoolsGoldState()
    clients = [(n, _cast(d, dt, i)) for i, (n, d) in enumerate(tgf._round(8, 1, g32, bad=5))]
    out, info = dfn.foolsgold(clients, _cast(g32, dt), state, method=method, return_info=True)
    assert info.alpha[5] == 0 and info.alpha[0] > 0
    assert not state.rows[state.slots[5]].any() and state.rows[state.slots[0]].any()
    assert all(torch.isfinite(t).all() for t in out.values())
