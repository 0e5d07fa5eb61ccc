"""fedagg_histgram_f32 (csrc/histgram.hip) against the fp64 reference, and the
"foolsgold_cos" rule end to end, on the device.

Measured on an MI355X: the largest HISTGRAM_RATIO over the cases of
test_gram_and_history is 1.36e-7 (the bound, 1e-6, is not tightened to it).
"""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

from chunk_groups import gaussian_rows, integer_rows, shifted_rows
from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn

pytestmark = pytest.mark.gpu

L = 5000
SEGS = [(0, 1), (3, 700), (704, 1), (960, 2500), (4000, 999)]  # ragged, four gaps, partial stages everywhere
TABLE = np.array([(s, min(nat.PAIR_CHUNK, o + n - s)) for o, n in SEGS for s in range(o, o + n, nat.PAIR_CHUNK)],
                 dtype=np.int64)
COLS = np.concatenate([np.arange(s, s + n) for s, n in TABLE])


def _per(K):
    nb = (K + 15) // 16
    return nb * (nb + 1) // 2 * 256


def _call(views, K, ref, hviews, dev, work=None, groups=0):
    """One fedagg_histgram_f32 call on row views; groups > 0 forces that many chunk groups."""
    chunks = kn.upload_i64(TABLE.ravel().tolist(), dev)
    if work is None:
        work = torch.empty(_per(K) * groups if groups else
                           int(nat.lib().fedagg_robust_work_len(nat.WORK_HISTGRAM, K, len(TABLE))),
                           dtype=torch.float64, device=dev)
    out = torch.empty((K, K), dtype=torch.float64, device=dev)
    ptrs = kn.upload_i64([v.data_ptr() for v in views[:K]], dev)
    hp = kn.upload_i64([v.data_ptr() for v in hviews[:K]], dev) if hviews is not None else None
    nat.check(nat.lib().fedagg_histgram_f32(ptrs.data_ptr(), K, ref.data_ptr(), hp.data_ptr() if hp is not None else None,
                                            chunks.data_ptr(), len(TABLE), out.data_ptr(), work.data_ptr(),
                                            _per(K) * groups if groups else work.numel(), nat.stream_handle()),
              "histgram")
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gauss(K):
    """Inputs and the references of histgram_rows_torch on the CPU, with and without history."""
    x, r = gaussian_rows(K, L, 10 + K), gaussian_rows(1, L, 7)[0]
    h = gaussian_rows(K + 1, L, 20 + K)  # one history row more than clients: it must stay untouched
    cols = torch.from_numpy(COLS)
    hnew = torch.from_numpy(h.copy())
    G_h = dfn.histgram_rows_torch(torch.from_numpy(x), torch.from_numpy(r), hnew[:K], cols).numpy()
    G_0 = dfn.histgram_rows_torch(torch.from_numpy(x), torch.from_numpy(r), None, cols).numpy()
    return x, r, h, hnew.numpy(), G_h, G_0


@pytest.mark.parametrize("groups", [0, 3])  # the default workspace; 3 groups: ~20 stages a block, folds mid-stream
@pytest.mark.parametrize("hist", [True, False])
@pytest.mark.parametrize("K", [1, 16, 17, 112, 113, 128])
def test_gram_and_history(K, hist, groups):
    dev = torch.device("cuda", 0)
    x, r, h, hnew, G_h, G_0 = _gauss(K)
    _, xv = shifted_rows(x, [i % 4 for i in range(K)], dev)
    _, rv = shifted_rows(r[None], [1], dev)
    hshift = [(i + 1) % 4 for i in range(K + 1)]
    hbuf, hv = shifted_rows(h, hshift, dev, fill=-7.0)
    G = _call(xv, K, rv[0], hv if hist else None, dev, groups=groups)
    ref = G_h if hist else G_0
    n = np.diag(ref)
    ratio = (np.abs(G - ref) / (n[:, None] + n[None, :])).max()
    print(f"HISTGRAM_RATIO K={K} hist={hist} groups={groups} {ratio:.3e}")
    assert (np.abs(G - ref) <= 1e-6 * (n[:, None] + n[None, :]) + 1e-300).all()
    assert np.array_equal(G, G.T)
    want = np.full(tuple(hbuf.shape), -7.0, dtype=np.float32)
    for i, s in enumerate(hshift):
        want[i, s:s + L] = hnew[i] if hist else h[i]  # hnew: updated on COLS only, row K not at all
    assert np.array_equal(hbuf.cpu().numpy(), want)


@pytest.mark.parametrize("K", [16, 113, 128])
def test_exact_integers(K):
    dev = torch.device("cuda", 0)
    x, h = integer_rows(K, L, K, -1, 1), integer_rows(K, L, K + 1, -1, 1)
    r = integer_rows(1, L, 3, -1, 1)
    A = (x.astype(np.int64) - r.astype(np.int64) + h.astype(np.int64))[:, COLS]
    want = (A @ A.T).astype(np.float64)
    _, xv = shifted_rows(x, [0] * K, dev)
    _, rv = shifted_rows(r, [0], dev)
    n_def = int(nat.lib().fedagg_robust_work_len(nat.WORK_HISTGRAM, K, len(TABLE)))
    for groups, poisoned in ((0, False), (1, False), (2, False), (0, True)):
        _, hv = shifted_rows(h, [0] * K, dev)
        work = torch.full((n_def + 64,), float("nan"), dtype=torch.float64, device=dev) if poisoned else None
        G = _call(xv, K, rv[0], hv, dev, work=work[:n_def] if poisoned else None, groups=groups)
        assert np.array_equal(G, want), (groups, poisoned)
        if poisoned:
            assert torch.isnan(work[n_def:]).all()


# ---- the rule ---------------------------------------------------------------------

SYBILS = (1, 4, 6)


def _model(rng, scale=1.0):
    return OrderedDict([("fc.weight", torch.from_numpy((scale * rng.standard_normal((40, 7))).astype(np.float32))),
                        ("bn.running_mean", torch.from_numpy((scale * rng.standard_normal(7)).astype(np.float32))),
                        ("fc.bias", torch.from_numpy((scale * rng.standard_normal(7)).astype(np.float32)))])


def _round(K, seed, g, bad=None):
    """K clients: honest ones send g + an independent update, the sybils g + one shared direction + tiny noise."""
    rng = np.random.default_rng(seed)
    push = _model(np.random.default_rng(99), 0.1)
    out = []
    for i in range(K):
        u = _model(rng, 1e-4 if i in SYBILS else 0.1)
        d = OrderedDict((k, g[k] + u[k] + (push[k] if i in SYBILS else 0)) for k in g)
        if i == bad:
            d["fc.weight"][3, 2] = float("nan")
        out.append((10.0 + i, d))
    return out


@functools.lru_cache(maxsize=None)
def _two_rounds(K, method):
    g = _model(np.random.default_rng(5))
    state = dfn.FoolsGoldState()
    for rnd in range(2):
        clients = _round(K, 100 * rnd + K, g)
        out, info = dfn.foolsgold(clients, g, state, method=method, return_info=True)
    return g, clients, out, info


@pytest.mark.parametrize("K,method", [(8, "fused"), (8, "composed"), (130, "composed")])
def test_rule_two_rounds(K, method):
    g, clients, out, info = _two_rounds(K, method)
    assert info.method == method
    assert all(info.alpha[i] == 0 for i in SYBILS)
    assert all(info.alpha[i] > 0 for i in range(K) if i not in SYBILS)
    if K == 8:
        assert np.abs(info.alpha - _two_rounds(K, "composed" if method == "fused" else "fused")[3].alpha).max() <= 1e-9
    incl = [i for i in range(K) if info.alpha[i] > 0]
    assert list(out.keys()) == list(g.keys())
    for k in g:
        want = dfn.wsum_diff_rows_torch([clients[i][1][k].flatten() for i in incl], info.coeffs[incl], g[k].flatten())
        assert torch.equal(out[k].flatten(), want), k


@pytest.mark.parametrize("method", ["fused", "composed"])
def test_nan_client_and_all_copies(method):
    g = _model(np.random.default_rng(5))
    state = dfn.FoolsGoldState()
    out, info = dfn.foolsgold(_round(8, 1, g, bad=5), g, state, method=method, return_info=True)
    assert info.alpha[5] == 0 and info.alpha[0] > 0
    assert not state.rows[state.slots[5]].any()
    assert all(torch.isfinite(t).all() for t in out.values())
    copies = dfn.FoolsGoldState()  # K identical clients: each is another's copy, nobody is trusted
    same = _round(1, 2, g)[0][1]
    for _ in range(2):
        out, info = dfn.foolsgold([(1.0, same)] * 8, g, copies, method=method, return_info=True)
    assert not info.alpha.any()
    assert all(torch.equal(out[k], g[k]) for k in g)
