"""The "fltrust" defense on the device: fedagg_dotnorm2_f32 and
fedagg_wsum_diff_f32 (csrc/robust.hip) at the smallest shapes at which each of
their paths can go wrong, and fedml_amd.defense.fltrust end to end.

Bounds.  dotnorm2 sums exact fp64 products in its own fixed order: any-order
fp64 summation of n terms errs by at most (n - 1) 2^-53 sum|terms|; doubled
for the wave-level and group-level combines, |got - fsum| <= n 2^-52
sum|terms| with n the table's columns (the reference, math.fsum, is correctly
rounded).  The cosine divides a dot by two roots: each of the three sums errs
by at most n 2^-53 sum|terms| and sum|a b| <= |a| |b|, so the cosine errs by
at most n 2^-52, doubled again for the roots and the divisions: n 2^-50.
wsum_diff is an fp32 chain with a fixed order: bit for bit.
"""
from __future__ import annotations

import logging
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chunk_groups as cg
import fltrust_ref as ref
from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn
from test_fltrust import check_fma_column, fma_rows

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = -7.25
# a block pass of dotnorm2_kernel is kWaves * kDotBatch = 4 * 8 = 32 clients
# (csrc/robust.hip); 63 .. 65 are the edges of the 16-client build the probe
# times beside it, two passes here
DOT_KS = (1, 2, 31, 32, 33, 63, 64, 65, 129)
TILE = nat.WSUM_DIFF_TILE  # FEDAGG_WSUM_DIFF_TILE, the kernel's kWdTile


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def ptr_table(views, dev):
    return kn.upload_i64([v.data_ptr() for v in views], dev)


# ---- fedagg_dotnorm2_f32 ------------------------------------------------------------

@pytest.fixture(scope="module")
def dist_table(cuda_device):
    tab, cols = cg.tiny_chunk_table(nat.DIST_CHUNK, cg.STRIDE256_CHUNKS, 0)
    assert len(cols) <= cg.MAX_TABLE_COLUMNS
    L = int(cols[-1]) + 4
    outside = np.setdiff1d(np.arange(L), cols)
    assert len(outside) > 0
    return tab, cols, outside, kn.upload_i64(tab.reshape(-1).tolist(), cuda_device), L


def _dotnorm2(ptrs, K, d_ref, d_dir, d_chunks, n, G, dev, what):
    """One call with the workspace that forces G chunk groups: every one of
    its 2 K G doubles written, nothing past them."""
    wl = 2 * K * G
    work = torch.full((wl + 64,), NAN, dtype=torch.float64, device=dev)
    out = torch.full((2 * K,), NAN, dtype=torch.float64, device=dev)
    nat.check(nat.lib().fedagg_dotnorm2_f32(ptrs.data_ptr(), K, d_ref.data_ptr(), d_dir.data_ptr(),
                                            d_chunks.data_ptr(), n, out.data_ptr(), work.data_ptr(), wl,
                                            nat.stream_handle()), what)
    unwritten = int(torch.isnan(work[:wl]).sum().item())
    assert unwritten == 0, f"{what}: {unwritten} of {wl} workspace doubles not written (G = {G} did not run)"
    assert bool(torch.isnan(work[wl:]).all().item()), f"{what}: written past work_len"
    return out.cpu().numpy()


@pytest.mark.parametrize("K", DOT_KS)
def test_dotnorm2_every_group_count(K, dist_table, cuda_device):
    """K rows, the last of them the direction itself (the root as a row), at
    every alignment mod 4 (rows i mod 4, ref and dir their own), NaN in every
    column outside the table, G = 1 .. 513 groups on 600 tiny chunks."""
    dev = cuda_device
    tab, cols, outside, d_chunks, L = dist_table
    n, ncols = len(tab), len(cols)
    rng = np.random.default_rng(50 + K)
    g = (0.05 * rng.standard_normal(L)).astype(np.float32)
    b = (0.01 * rng.standard_normal(L)).astype(np.float32)
    r = (g + b).astype(np.float32)
    rows = (g[None, :] + b[None, :] + 0.01 * rng.standard_normal((K, L))).astype(np.float32)
    if K > 2:
        rows[1] = (g - 3 * b).astype(np.float32)  # an attacker: a negative dot
    rows[K - 1] = r
    for a in (g, r, rows):
        a[..., outside] = NAN
    wd, wda, wn, wnb = ref.dot_norm(rows, g, r, cols)
    assert wd[K - 1] == wnb == wn[K - 1] and (K <= 2 or wd[1] < 0)
    _, views = cg.shifted_rows(rows, [i % 4 for i in range(K)], dev)
    _, (d_ref,) = cg.shifted_rows(g[None, :], [1 + K % 3], dev)
    _, (d_dir,) = cg.shifted_rows(r[None, :], [(K + 2) % 4], dev)
    ptrs = ptr_table(views[:K - 1] + [d_dir], dev)
    tol = ncols * 2.0 ** -52
    worst = 0.0
    for G in cg.STRIDE256_G:
        what = f"dotnorm2 K={K} G={G}"
        got = _dotnorm2(ptrs, K, d_ref, d_dir, d_chunks, n, G, dev, what)
        again = _dotnorm2(ptrs, K, d_ref, d_dir, d_chunks, n, G, dev, what)
        assert np.array_equal(bits64(got), bits64(again)), f"{what}: not deterministic"
        dot, n2 = got[:K], got[K:]
        assert np.isfinite(got).all(), f"{what}: a column outside the table was read"
        for i in range(K):
            worst = max(worst, abs(dot[i] - wd[i]) / wda[i], abs(n2[i] - wn[i]) / wn[i])
            assert abs(dot[i] - wd[i]) <= tol * wda[i], (what, i, dot[i], wd[i])
            assert abs(n2[i] - wn[i]) <= tol * wn[i], (what, i, n2[i], wn[i])
        assert bits64(dot[K - 1]) == bits64(n2[K - 1]), f"{what}: the root's dot is not its squared norm"
    print(f"DOTNORM2_WORST K={K} {worst:.3e} (bound {tol:.3e})")


def test_dotnorm2_default_workspace_and_empty_table(dist_table, cuda_device):
    """defense.dotnorm2_rows (the full workspace: G = n_chunks) and n_chunks == 0."""
    dev = cuda_device
    tab, cols, outside, d_chunks, L = dist_table
    K = 5
    rng = np.random.default_rng(7)
    rows = (0.05 * rng.standard_normal((K, L))).astype(np.float32)
    g = (0.05 * rng.standard_normal(L)).astype(np.float32)
    r = (0.05 * rng.standard_normal(L)).astype(np.float32)
    d_rows = torch.from_numpy(rows).to(dev)
    d_g, d_r = torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev)
    ptrs = ptr_table([d_rows[i] for i in range(K)], dev)
    dot, n2 = dfn.dotnorm2_rows(ptrs, K, d_g, d_r, d_chunks, len(tab), dev)
    wd, wda, wn, _ = ref.dot_norm(rows, g, r, cols)
    tol = len(cols) * 2.0 ** -52
    assert all(abs(float(dot[i]) - wd[i]) <= tol * wda[i] and abs(float(n2[i]) - wn[i]) <= tol * wn[i]
               for i in range(K))
    td, tn = dfn.dotnorm2_rows_torch(d_rows, d_g, d_r, torch.from_numpy(cols).to(dev))  # the spec, on the device
    assert all(abs(float(td[i]) - wd[i]) <= tol * wda[i] and abs(float(tn[i]) - wn[i]) <= tol * wn[i]
               for i in range(K))
    dot, n2 = dfn.dotnorm2_rows(ptrs, K, d_g, d_r, d_chunks, 0, dev)
    assert dot.tolist() == [0.0] * K and n2.tolist() == [0.0] * K


# ---- fedagg_wsum_diff_f32 -----------------------------------------------------------

WD_NS = (TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 1)
# (rows aligned?, ref shift, out shift): every row, ref and out on a 16-byte
# boundary (the vector path throughout), then each of them off it, alone and together
WD_SHIFTS = ((True, 0, 0), (False, 0, 0), (True, 1, 0), (True, 0, 2), (False, 3, 1), (False, 2, 3))


@pytest.mark.parametrize("K", [0, 1, 2, 3, 17])
def test_wsum_diff_tile_edges_and_alignments(K, cuda_device):
    """K = 1: the chain's first term alone; 2, 3: the client loop's tail only;
    17: four rounds of four clients in flight.  N around the 2,048-column tile
    (a ragged last tile takes the bounded 4-byte path), rows, ref and out each
    0 .. 3 elements past a 16-byte boundary, 0.0, a subnormal and the
    FMA-revealing value among the coefficients, guards around out."""
    dev = cuda_device
    for case, N in enumerate(WD_NS):
        rows, g, c = fma_rows(K, N, 1000 * K + N)
        want = ref.rebuild(rows, c, g)
        d_c = kn.upload_f32(c, dev) if K else None
        for aligned, rs, os_ in WD_SHIFTS:
            what = f"wsum_diff K={K} N={N} rows_aligned={aligned} ref+{rs} out+{os_}"
            ptrs = None
            if K:
                _, views = cg.shifted_rows(rows, [0 if aligned else (i + case + 1) % 4 for i in range(K)], dev)
                ptrs = ptr_table(views, dev)
            _, (d_ref,) = cg.shifted_rows(g[None, :], [rs], dev)
            obuf, (d_out,) = cg.shifted_rows(np.full((1, N), GUARD, np.float32), [os_], dev, fill=GUARD)
            dfn.wsum_diff_rows(ptrs, d_c, K, d_ref, N, d_out)
            ob = obuf.cpu().numpy()[0]
            got = ob[os_:os_ + N]
            bad = np.flatnonzero(bits32(got) != bits32(want))
            assert bad.size == 0, f"{what}: columns {bad[:8].tolist()}"
            assert (ob[:os_] == GUARD).all() and (ob[os_ + N:] == GUARD).all(), f"{what}: guard"
            check_fma_column(got[0], K)
            check_fma_column(got[N - 1], K)
            if K == 0:
                assert np.array_equal(bits32(got), bits32(g)), what


def test_wsum_diff_matches_the_torch_specification_on_the_device(cuda_device):
    dev = cuda_device
    K, N = 6, 2 * TILE + 3
    rows, g, c = fma_rows(K, N, 5)
    d_rows, d_g = torch.from_numpy(rows).to(dev), torch.from_numpy(g).to(dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    dfn.wsum_diff_rows(ptr_table([d_rows[i] for i in range(K)], dev), kn.upload_f32(c, dev), K, d_g, N, out)
    spec = dfn.wsum_diff_rows_torch(d_rows, c, d_g)
    assert torch.equal(out.view(torch.int32), spec.view(torch.int32))


def test_wsum_diff_beyond_32_bit_columns(cuda_device):
    """2^31 + 12,345 columns: 64-bit column indices in both access paths, and
    more tiles (2^20 + 7) than the grid's 2^20 blocks, so the first blocks go
    round.  Every column's chain is independent of N: the reference runs on
    sampled columns (random ones, both ends, around 2^31)."""
    dev = cuda_device
    N, K = 2 ** 31 + 12_345, 2
    gen = torch.Generator(device=dev).manual_seed(3)
    buf = torch.empty((K + 1, (N + 8 + 3) // 4 * 4), dtype=torch.float32, device=dev)
    buf[K].normal_(0.0, 0.05, generator=gen)
    for i in range(K):
        buf[i].normal_(0.0, 0.01, generator=gen).add_(buf[K])
    c = [0.75, float(np.float32(0.3))]
    rng = np.random.default_rng(4)
    cols = np.unique(np.concatenate([rng.integers(0, N, 100_000), np.arange(64), np.arange(N - 64, N),
                                     np.arange(2 ** 31 - 64, 2 ** 31 + 64)]))
    idx = torch.from_numpy(cols).to(dev)
    out = torch.full((N + 8,), GUARD, dtype=torch.float32, device=dev)
    for shift in (0, 1):  # 16-byte and 4-byte accesses (the row stride is a multiple of 16 bytes)
        rows = [buf[i, shift:shift + N] for i in range(K)]
        g = buf[K, shift:shift + N]
        assert g.data_ptr() % 16 == 4 * shift
        out.fill_(GUARD)
        o = out[shift:shift + N]
        dfn.wsum_diff_rows(ptr_table(rows, dev), kn.upload_f32(c, dev), K, g, N, o)
        want = ref.rebuild([r[idx].cpu().numpy() for r in rows], c, g[idx].cpu().numpy())
        assert np.array_equal(bits32(o[idx].cpu().numpy()), bits32(want)), f"shift {shift}"
        assert bool((out[:shift] == GUARD).all()) and bool((out[shift + N:] == GUARD).all()), f"shift {shift}: guard"
    del buf, out
    torch.cuda.empty_cache()


# ---- defense.fltrust end to end -----------------------------------------------------

W_SHAPE, BN = (37, 31), 31   # 1,147 weight columns: two chunks of the table, neither a whole one
E2E_K, E2E_BAD = 9, (6, 7, 8)


def _flat(d):
    """the model as one fp32 row in key order, integer keys as fl32(v)"""
    return np.concatenate([d[k].detach().reshape(-1).cpu().to(torch.float32).numpy()
                           for k in ("weight", "bn.running_mean", "bn.num_batches_tracked")])


@pytest.fixture(scope="module")
def e2e():
    """(clients, g, r, reference) with host tensors: six honest clients at
    g + b + noise, three attackers at g - 3 b, the last of them with a NaN in
    a weight.  The reference's cosines stay clear of 0, so the ReLU's branch
    does not hang on the last bits."""
    rng = np.random.default_rng(11)
    nw = W_SHAPE[0] * W_SHAPE[1]

    def model(w, m, cnt):
        return OrderedDict([("weight", torch.from_numpy(w.astype(np.float32).reshape(W_SHAPE))),
                            ("bn.running_mean", torch.from_numpy(m.astype(np.float32))),
                            ("bn.num_batches_tracked", torch.tensor(cnt, dtype=torch.int64))])

    gw, gm = 0.05 * rng.standard_normal(nw), 0.1 * rng.standard_normal(BN)
    bw, bm = 0.01 * rng.standard_normal(nw), 0.01 * rng.standard_normal(BN)
    g, r = model(gw, gm, 100), model(gw + bw, gm + bm, 110)
    clients = []
    for i in range(E2E_K):
        if i in E2E_BAD:
            d = model(gw - 3 * bw, gm - 3 * bm, 70)
        else:
            d = model(gw + bw + 0.005 * rng.standard_normal(nw), gm + bm + 0.005 * rng.standard_normal(BN), 105 + i)
        clients.append((10 + i, d))
    clients[8][1]["weight"][3, 4] = NAN
    want = ref.fltrust([_flat(d) for _, d in clients], _flat(g), _flat(r), np.arange(nw))
    cos = want[1]
    assert all(abs(cos[i]) > 1e-3 for i in range(E2E_K) if np.isfinite(cos[i])) and np.isnan(cos[8])
    assert want[4] == [0, 1, 2, 3, 4, 5]
    return clients, g, r, want


def _to(d, dev):
    return OrderedDict((k, v.to(dev)) for k, v in d.items())


def _snapshot(dicts):
    return [OrderedDict((k, v.clone()) for k, v in d.items()) for d in dicts]


def _same(a, b):
    return all(torch.equal(torch.nan_to_num(a[k].double().cpu(), nan=123.0),
                           torch.nan_to_num(b[k].double().cpu(), nan=123.0)) and a[k].dtype == b[k].dtype for k in a)


@pytest.mark.parametrize("where", ["host", "device"])
def test_fltrust_end_to_end(where, e2e, cuda_device):
    dev = cuda_device
    clients, g, r, (want_out, want_cos, want_trust, want_c32, want_trusted) = e2e
    if where == "device":
        clients = [(n, _to(d, dev)) for n, d in clients]
        g, r = _to(g, dev), _to(r, dev)
    before = _snapshot([d for _, d in clients] + [g, r])
    out, info = dfn.fltrust(clients, g, r, device=dev, return_info=True)
    assert all(_same(a, b) for a, b in zip(before, [d for _, d in clients] + [g, r])), "an input was modified"
    assert info.trusted == [0, 1, 2, 3, 4, 5]
    nw = W_SHAPE[0] * W_SHAPE[1]
    for i in range(E2E_K):
        if np.isfinite(want_cos[i]):
            assert abs(info.cos[i] - want_cos[i]) <= nw * 2.0 ** -50, (i, info.cos[i], want_cos[i])
        else:
            assert not np.isfinite(info.cos[i])
    assert (info.coeffs[list(E2E_BAD)] == 0).all() and (info.coeffs[:6] > 0).all()
    assert abs(info.root_norm - np.sqrt(ref.dot_norm([], _flat(g), _flat(r), np.arange(nw))[3])) <= 1e-12
    # the output is the specification's chain with the coefficients used, bit for bit
    rows = torch.from_numpy(np.stack([_flat(d) for _, d in clients]))
    spec = dfn.wsum_diff_rows_torch([rows[i] for i in info.trusted], [info.coeffs[i] for i in info.trusted],
                                    torch.from_numpy(_flat(g))).numpy()
    assert list(out) == ["weight", "bn.running_mean", "bn.num_batches_tracked"]
    got = np.concatenate([out[k].reshape(-1).cpu().numpy() for k in out])
    assert np.array_equal(bits32(got), bits32(spec))
    assert all(v.dtype == torch.float32 and v.device.type == ("cuda" if where == "device" else "cpu")
               for v in out.values())
    assert out["weight"].shape == W_SHAPE and out["bn.num_batches_tracked"].shape == ()
    assert np.isfinite(got).all(), "the untrusted client's NaN reached the output"
    # ... and close to the independent reference (its coefficients may differ in the last bits of the cosines)
    np.testing.assert_allclose(got, want_out, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(info.coeffs, want_c32, rtol=1e-6, atol=0)


def _model(g):
    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(g["weight"].clone())
            self.bn = torch.nn.Module()
            self.bn.register_buffer("running_mean", g["bn.running_mean"].clone())
            self.bn.register_buffer("num_batches_tracked", g["bn.num_batches_tracked"].clone())

    return M()


def test_fltrust_through_the_server_aggregator(e2e, cuda_device):
    from fedml_amd.server_aggregator import MI355XServerAggregator

    clients, g, r, _ = e2e
    args = SimpleNamespace(federated_optimizer="FedAvg", enable_defense=True, defense_type="fltrust",
                           fltrust_lr=0.5, fedagg_device=str(cuda_device))
    agg = MI355XServerAggregator(_model(g), args)
    assert list(agg.get_model_params()) == list(g)
    direct = dfn.fltrust(clients, g, r, 0.5, cuda_device)
    lst, idxs = agg.on_before_aggregation(clients)
    assert lst is clients
    agg.set_fltrust_root(r)
    out = agg.on_after_aggregation(agg.aggregate(lst))
    assert list(out) == list(direct)
    assert all(np.array_equal(bits32(out[k].numpy()), bits32(direct[k].numpy())) for k in out)
    with pytest.raises(RuntimeError, match="set_fltrust_root"):
        agg.aggregate(lst)


def test_fltrust_round_of_attackers_keeps_the_global_model(e2e, cuda_device, caplog):
    clients, g, r, _ = e2e
    bad = [clients[i] for i in E2E_BAD]
    with caplog.at_level(logging.WARNING):
        out, info = dfn.fltrust(bad, g, r, device=cuda_device, return_info=True)
    assert "global model is kept" in caplog.text
    assert info.trusted == [] and (info.coeffs == 0).all() and (info.trust == 0).all()
    assert np.array_equal(bits32(np.concatenate([out[k].reshape(-1).numpy() for k in out])), bits32(_flat(g)))
    assert out["bn.num_batches_tracked"].dtype == torch.float32
