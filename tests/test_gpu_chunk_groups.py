"""The distance kernels (csrc/robust.hip: dist2, pairtri<16|32>, pairdist,
pairgram_split8<1..8>, clip_diff; csrc/geomed.hip: wsum_dist2<8..128>) at
every chunk-group count G and finish path, on tables of many tiny chunks
(tests/chunk_groups.py).  The other small-shape tests run G = n_chunks only:
every block walks one chunk, the Gram never folds mid-stream and the finish
kernels run only their predicated tails.

Each test calls the C ABI with a workspace of work_len + 64 doubles filled
with NaN and passes the work_len that forces G groups.  Afterwards the first
work_len doubles hold no NaN (every partial slot, and the Gram's matrix M,
was written: the call ran with the intended G) and the 64 after them are
still NaN (nothing is written past a reduced workspace).

Bounds.  Integer inputs in [-8, 8]: differences, squares, fp32 stage sums
(<= 64 * 256) and fp64 sums are exact, so dist2 and pairdist2 equal the
integer reference bit for bit at every G.  Gaussian inputs: dist2 within
1e-12 relative of numpy's fp64 sum (test_dist2_vs_numpy's bound); pairdist2
within 2^-18 relative (an fp32 FMA chain over <= 64 non-negative terms) and
within 1e-12 between any two G (the stage sums do not depend on G).  The Gram
within 2e-6 (|c_i|^2 + |c_j|^2) (test_pairgram2_vs_numpy's bound; at most 4
stages are summed in fp32 whatever G is), and bit-exact on {-1, 0, 1} entries
for K = 2, 4, 16, 64 (derivation: test_chunk_groups.py).  wsum_dist2: z bit
for bit the numpy chain and fedagg_wsum_f32 at every G, D within 1e-12.  clip
and scale: bit for bit the numpy rounding chains, NaN by position.

Largest observed Gram ratio |D - ref| / (|c_i|^2 + |c_j|^2) over all K and G
on an MI355X: 1.94e-7 (K = 64; every K >= 16 between 1.5e-7 and 1.94e-7),
a tenth of the 2e-6 bound.  The module takes about 6 s there.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import chunk_groups as cg
import geomed_ref
from fedml_amd import _native as nat
from fedml_amd import kernels as kn
from test_chunk_groups import (CLIP_KS, CLIP_NS, DIST2_KS, GRAM_EXACT_KS, GRAM_KS, PAIR_KS, WSUM_KS)
from test_gpu_geomed import GUARD, client_rows

pytestmark = pytest.mark.gpu

NAN = float("nan")


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _table(chunk_max, n_chunks, dev):
    tab, cols = cg.tiny_chunk_table(chunk_max, n_chunks, 0)
    assert len(cols) <= cg.MAX_TABLE_COLUMNS
    return tab, cols, kn.upload_i64(tab.reshape(-1).tolist(), dev), int(cols[-1]) + 4


@pytest.fixture(scope="module")
def pair_table(cuda_device):
    return _table(nat.PAIR_CHUNK, cg.QUARTERED_CHUNKS, cuda_device)


@pytest.fixture(scope="module")
def dist_table(cuda_device):
    return _table(nat.DIST_CHUNK, cg.STRIDE256_CHUNKS, cuda_device)


def run_forced(kind, K, G, dev, call, what):
    """call(work pointer, work_len) with the workspace that forces G chunk
    groups; every slot written, nothing past work_len."""
    wl = cg.forced_work(kind, K, G)
    work = torch.full((wl + 64,), NAN, dtype=torch.float64, device=dev)
    call(work.data_ptr(), wl)
    unwritten = int(torch.isnan(work[:wl]).sum().item())
    assert unwritten == 0, f"{what}: {unwritten} of {wl} workspace doubles not written (G = {G} did not run)"
    assert bool(torch.isnan(work[wl:]).all().item()), f"{what}: written past work_len"


def ptr_table(views, dev):
    return kn.upload_i64([v.data_ptr() for v in views], dev)


# ---- a. dist2 ---------------------------------------------------------------------

def _dist2(ptrs, K, ref, d_chunks, n, G, dev, what):
    out = torch.full((K,), NAN, dtype=torch.float64, device=dev)
    st = nat.stream_handle()
    run_forced(nat.WORK_DIST2, K, G, dev, lambda w, wl: nat.check(nat.lib().fedagg_dist2_f32(
        ptrs.data_ptr(), K, ref.data_ptr() if ref is not None else None, d_chunks.data_ptr(), n, out.data_ptr(),
        w, wl, st), what), what)
    return out.cpu().numpy()


@pytest.mark.parametrize("with_ref", [False, True])
@pytest.mark.parametrize("K", DIST2_KS)
def test_dist2_every_group_count(K, with_ref, dist_table, cuda_device):
    """64 clients are one pass of the client batches (cb), 65 and 129 start a
    second and third; row i starts i mod 4 elements past a 256-byte boundary
    and ref 1, 2 or 3, so load_chunk's per-pointer alignment is mixed."""
    dev = cuda_device
    tab, cols, d_chunks, L = dist_table
    n = len(tab)
    Gs = cg.STRIDE256_G
    rshift = 1 + DIST2_KS.index(K) % 3
    for kind in ("int", "gauss"):
        if kind == "int":
            rows, ref = cg.integer_rows(K, L, 10 + K, -8, 8), cg.integer_rows(1, L, 11 + K, -8, 8)[0]
        else:
            rows = cg.gaussian_rows(K, L, 12 + K)
            ref = (0.05 * np.random.default_rng(13 + K).standard_normal(L)).astype(np.float32)
        _, views = cg.shifted_rows(rows, [i % 4 for i in range(K)], dev)
        ptrs = ptr_table(views, dev)
        d_ref = None
        if with_ref:
            _, (d_ref,) = cg.shifted_rows(ref[None, :], [rshift], dev)
        else:
            ref = None
        want = cg.int_dist2(rows, ref, cols) if kind == "int" else cg.np_dist2(rows, ref, cols)
        for G in Gs:
            what = f"dist2 {kind} K={K} ref={with_ref} G={G}"
            got = _dist2(ptrs, K, d_ref, d_chunks, n, G, dev, what)
            if kind == "int":
                assert np.array_equal(bits64(got), bits64(want)), what
            else:
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=what)
                again = _dist2(ptrs, K, d_ref, d_chunks, n, G, dev, what)
                assert np.array_equal(bits64(got), bits64(again)), what


# ---- b. pairdist2 -----------------------------------------------------------------

def _pair(fn, kind, ptrs, K, d_chunks, n, G, dev, what):
    out = torch.full((K, K), NAN, dtype=torch.float64, device=dev)
    st = nat.stream_handle()
    run_forced(kind, K, G, dev, lambda w, wl: nat.check(fn(
        ptrs.data_ptr(), K, d_chunks.data_ptr(), n, out.data_ptr(), w, wl, st), what), what)
    return out.cpu().numpy()


@pytest.mark.parametrize("K", PAIR_KS)
def test_pairdist2_every_group_count(K, pair_table, cuda_device):
    """pairtri<16> (K <= 64), pairtri<32> (K <= 128) and the tiled kernel
    (T = 3 and 4 tiles a side).  K = 25 .. 40 has a wave that stages rows but
    owns no 4 x 4 block.  Any lost, doubled or mis-assigned column, stage,
    pair or partial shows as a nonzero integer."""
    dev = cuda_device
    tab, cols, d_chunks, L = pair_table
    n = len(tab)
    fn = nat.lib().fedagg_pairdist2_f32
    Gs = cg.QUARTERED_G
    shifts = [i % 4 for i in range(K)]

    rows = cg.integer_rows(K, L, 20 + K, -8, 8)
    _, views = cg.shifted_rows(rows, shifts, dev)
    ptrs = ptr_table(views, dev)
    want = cg.int_pair(rows, cols)
    for G in Gs:
        what = f"pairdist2 int K={K} G={G}"
        D = _pair(fn, nat.WORK_PAIRDIST2, ptrs, K, d_chunks, n, G, dev, what)
        assert np.array_equal(bits64(D), bits64(want)), (what, np.argwhere(D != want)[:8].tolist())
        assert (np.diag(D) == 0).all() and np.array_equal(D, D.T), what

    rows = cg.gaussian_rows(K, L, 21 + K, outliers=[0] if K > 2 else [])
    _, views = cg.shifted_rows(rows, shifts, dev)
    ptrs = ptr_table(views, dev)
    want = cg.np_pair(rows, cols)
    first = None
    for G in Gs:
        what = f"pairdist2 gauss K={K} G={G}"
        D = _pair(fn, nat.WORK_PAIRDIST2, ptrs, K, d_chunks, n, G, dev, what)
        assert (np.abs(D - want) <= 2.0 ** -18 * want).all(), (what, (np.abs(D - want) / np.maximum(want, 1e-300)).max())
        assert (np.diag(D) == 0).all() and np.array_equal(D, D.T), what
        if first is None:
            first = D
        assert (np.abs(D - first) <= 1e-12 * first).all(), what


# ---- c. pairgram2 -----------------------------------------------------------------

@pytest.mark.parametrize("K", GRAM_KS)
def test_pairgram2_every_group_count(K, pair_table, cuda_device):
    """Every build NB = 1 .. 8 with a full and a partial last group.  G = 1
    streams the whole table through the mid-stream folds; at G = 36 blocks
    30 .. 34 own two one-stage chunks, a stream of exactly 2 stages."""
    dev = cuda_device
    tab, cols, d_chunks, L = pair_table
    n = len(tab)
    fn = nat.lib().fedagg_pairgram2_f32
    rows = cg.gaussian_rows(K, L, 100 + K, outliers=[0] if K > 2 else [])
    _, views = cg.shifted_rows(rows, [i % 4 for i in range(K)], dev)
    ptrs = ptr_table(views, dev)
    want = cg.np_pair(rows, cols)
    X = rows[:, cols].astype(np.float64)
    C = X - X.mean(axis=0)[None, :]
    nrm = (C * C).sum(axis=1)
    scale = nrm[:, None] + nrm[None, :]
    worst = 0.0
    for G in cg.QUARTERED_G:
        what = f"pairgram2 K={K} G={G}"
        D = _pair(fn, nat.WORK_PAIRGRAM, ptrs, K, d_chunks, n, G, dev, what)
        if K > 1:
            worst = max(worst, float((np.abs(D - want) / scale).max()))
        assert (np.abs(D - want) <= 2e-6 * scale + 1e-300).all(), (what, worst)
        assert (np.diag(D) == 0).all() and (D >= 0).all() and np.array_equal(D, D.T), what
    print(f"GRAM_RATIO K={K} {worst:.3e}")


@pytest.mark.parametrize("K", GRAM_EXACT_KS)
def test_pairgram2_exact_on_small_integers(K, pair_table, cuda_device):
    """Entries in {-1, 0, 1}, K a power of two: the centred values are
    multiples of 1/K with at most 8 significant bits (h = c, m = l = 0), every
    fp32 accumulator over <= 256 columns is exact, and so are the fp64 folds
    and M_ii + M_jj - (M_ij + M_ji): the Gram equals the integer reference bit
    for bit, whichever stages a fold joins (test_chunk_groups.py emulates it)."""
    dev = cuda_device
    tab, cols, d_chunks, L = pair_table
    rows = cg.integer_rows(K, L, 300 + K, -1, 1)
    _, views = cg.shifted_rows(rows, [i % 4 for i in range(K)], dev)
    ptrs = ptr_table(views, dev)
    want = cg.int_pair(rows, cols)
    for G in cg.QUARTERED_G:
        what = f"pairgram2 exact K={K} G={G}"
        D = _pair(nat.lib().fedagg_pairgram2_f32, nat.WORK_PAIRGRAM, ptrs, K, d_chunks, len(tab), G, dev, what)
        assert np.array_equal(bits64(D), bits64(want)), (what, np.argwhere(D != want)[:8].tolist())


# ---- d. wsum_dist2 ----------------------------------------------------------------

@pytest.mark.parametrize("K", WSUM_KS)
def test_wsum_dist2_every_group_count(K, dist_table, cuda_device):
    """Both the FULL and the partial build of every tier KMAX = 8 .. 128."""
    dev = cuda_device
    tab, cols, d_chunks, L = dist_table
    n = len(tab)
    rows, w32 = client_rows(K, L, 40 + K)   # a column of -0, denormals
    outside = np.setdiff1d(np.arange(L), cols)
    zr = geomed_ref.chain(rows, w32)
    st = nat.stream_handle()
    for shift in (0, 1):
        _, views = cg.shifted_rows(rows, [shift] * K, dev)
        ptrs = ptr_table(views, dev)
        for host_w in (False, True):
            d_w = kn.HostWeights([float(v) for v in w32]) if host_w else torch.from_numpy(w32).to(dev)
            zw = torch.empty(L + 64, dtype=torch.float32, device=dev)   # fedagg_wsum_f32 on the same inputs
            kn.wsum_ptrs(torch.float32, ptrs, d_w, K, L, zw[shift:shift + L], shift == 0)
            zw = zw[shift:shift + L].cpu().numpy()
            for G in cg.STRIDE256_G:
                what = f"wsum_dist2 K={K} shift={shift} host_w={host_w} G={G}"
                zbuf = torch.full((L + 64,), GUARD, dtype=torch.float32, device=dev)
                z = zbuf[shift:shift + L]
                flags = (nat.FEDAGG_ALIGNED16 if z.data_ptr() % 16 == 0 else 0) | (nat.FEDAGG_HOST_WEIGHTS if host_w else 0)
                Ds = []
                for _ in range(2):
                    out = torch.full((K,), NAN, dtype=torch.float64, device=dev)
                    run_forced(nat.WORK_WSUM_DIST2, K, G, dev, lambda w, wl: nat.check(
                        nat.lib().fedagg_wsum_dist2_f32(ptrs.data_ptr(), d_w.data_ptr(), K, d_chunks.data_ptr(), n,
                                                        z.data_ptr(), out.data_ptr(), w, wl, flags, st), what), what)
                    Ds.append(out.cpu().numpy())
                zb = zbuf.cpu().numpy()
                zz = zb[shift:shift + L]
                assert np.array_equal(bits32(zz[cols]), bits32(zr[cols])), what   # the numpy chain, hence every G alike
                assert np.array_equal(bits32(zz[cols]), bits32(zw[cols])), what   # fedagg_wsum_f32
                assert (zz[outside] == GUARD).all() and (zb[:shift] == GUARD).all() and \
                    (zb[shift + L:] == GUARD).all(), what
                np.testing.assert_allclose(Ds[0], geomed_ref.dist2(rows, zz, cols), rtol=1e-12, atol=0, err_msg=what)
                assert np.array_equal(bits64(Ds[0]), bits64(Ds[1])), what


# ---- e. clip_diff / scale_diff ----------------------------------------------------

DIVS = [1.0, 1.5, 3.0000002, 0.25, 1e-3]
SRC_SPECIALS = [0.0, -0.0, 1e-42, -1e-45, 3e-39, float("inf"), -float("inf"), NAN]
REF_SPECIALS = [-0.0, 1e-41, float("inf"), NAN, 0.0]


def _clip_inputs(K, N, seed):
    rng = np.random.default_rng(seed)
    x = (0.05 * rng.standard_normal((1, N)) + 0.01 * rng.standard_normal((K, N))).astype(np.float32)
    r = (0.05 * rng.standard_normal(N)).astype(np.float32)
    for k, v in enumerate(SRC_SPECIALS):
        for base in (0, max(0, N - 40)):          # the first tile's head and the last tile's tail
            x[k % K, (base + 3 * k) % N] = v
            x[(k + 1) % K, (base + 3 * k + 1) % N] = v   # ... and against a special reference column
    for k, v in enumerate(REF_SPECIALS):
        for base in (0, max(0, N - 40)):
            r[(base + 3 * k + 1) % N] = v
    x[K - 1, N - 1] = float("inf")
    return x, r


def _check_clip(K, N, case, dev):
    x, r = _clip_inputs(K, N, 1000 * K + N)
    divs = [DIVS[(i + case) % len(DIVS)] for i in range(K)]
    sshift, dshift, rshift = cg.clip_shifts(K, case)
    _, src = cg.shifted_rows(x, sshift, dev)
    _, (d_ref,) = cg.shifted_rows(r[None, :], [rshift], dev)
    d_div = kn.upload_f32(divs, dev)
    sp = ptr_table(src, dev)
    for name, fn, ref_fn in (("clip", nat.lib().fedagg_clip_diff_f32, cg.np_clip),
                             ("scale", nat.lib().fedagg_scale_diff_f32, cg.np_scale)):
        what = f"{name} K={K} N={N}"
        dbuf, dst = cg.shifted_rows(np.full((K, N), GUARD, np.float32), dshift, dev, fill=GUARD)
        dp = ptr_table(dst, dev)
        nat.check(fn(sp.data_ptr(), K, d_ref.data_ptr(), d_div.data_ptr(), N, dp.data_ptr(), nat.stream_handle()), what)
        got = dbuf.cpu().numpy()
        for i in range(K):
            s = dshift[i]
            want = ref_fn(x[i], r, divs[i])
            y = got[i, s:s + N]
            wn = np.isnan(want)
            assert np.array_equal(np.isnan(y), wn), f"{what} row {i}: NaN positions"
            bad = np.flatnonzero((bits32(y) != bits32(want)) & ~wn)
            assert bad.size == 0, f"{what} row {i} (div {divs[i]}): columns {bad[:8].tolist()}"
            assert (got[i, :s] == GUARD).all() and (got[i, s + N:] == GUARD).all(), f"{what} row {i}: guard"


@pytest.mark.parametrize("K", CLIP_KS)
def test_clip_and_scale_small_shapes(K, cuda_device):
    """K mod 8 in 1 .. 4 leaves a wave its "last < CU clients" loop; N around
    the 1,024-column tile and the 4-column vector; source, destination and
    reference rows each at their own alignment; +-0, denormals, +-inf and NaN
    among the inputs; a divisor of 1 (the skipped division) among the rest."""
    for j, N in enumerate(CLIP_NS):
        _check_clip(K, N, CLIP_KS.index(K) * len(CLIP_NS) + j, cuda_device)


def test_clip_and_scale_second_round_of_tiles(cuda_device):
    """2,050 tiles against the grid's 2,048 blocks: blocks 0 and 1 take a
    second tile (t += G), the last one a single ragged column."""
    _check_clip(3, 2048 * 1024 + 1025, 7, cuda_device)
