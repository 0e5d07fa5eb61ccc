"""fedagg_nearmedian_mean_wide_f32 (Bulyan's stage 2 for 129 to 1024 selected
clients, the column spread over 4 or 8 lanes) on the GPU, bit for bit against
the two-pointer reference (tests/bulyan_ref.py): every tier in its full and
padded form at column counts on both sides of a wave's and a block's last
column, at the keeps where the partner changes lane; the one-lane-per-column
kernel as an independent cross-check up to 128 rows; window starts planted at
every lane boundary, exact ties, NaN / inf / zero columns; and bulyan()'s
dispatch and end-to-end result."""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bulyan_ref as br
import trimmed_mean_ref as tmr
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn

pytestmark = pytest.mark.gpu

KS = [129, 130, 200, 255, 256, 257, 300, 511, 512, 513, 700, 1023, 1024]
# a wave holds 16 or 8 columns and a block 64 or 32
N_LIST = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1031)
GUARD = 8  # output elements past the last column, which no launch may write
INF, NAN = br.INF, br.NAN


def _tier(K: int):
    """(P, R) of the kernel tier holding K rows."""
    return (4, 64) if K <= 256 else (4, 128) if K <= 512 else (8, 128)


def _keeps(K: int) -> list:
    """bulyan_ref.keeps(K), and R - 1, R, R + 1, 2R for the tier's R: where
    the partner `keep` ranks up changes lane and the in-lane shift is 0 or
    R - 1."""
    R = _tier(K)[1]
    out = br.keeps(K)
    for k in (R - 1, R, R + 1, 2 * R):
        if 1 <= k <= K and k not in out:
            out.append(k)
    return out


class _Placed:
    """The (K, N) CPU values once on the device, as strided rows of one
    buffer that start `offset` elements past a 256-byte boundary, with their
    pointer table: launches take prefixes of the columns and of the rows."""

    def __init__(self, vals: torch.Tensor, offset: int, dev):
        K, N = vals.shape
        self.K, self.N, self.offset, self.dev = K, N, offset, dev
        buf = torch.empty((K, (N + offset + 127) // 128 * 128), dtype=torch.float32, device=dev)
        self.rows = buf[:, offset:offset + N]
        self.rows.copy_(vals)
        base, step = self.rows.data_ptr(), buf.stride(0) * buf.element_size()
        self.addr = [base + i * step for i in range(K)]
        self.ptrs = kn.upload_i64(self.addr, dev)

    def table(self, order):
        return kn.upload_i64([self.addr[i] for i in order], self.dev)

    def launch(self, n: int, keep: int, fn=None, K: "int | None" = None, ptrs=None) -> torch.Tensor:
        """fn (default: the wide kernel) on the first K rows' first n columns."""
        out = torch.full((n + self.offset + GUARD,), 7.0, dtype=torch.float32, device=self.dev)[self.offset:]
        (fn or dfn.nearmedian_mean_rows_wide)(self.ptrs if ptrs is None else ptrs, self.K if K is None else K, n,
                                              keep, out)
        got = out.cpu()
        assert bool((got[n:] == 7.0).all()), "wrote past the last column"
        return got[:n]


@functools.lru_cache(maxsize=None)
def _kernel_case(K: int):
    """The rows of a kernel case and the reference per keep, shared by the
    aligned and the offset form."""
    x = tmr.make_rows(K, max(N_LIST), torch.float32, seed=5000 + K)
    x[0, 50], x[1, 51], x[2, 52] = NAN, INF, -INF
    return x, {keep: br.nearmedian_mean_ref(x, keep) for keep in _keeps(K)}


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("K", KS)
def test_kernel_matches_reference(K, offset, cuda_device):
    x, refs = _kernel_case(K)
    placed = _Placed(x, offset, cuda_device)
    for keep, ref in refs.items():
        for N in N_LIST:  # columns are independent: a prefix of the rows gives a prefix
            tmr.assert_same(placed.launch(N, keep), ref[:N], f"K={K} keep={keep} N={N} offset={offset}")


def test_equals_the_narrow_kernel_below_129_rows(cuda_device):
    """Small K pads into the 256 tier: the one-lane-per-column kernel is an
    independent implementation of the same specification."""
    N = 300
    x = tmr.make_rows(128, N, torch.float32, seed=43)
    x[0, 50], x[1, 51], x[2, 52] = NAN, INF, -INF
    placed = _Placed(x, 0, cuda_device)
    for K in (1, 2, 3, 8, 65, 128):  # the first K rows
        for keep in br.keeps(K):
            got = placed.launch(N, keep, K=K)
            tmr.assert_same(got, placed.launch(N, keep, fn=dfn.nearmedian_mean_rows, K=K), f"K={K} keep={keep} narrow")
            tmr.assert_same(got, br.nearmedian_mean_ref(x[:K], keep), f"K={K} keep={keep} reference")


@pytest.mark.parametrize("K", [130, 512, 1024])
def test_keep_all_is_the_trimmed_mean_at_trim_zero(K, cuda_device):
    x = tmr.make_rows(K, 300, torch.float32, seed=45 + K)
    x[0, 60], x[1, 61], x[2, 62] = NAN, INF, -INF
    x[0, 63], x[1, 63] = INF, -INF
    placed = _Placed(x, 0, cuda_device)
    got = placed.launch(300, K)
    tmr.assert_same(got, placed.launch(300, 0, fn=dfn.trimmed_mean_rows_wide), f"K={K} wide trimmed mean")
    tmr.assert_same(got, tmr.trimmed_mean_ref(x, 0), f"K={K} reference")


# ---- planted window starts ------------------------------------------------------

FAR = 10000.0  # farther from the median than any value inside a planted window


def _window_bounds(K: int, keep: int):
    r = (K - 1) // 2
    return r, max(0, r - keep + 1), min(r, K - keep)


def _start_targets(K: int, keep: int) -> list:
    """Window starts: lo_min, lo_min + 1, lo_max - 1, lo_max; around every lane
    boundary b in [lo_min, lo_max] the last rank of the lane below and b
    itself; and for every lane boundary b the start b - keep whose window ends
    exactly at b."""
    R = _tier(K)[1]
    r, lo_min, lo_max = _window_bounds(K, keep)
    want = [lo_min, lo_min + 1, lo_max - 1, lo_max]
    for b in range(0, K + R, R):
        want += [b - 1, b, b - keep, b - keep - 1, b - keep + 1]
    return sorted({lo for lo in want if lo_min <= lo <= lo_max})


def _sorted_column(K: int, keep: int, lo: int) -> np.ndarray:
    """Distinct ascending values whose window is [lo, lo + keep): the ranks
    inside are the integers rank - r (the median is 0), every other rank lies
    FAR beyond them."""
    r = (K - 1) // 2
    j = np.arange(K, dtype=np.float64)
    s = j - r
    s[:lo] -= FAR
    s[lo + keep:] += FAR
    return s.astype(np.float32)


def _chain(vals: np.ndarray) -> np.float32:
    """fl32(fl32(.. fl32(v0 + v1) ..) / fl32(len)): the specification's sum and division."""
    acc = np.float32(vals[0])
    for v in vals[1:]:
        acc = np.float32(acc + np.float32(v))
    return np.float32(acc / np.float32(len(vals)))


@functools.lru_cache(maxsize=None)
def _planted_case(K: int, keep: int):
    """(x, ref, wanted windows): one column per target start, then per start
    lo < lo_max two columns that decide lo against lo + 1 at the last step: the
    lowest value of the window and the value it would gain exactly equidistant
    from the median (the tie goes left: lo), and the gained value one ulp
    nearer (lo + 1).  Every column's rows are shuffled."""
    r, lo_min, lo_max = _window_bounds(K, keep)
    cols, windows = [], []
    for lo in _start_targets(K, keep):
        cols.append(_sorted_column(K, keep, lo))
        windows.append(lo)
    for lo in [t for t in _start_targets(K, keep) if t < lo_max]:
        for right, start in ((np.float32(2.0), lo), (np.nextafter(np.float32(2.0), np.float32(0)), lo + 1)):
            s = _sorted_column(K, keep - 1, lo + 1).astype(np.float64)  # ranks lo+1 .. lo+keep-1 inside
            s[lo + 1:lo + keep] /= 1024.0  # all of them nearer than 1
            s[lo], s[lo + keep] = -2.0, right
            s = s.astype(np.float32)
            assert bool(np.all(np.diff(s) > 0)), (K, keep, lo)
            cols.append(s)
            windows.append(start)
    rng = np.random.default_rng(K * 1000 + keep)
    x = np.stack([c[rng.permutation(K)] for c in cols], axis=1)
    sx = np.sort(x, axis=0)
    ref = br.nearmedian_mean_ref(torch.from_numpy(x), keep)
    # the inputs do what they claim: the reference averages the intended ranks
    want = torch.from_numpy(np.array([_chain(sx[lo:lo + keep, c]) for c, lo in enumerate(windows)], dtype=np.float32))
    assert not bool(torch.isnan(ref).any())
    assert torch.equal(tmr.bits(ref), tmr.bits(want)), (K, keep)
    return torch.from_numpy(x), ref, windows


PLANTED = [(K, keep) for K in (256, 200, 512, 384, 1024, 700) for keep in (int(0.4 * K), int(0.78 * K))]


@pytest.mark.parametrize("K,keep", PLANTED, ids=[f"K{K}-keep{k}" for K, k in PLANTED])
def test_planted_window_starts(K, keep, cuda_device):
    R = _tier(K)[1]
    r, lo_min, lo_max = _window_bounds(K, keep)
    x, ref, windows = _planted_case(K, keep)
    assert {lo_min, lo_max} <= set(windows) and lo_max - lo_min >= 2
    assert any(lo % R == 0 and lo for lo in windows) or any((lo + keep) % R == 0 for lo in windows), windows
    tmr.assert_same(_Placed(x, 0, cuda_device).launch(x.shape[1], keep), ref, f"K={K} keep={keep} starts {windows}")


@pytest.mark.parametrize("K,keep", [(130, 100), (1024, 600)])
def test_planted_specials(K, keep, cuda_device):
    N, c0 = 128, 100
    r = (K - 1) // 2
    assert r + 2 <= keep <= K - 2 and keep // 2 <= r
    x = tmr.make_rows(K, N, torch.float32, seed=277 + K)
    n = K - keep  # lo_min = 0: with every distance tied the window is [0, keep)
    x[:, c0], x[:, c0 + 1] = 0.25, 0.25
    x[1:1 + n, c0] = NAN  # the window stops one rank short of the first NaN
    x[1:2 + n, c0 + 1] = NAN  # one more: it touches it
    x[:K - r, c0 + 2] = INF  # m = +inf
    x[:K - r, c0 + 3] = NAN  # m a NaN: more than half the column
    # -inf, keep - 2 ones (m among them), K - keep + 1 +inf: the ones go first,
    # then the tie of the two infinities goes left, then right is all that is
    # left: a kept +inf with a kept -inf
    x[:, c0 + 4] = 1.0
    x[0, c0 + 4] = -INF
    x[keep - 1:, c0 + 4] = INF
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    x[:, c0 + 5] = perm.float() - r  # the integers -r .. K-1-r: symmetric about m = 0
    x[:, c0 + 6] = -0.0  # an all -0 window stays -0
    x[:, c0 + 7] = 0.3
    x[3:3 + n, c0 + 8] = NAN  # the same two NaN counts among random values
    x[3:4 + n, c0 + 9] = NAN
    # +-0 around the median, one value of each sign beyond them
    x[:r, c0 + 10], x[r:, c0 + 10] = -0.0, 0.0
    x[0, c0 + 10], x[K - 1, c0 + 10] = -5.0, 5.0
    x[:3, c0 + 11], x[K - 3:, c0 + 11] = -INF, INF  # infinities at both ends of a random column
    x[:r + 1, c0 + 12] = -INF  # m = -inf
    # NaNs spread over the lanes' first slots (as clients), among random values
    heads = [p * _tier(K)[1] for p in range(_tier(K)[0]) if p * _tier(K)[1] < K]
    x[heads, c0 + 13] = NAN
    ref = br.nearmedian_mean_ref(x, keep)
    assert ref[c0].item() == 0.25 and bool(torch.isnan(ref[c0 + 1]))
    assert ref[c0 + 2].item() == INF
    assert bool(torch.isnan(ref[c0 + 3])) and bool(torch.isnan(ref[c0 + 4]))
    # symmetric about m: with an even keep the odd last step is a tie, which goes left
    assert ref[c0 + 5].item() == (-0.5 if keep % 2 == 0 else 0.0)
    assert ref[c0 + 6].item() == 0 and bool(torch.signbit(ref[c0 + 6]))
    assert ref[c0 + 7].item() == pytest.approx(0.3, rel=1e-3)  # a chain of up to 600 fp32 adds
    assert bool(torch.isnan(ref[c0 + 9]))
    assert ref[c0 + 10].item() == 0 and ref[c0 + 12].item() == -INF
    assert torch.nonzero(torch.isnan(ref[:c0])).numel() == 0
    placed = _Placed(x, 0, cuda_device)
    got = placed.launch(N, keep)
    tmr.assert_same(got, ref, f"K={K} keep={keep}")
    assert int(tmr.bits(got)[c0 + 6]) == int(tmr.bits(torch.tensor([-0.0]))[0])
    # a window that reaches the planted infinities and NaNs at the ends
    tmr.assert_same(placed.launch(N, K - 1), br.nearmedian_mean_ref(x, K - 1), f"K={K} keep={K - 1}")


@pytest.mark.parametrize("K", [300, 1024])
def test_row_order_does_not_matter(K, cuda_device):
    x = tmr.make_rows(K, 300, torch.float32, seed=65 + K)
    x[0, 60], x[1, 61], x[2, 62] = NAN, INF, -INF
    placed = _Placed(x, 0, cuda_device)
    g = torch.Generator().manual_seed(K)
    for keep in br.keeps(K):
        a = placed.launch(300, keep)
        b = placed.launch(300, keep, ptrs=placed.table(torch.randperm(K, generator=g).tolist()))
        tmr.assert_same(b, a, f"K={K} keep={keep}")


# ---- bulyan(): dispatch and end to end ------------------------------------------

ROW_FUNCTIONS = ("nearmedian_mean_rows", "nearmedian_mean_rows_wide", "nearmedian_mean_rows_torch")


def _record(monkeypatch, ran: list):
    for name in ROW_FUNCTIONS:
        real = getattr(dfn, name)

        def f(*a, _real=real, _name=name, **kw):
            ran.append(_name)
            return _real(*a, **kw)

        monkeypatch.setattr(dfn, name, f)


def _two_keys(K: int, dev):
    x = tmr.make_rows(K, 200, torch.float32, seed=19 + K)
    x[5, 70], x[6, 71], x[7, 72] = NAN, INF, -INF
    count = 100 + 7 * torch.arange(K, dtype=torch.int64)
    xd, cd = x.to(dev), count.to(dev)
    return x, count, [(1, OrderedDict(w=xd[i], n=cd[i])) for i in range(K)]


@pytest.mark.parametrize("K", [128, 129, 1024, 1025])
def test_dispatch(K, cuda_device, monkeypatch):
    """f = 0 needs no distances and selects every client, so theta = beta = K:
    up to 128 the narrow kernel, 129 to 1024 the wide one in a tier that
    NEARMEDIAN_WIDE_AUTO holds True and the torch path in one it holds False,
    above 1024 the torch path."""
    x, count, raw = _two_keys(K, cuda_device)
    # stage 2 of bulyan_ref over every client (bulyan_ref itself also builds the
    # K x K distances in Python loops, which f = 0 never looks at)
    want_w = br.nearmedian_mean_ref(x, K)
    want_n = br.nearmedian_mean_ref(count.float().reshape(K, 1), K)
    if K <= 129:
        ref, selected, _, _ = br.bulyan_ref([(1, OrderedDict(w=x[i], n=count[i])) for i in range(K)], 0)
        assert selected == list(range(K))
        tmr.assert_same(ref["w"], want_w, "reference w")
        tmr.assert_same(ref["n"].reshape(1), want_n, "reference n")
    assert bool(torch.isnan(want_w[70])) and int(torch.isnan(want_w).sum()) == 1
    ran = []
    _record(monkeypatch, ran)
    for table, path in (({256: True, 512: True, 1024: True}, "nearmedian_mean_rows_wide"),
                        ({256: False, 512: False, 1024: False}, "nearmedian_mean_rows_torch")):
        monkeypatch.setattr(dfn, "NEARMEDIAN_WIDE_AUTO", table)
        del ran[:]
        out, info = dfn.bulyan(raw, 0, return_info=True)
        expect = "nearmedian_mean_rows" if K <= 128 else path if K <= 1024 else "nearmedian_mean_rows_torch"
        assert ran == [expect], (K, table, ran)
        assert (info.theta, info.beta, info.selected) == (K, K, list(range(K)))
        assert list(out) == ["w", "n"]
        assert out["w"].is_cuda and out["w"].dtype == torch.float32 and out["w"].shape == (200,)
        tmr.assert_same(out["w"], want_w, f"K={K} {expect}")
        assert out["n"].dtype == torch.float32 and out["n"].shape == ()
        tmr.assert_same(out["n"].reshape(1), want_n, f"K={K} counter {expect}")


def test_dispatch_takes_the_tier_of_theta(cuda_device, monkeypatch):
    """One tier False, the others True: theta = 300 follows the 512 entry."""
    _, _, raw = _two_keys(300, cuda_device)
    ran = []
    _record(monkeypatch, ran)
    monkeypatch.setattr(dfn, "NEARMEDIAN_WIDE_AUTO", {256: True, 512: False, 1024: True})
    dfn.bulyan(raw, 0)
    monkeypatch.setattr(dfn, "NEARMEDIAN_WIDE_AUTO", {256: False, 512: True, 1024: False})
    dfn.bulyan(raw, 0)
    assert ran == ["nearmedian_mean_rows_torch", "nearmedian_mean_rows_wide"]


K_E2E, F_E2E = 140, 3


@pytest.fixture(scope="module")
def e2e_reference():
    """134 clients in a tight cluster, three at three times their spread and
    three far away: in every round the six score worse than any other client,
    so the selected SET is pinned (the pick order among 134 i.i.d. clients is
    not: some round's two lowest scores are bound to be close)."""
    K, f, N = K_E2E, F_E2E, 300
    spread = [0.05] * 134 + [0.15] * 3 + [5.0] * 3
    g = torch.Generator().manual_seed(11)
    centre = torch.randn(N, generator=g)
    x = torch.stack([centre + spread[i] * torch.randn(N, generator=g) for i in range(K)])
    # NaN and infinities where the distances do not look: a BatchNorm statistic
    y = tmr.make_rows(K, 64, torch.float32, seed=12)
    y[5, 50], y[9, 51], y[11, 52] = NAN, INF, -INF
    y[20:27, 53] = NAN  # more than theta - beta of them: the window reaches a NaN
    host = [(1, OrderedDict([("w", x[i].clone()), ("bn.running_mean", y[i].clone())])) for i in range(K)]
    ref, selected, _, D = br.bulyan_ref(host, f)
    assert set(selected) == set(range(134)) and len(selected) == 134 > dfn.NEARMEDIAN_MAX_CLIENTS
    # the set survives distances moved by 1e-5 relative, a hundred times the
    # kernel's error (symmetric, as the kernel's matrix is)
    e = np.random.default_rng(1).uniform(-1e-5, 1e-5, size=D.shape)
    assert set(br.bulyan_select_ref(D * (1 + np.triu(e, 1) + np.triu(e, 1).T), f)[0]) == set(selected)
    assert bool(torch.isnan(ref["bn.running_mean"][53])) and not bool(torch.isnan(ref["bn.running_mean"][50]))
    return host, ref, selected


@pytest.mark.parametrize("device_inputs", [False, True], ids=["host", "device"])
def test_end_to_end_with_byzantine_clients(device_inputs, e2e_reference, cuda_device, monkeypatch):
    """K = 140, f = 3: theta = 134 rows, beta = 128, through the wide kernel."""
    host, ref, selected = e2e_reference
    raw = host
    if device_inputs:
        raw = [(n, OrderedDict((k, t.to(cuda_device)) for k, t in d.items())) for n, d in host]
    ran = []
    _record(monkeypatch, ran)
    monkeypatch.setattr(dfn, "NEARMEDIAN_WIDE_AUTO", {256: True, 512: True, 1024: True})
    out, info = dfn.bulyan(raw, F_E2E, cuda_device, method="exact", return_info=True)
    assert ran == ["nearmedian_mean_rows_wide"]
    assert set(info.selected) == set(selected) and (info.theta, info.beta) == (134, 128)
    for k in ("w", "bn.running_mean"):
        assert out[k].is_cuda == device_inputs and out[k].dtype == torch.float32
        tmr.assert_same(out[k], ref[k], f"K={K_E2E} {k}")
