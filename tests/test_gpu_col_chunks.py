"""The later launches of launch_col_chunks (csrc/sortnet.h) at small shapes.

A call of more than kColsChunk = 2^30 columns runs its launches after the
first on other kernels than every other test reaches: the OFF = true
instantiations of the padded median_kernel, median_pk16_kernel,
trimmed_mean_kernel and nearmedian_mean_kernel (62 kernels; row_base(p, col0),
pads read at their own address, the 16-bit NaN re-read through row_base, and
the padded form at K == KMAX).  FEDAGG_COLS_CHUNK = 130 makes the same shipped
kernels run on a few hundred columns: even, no multiple of the 64-lane wave,
so every launch ends in a partly filled wave and every later one starts
mid-line.  Every result is compared bit for bit over every column with the
references of the other GPU tests (the oracle's lower median, the numpy trimmed
mean, the two-pointer nearest-to-median mean); the output is filled with a
sentinel and 64 guard elements past N (and the element before an unaligned
output) must stay untouched."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import bulyan_ref as br
import golden_util as gu
import trimmed_mean_ref as tmr
from fedml_amd import defense as dfn
from fedml_amd import kernels as kn
from oracle import fedavg_oracle as orc

pytestmark = pytest.mark.gpu

C = 130  # columns per launch
N_ALL = 3 * C + 38  # the rows are built once at this length; columns are independent, so a prefix gives a prefix
# one launch (the control); an offset launch of one column (the packed kernel's
# lone last column); an exact end; three offset launches with an odd and an
# even ragged end
NS = [C, C + 1, 2 * C, 3 * C + 37, 3 * C + 38]
GUARD = 64
STRIDE = 512  # elements from row to row: 1 KiB or 2 KiB, aligned rows as bucket rows are
SENTINEL = 7.0  # no result here: the medians lie in [-6.25, 6.125], the means near 0, 0.25 or at an infinity
# every tier at its smallest and largest K (K == tier: the full kernel on the
# first chunk, the padded offset kernel at K == KMAX on the rest), 3 and 127
KS = [1, 3, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 127, 128]
KS_PACKED = [1, 3, 32, 33, 64, 65, 96]  # the tiers of median_pk16_kernel
KS_16BIT = [3, 8, 33, 96, 128]
DT_IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
INF, NAN = float("inf"), float("nan")


@pytest.fixture(autouse=True)
def small_chunk(monkeypatch):
    monkeypatch.setenv("FEDAGG_COLS_CHUNK", str(C))


def _ibits(x: torch.Tensor) -> torch.Tensor:
    """A writable integer view of a contiguous CPU tensor's bits."""
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _nan_bits(dtype, negative: bool) -> int:
    """A quiet NaN of either sign, as the signed integer of the dtype's width."""
    pos = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}[dtype]
    return -1 if negative else pos  # all ones: a quiet NaN with the sign set


class _Rows:
    """The rows of CPU tensor x (K, N_ALL) on the device, `offset` elements
    off their aligned row starts (1: rows and output aligned to nothing beyond
    their element); NaN fills the rest of every row's stride."""

    def __init__(self, x: torch.Tensor, dev, offset: int = 0):
        self.K, n = x.shape
        assert n == N_ALL and offset + n <= STRIDE
        self.dev, self.offset, self.dtype = dev, offset, x.dtype
        self.buf = torch.full((self.K, STRIDE), NAN, dtype=x.dtype, device=dev)
        self.buf[:, offset:offset + n] = x.to(dev)
        es = self.buf.element_size()
        self.ptrs = kn.upload_i64([self.buf.data_ptr() + (i * STRIDE + offset) * es for i in range(self.K)], dev)

    def run(self, launch, N: int) -> torch.Tensor:
        """launch(ptrs, K, N, out) over the first N columns -> out on the CPU."""
        full = torch.full((self.offset + N + GUARD,), SENTINEL, dtype=self.dtype, device=self.dev)
        out = full[self.offset:self.offset + N]
        # what median_rows' aligned flag needs, or the packed kernel is silently not the one run
        assert self.offset or (out.data_ptr() % 16 == 0 and self.buf.data_ptr() % 16 == 0)
        launch(self.ptrs, self.K, N, out)
        torch.cuda.synchronize(self.dev)
        full = full.cpu()
        edge = torch.cat([full[:self.offset], full[self.offset + N:]])
        assert torch.equal(tmr.bits(edge), tmr.bits(torch.full_like(edge, SENTINEL))), \
            f"N={N}: written outside the output at {torch.nonzero(edge != SENTINEL).flatten()[:5].tolist()}"
        return full[self.offset:self.offset + N].clone()


# ---- median -------------------------------------------------------------------

# client K // 2 holds a positive NaN and client K - 1 a negative one in
# overlapping columns: where both stand, the first in client order is pinned
MED_POS_NAN = [C - 1, C, C + 1, 173, 3 * C - 1, 3 * C, N_ALL - 1]
MED_NEG_NAN = [C, C + 1, C + 2, 176, 301, 3 * C, 3 * C + 1, N_ALL - 2, N_ALL - 1]
# 173, 176 and 301: a NaN in only one column of a packed pair
MED_POS_INF, MED_NEG_INF, MED_NEG_ZERO = [200, 2 * C - 1], [201, 2 * C], [202, 203, 2 * C + 1]


@functools.lru_cache(maxsize=None)
def _median_case(K: int, dtype):
    """(rows, reference, bits of every NaN column's first NaN); shared by the
    aligned and the offset run, never written to."""
    g = torch.Generator().manual_seed(7000 + K)
    x = (torch.randint(-50, 50, (K, N_ALL), generator=g).float() * 0.125).to(dtype)  # k / 8: exact in bf16 and f16
    x[:, MED_POS_INF], x[:, MED_NEG_INF], x[:, MED_NEG_ZERO] = INF, -INF, -0.0
    xi = _ibits(x)
    xi[K // 2, MED_POS_NAN] = _nan_bits(dtype, False)
    xi[K - 1, MED_NEG_NAN] = _nan_bits(dtype, True)  # K = 1: the one client, written last
    ref = torch.from_numpy(orc.lower_median_cols(x.float().numpy())).to(dtype)
    # the planted columns give what they were planted for
    nan_cols = sorted(set(MED_POS_NAN) | set(MED_NEG_NAN))
    assert torch.nonzero(torch.isnan(ref)).flatten().tolist() == nan_cols
    assert bool((ref[MED_POS_INF] == INF).all()) and bool((ref[MED_NEG_INF] == -INF).all())
    assert bool((ref[MED_NEG_ZERO] == 0).all()) and bool(torch.signbit(ref[MED_NEG_ZERO]).all())
    # the first NaN of every NaN column in client order, from the rows' own bits
    isn = torch.isnan(x[:, nan_cols]).numpy()
    first = torch.from_numpy(xi.numpy()[np.argmax(isn, axis=0), nan_cols])
    if K >= 3:  # two clients: the earlier one's NaN, sign and payload
        both = [nan_cols.index(c) for c in sorted(set(MED_POS_NAN) & set(MED_NEG_NAN))]
        only_neg = [nan_cols.index(c) for c in sorted(set(MED_NEG_NAN) - set(MED_POS_NAN))]
        assert len(both) == 4 and len(only_neg) == 5 and bool((first[both] == _nan_bits(dtype, False)).all())
        assert bool((first[only_neg] == -1).all())
    return x, ref, nan_cols, first


def _check_median(K, dtype, offset, aligned, dev):
    x, ref, nan_cols, first = _median_case(K, dtype)
    rows = _Rows(x, dev, offset)
    what = f"median K={K} {DT_IDS[dtype]} offset={offset} aligned={aligned}"
    for N in NS:
        got = rows.run(lambda p, k, n, out: dfn.median_rows(p, k, n, out, aligned=aligned), N)
        gu.assert_same(got, ref[:N], f"{what} N={N}")
        here = [i for i, c in enumerate(nan_cols) if c < N]
        got_nan = _ibits(got)[[nan_cols[i] for i in here]]
        assert torch.equal(got_nan, first[here]), \
            f"{what} N={N}: not the column's first NaN at {[nan_cols[i] for i in here]}: {got_nan.tolist()}"


@pytest.mark.parametrize("K", KS)
def test_median_f32(K, cuda_device):
    _check_median(K, torch.float32, 0, False, cuda_device)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
def test_median_16bit_rows_one_element_off(K, dtype, cuda_device):
    """The widening one-column kernel and its NaN re-read through row_base."""
    _check_median(K, dtype, 1, False, cuda_device)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("K", KS_PACKED)
def test_median_16bit_packed(K, dtype, cuda_device):
    """median_pk16_kernel: the chunk start keeps the 4-byte column pairs
    aligned, N = C + 1 is an offset launch of the lone last column."""
    _check_median(K, dtype, 0, True, cuda_device)


@pytest.mark.parametrize("K,dtype", [(100, torch.bfloat16), (100, torch.float16), (128, torch.bfloat16),
                                     (128, torch.float16), (129, torch.float32)],
                         ids=["K100-bf16", "K100-f16", "K128-bf16", "K128-f16", "K129-f32"])
def test_median_paths_that_do_not_chunk(K, dtype, cuda_device):
    """Controls: the variable is set, the bit-plane select (aligned 16-bit
    rows, 97 <= K <= 128) and the lane-group kernel (K > 128) launch once."""
    _check_median(K, dtype, 0, True, cuda_device)


def test_empty_value_is_unset_and_a_bad_one_raises(monkeypatch, cuda_device):
    x, ref, _, _ = _median_case(3, torch.float32)
    rows = _Rows(x, cuda_device)
    monkeypatch.setenv("FEDAGG_COLS_CHUNK", "")
    gu.assert_same(rows.run(dfn.median_rows, N_ALL), ref, "empty FEDAGG_COLS_CHUNK")
    monkeypatch.setenv("FEDAGG_COLS_CHUNK", "129")
    from fedml_amd import _native as nat

    with pytest.raises(nat.FedAggNativeError, match="FEDAGG_COLS_CHUNK"):
        rows.run(dfn.median_rows, N_ALL)


# ---- trimmed mean and nearest-to-median mean ------------------------------------

# the i-th trim / keep of a case plants its two NaN counts at PLANT_A[i] (the
# result stays finite) and PLANT_B[i] (one NaN more: NaN), on both sides of
# every chunk boundary, in the last two columns and inside chunk 2
PLANT_A = [(C - 1, 210), (C + 1, 212), (2 * C - 1, 214), (3 * C - 1, 216), (N_ALL - 2, 218)]
PLANT_B = [(C, 211), (C + 2, 213), (2 * C, 215), (3 * C, 217), (N_ALL - 1, 219)]
ROLL = C + 10  # make_rows' bands of zeros, ties and denormals (columns 0-47) move into chunk 2


def _base_rows(K: int, dtype, seed: int) -> torch.Tensor:
    return torch.roll(tmr.make_rows(K, N_ALL, dtype, seed=seed), ROLL, dims=1).contiguous()


def _plant_nans(x: torch.Tensor, col: int, count: int) -> None:
    K = x.shape[0]
    assert 0 <= count <= K
    x[[(1 + j) % K for j in range(count)], col] = NAN


TM_POS_INF, TM_NEG_INF, TM_BOTH_INF, TM_NEG_ZERO = [200, 2 * C + 1], [201, 2 * C + 2], [202, 2 * C + 3], [203, 3 * C + 1]


@functools.lru_cache(maxsize=None)
def _trimmed_case(K: int, dtype):
    """(rows, [(trim, reference)]); shared by the aligned and the offset run."""
    x = _base_rows(K, dtype, 8000 + K)
    trims = tmr.trims(K, extra=(K // 4,))
    assert len(trims) <= len(PLANT_A)
    for i, trim in enumerate(trims):
        for a, b in zip(PLANT_A[i], PLANT_B[i]):
            _plant_nans(x, a, trim)  # exactly trim NaNs: all trimmed
            _plant_nans(x, b, trim + 1)  # one more: NaN
    x[:, TM_POS_INF], x[:, TM_NEG_INF], x[:, TM_NEG_ZERO] = INF, -INF, -0.0
    x[0, TM_BOTH_INF], x[K - 1, TM_BOTH_INF] = INF, -INF  # K = 1: -inf alone
    refs = []
    for i, trim in enumerate(trims):
        ref = tmr.trimmed_mean_ref(x, trim)
        assert bool(torch.isfinite(ref[list(PLANT_A[i])].float()).all()), (K, trim)
        assert bool(torch.isnan(ref[list(PLANT_B[i])]).all()), (K, trim)
        assert bool((ref[TM_POS_INF] == INF).all()) and bool((ref[TM_NEG_INF] == -INF).all())
        assert bool((ref[TM_NEG_ZERO] == 0).all()) and bool(torch.signbit(ref[TM_NEG_ZERO]).all())
        if K >= 2:  # both kept: inf - inf; both trimmed: finite
            both = ref[TM_BOTH_INF].float()
            assert bool(torch.isnan(both).all()) if trim == 0 else bool(torch.isfinite(both).all()), (K, trim)
        refs.append((trim, ref))
    return x, refs


def _check_trimmed(K, dtype, offset, dev):
    x, refs = _trimmed_case(K, dtype)
    rows = _Rows(x, dev, offset)
    for trim, ref in refs:
        for N in NS:
            got = rows.run(lambda p, k, n, out: dfn.trimmed_mean_rows(p, k, n, trim, out), N)
            tmr.assert_same(got, ref[:N], f"trimmed mean K={K} trim={trim} N={N} {DT_IDS[dtype]} offset={offset}")


@pytest.mark.parametrize("K", KS)
def test_trimmed_mean_f32(K, cuda_device):
    _check_trimmed(K, torch.float32, 0, cuda_device)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("K", KS_16BIT)
def test_trimmed_mean_16bit(K, dtype, offset, cuda_device):
    _check_trimmed(K, dtype, offset, cuda_device)


@functools.lru_cache(maxsize=None)
def _nearmedian_case(K: int):
    """(rows, [(keep, reference)]).  The two NaN counts of
    test_gpu_bulyan.test_planted_specials: every other value of the column is
    0.25, so every distance ties and the window goes left first; with n NaNs
    it stops one rank short of the first NaN, with n + 1 it touches it."""
    x = _base_rows(K, torch.float32, 9000 + K)
    keeps = br.keeps(K)
    assert len(keeps) <= len(PLANT_A)
    r = (K - 1) // 2
    for i, keep in enumerate(keeps):
        n = K - (max(0, r - keep + 1) + keep)
        assert 0 <= n < K - r  # the median itself stays 0.25 in the first column
        for a, b in zip(PLANT_A[i], PLANT_B[i]):
            x[:, a], x[:, b] = 0.25, 0.25
            _plant_nans(x, a, n)
            _plant_nans(x, b, n + 1)
    x[:, TM_POS_INF], x[:, TM_NEG_INF], x[:, TM_NEG_ZERO] = INF, -INF, -0.0
    refs = []
    for i, keep in enumerate(keeps):
        ref = br.nearmedian_mean_ref(x, keep)
        assert bool((ref[list(PLANT_A[i])] == 0.25).all()), (K, keep)
        assert bool(torch.isnan(ref[list(PLANT_B[i])]).all()), (K, keep)
        assert bool((ref[TM_POS_INF] == INF).all()) and bool((ref[TM_NEG_INF] == -INF).all())
        assert bool((ref[TM_NEG_ZERO] == 0).all()) and bool(torch.signbit(ref[TM_NEG_ZERO]).all())
        refs.append((keep, ref))
    return x, refs


@pytest.mark.parametrize("K", KS)
def test_nearmedian_mean_f32(K, cuda_device):
    """A tier's smallest K is where the select chain for the median's rank
    starts, its largest runs the padded offset kernel at K == KMAX."""
    x, refs = _nearmedian_case(K)
    rows = _Rows(x, cuda_device)
    for keep, ref in refs:
        for N in NS:
            got = rows.run(lambda p, k, n, out: dfn.nearmedian_mean_rows(p, k, n, keep, out), N)
            tmr.assert_same(got, ref[:N], f"nearmedian mean K={K} keep={keep} N={N}")
