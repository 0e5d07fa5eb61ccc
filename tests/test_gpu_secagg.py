"""The LightSecAgg field kernels (fedagg_sum_mod_i64, fedagg_lsa_reconstruct_f32
in csrc/fedagg.hip) at every tile, modulus and client-loop shape, bit for bit:
int64 equality for the modular sum, int32 views of the fp32 output for the
reconstruction.  The reference is secagg_ref.py's Python-integer restatement up
to _EXACT_BELOW chain steps and the numpy oracle above (test_secagg_ref.py pins
the two to each other).

Which launch a case reaches (launch_epi, reduce_block, reduce_edge at this
commit).  int64 rows hold E = 2 elements per 16-byte pack, and the tile is
picked from blocks_for(N) = ceil(ceil(N / 2) / 1024), the count of the shipped
256-lane x 4-pack blocks of 2,048 elements:

  tile   blocks            N                         U  V  lanes  elements/block
  Small  < 256             1 .. 522,240             16  1   64       128
  Mid2   256 .. 511        522,241 .. 1,046,528      2  4  256     2,048
  Mid    512 .. 4,096      1,046,529 .. 8,388,608    1  4  256     2,048
  Cfg    > 4,096           8,388,609 ..              4  4  256     2,048

(kSmallBelowBlocks = 256, kMid2BelowBlocks = 512, kMidUpToBlocks = 4096; the
block count is rounded up before it is compared, so the Small and Mid2 tiles
end one block below 2^19 and 2^20 elements.)

With FEDAGG_ALIGNED16 a block whose packs are all whole takes the fast path
(16-byte loads, LsaEpi::pack, the mask as a pack); a ragged last block, and
every block without the flag, takes reduce_edge (scalar loads, LsaEpi::one).
Client 0 seeds the chain, then the fast path takes (K - 1) // U batches of U
clients and a remainder block of (K - 1) % U; reduce_edge does the same with
batches of 16 (Small) or 8 (the 256-lane tiles) and a one-by-one remainder.

  K at Small (U = 16): 1 nothing, 2 remainder 1, 16 remainder 15, 17 one batch,
      18 one batch + 1, 33 two batches, 300 eighteen batches + 11
  K at Mid2 (U = 2): 2 remainder 1, 3 one batch, 4 one batch + 1, 5 two batches;
      10 without the flag: one edge batch of 8 + 1
  K at Mid (U = 1, no remainder block): 2 one step, 3 two steps
  K at Cfg (U = 4): 4 remainder 3, 5 one batch, 6 one batch + 1

Every input starts with the directed columns of secagg_ref.py; the other
columns alternate field elements (the conditional subtract of
OpSumModI64::step) and full-range int64 (its exact floor modulo)."""
from __future__ import annotations

import copy
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import secagg_ref as ref
from fedml_amd import _native as nat
from fedml_amd import kernels as kn
from fedml_amd import secagg
from oracle import fedavg_oracle as orc

pytestmark = pytest.mark.gpu

_EXACT_BELOW = 200_000  # K * N up to which the Python-integer reference runs
_PAD = 64  # sentinel elements on either side of an output
_SENT_I64 = 0x5A5A5A5A5A5A5A5A
_SENT_F32 = 0x7FC0BEEF  # a quiet NaN with a payload: equal only as bits


def _rows(x: np.ndarray, aligned: bool, dev):
    """The K rows of x in one device buffer, every row on a 16-byte boundary
    (aligned) or 8 bytes past one: (the buffer, the pointer table)."""
    K, N = x.shape
    stride = (N + 1) // 2 * 2 + 2  # even, so the rows keep the first one's alignment
    off = 0 if aligned else 1
    buf = torch.zeros(K * stride + 2, dtype=torch.int64, device=dev)
    buf[off:off + K * stride].view(K, stride)[:, :N].copy_(torch.from_numpy(x))
    ptrs = [buf.data_ptr() + 8 * (off + i * stride) for i in range(K)]
    assert all((q % 16 == 0) == aligned for q in ptrs)
    return buf, kn.upload_i64(ptrs, dev)


def _vector(v: np.ndarray, aligned: bool, dev):
    """(the buffer, the address of v in it), aligned as _rows does."""
    off = 0 if aligned else 1
    buf = torch.zeros(len(v) + 2, dtype=torch.int64, device=dev)
    buf[off:off + len(v)].copy_(torch.from_numpy(v))
    return buf, buf.data_ptr() + 8 * off


class _Out:
    """N output elements between _PAD sentinels; `shift` elements move the
    written range off its 16-byte boundary."""

    def __init__(self, N: int, dtype, shift: int, dev):
        self.N, self.lead = N, _PAD + shift
        self.bits = torch.int64 if dtype == torch.int64 else torch.int32
        self.sent = _SENT_I64 if dtype == torch.int64 else _SENT_F32
        self.buf = torch.full((self.lead + N + _PAD,), self.sent, dtype=self.bits, device=dev)
        self.ptr = self.buf.data_ptr() + self.lead * self.buf.element_size()
        assert (self.ptr % 16 == 0) == (shift == 0)

    def result(self, what: str) -> np.ndarray:
        """The written range as integers, after checking both sentinel ranges."""
        host = self.buf.cpu().numpy()
        assert (host[:self.lead] == self.sent).all(), f"{what}: wrote before the output"
        assert (host[self.lead + self.N:] == self.sent).all(), f"{what}: wrote past the output"
        return host[self.lead:self.lead + self.N]


def _flags(aligned: bool) -> int:
    return nat.FEDAGG_ALIGNED16 if aligned else 0


def gpu_sum(x: np.ndarray, p: int, aligned: bool, dev) -> np.ndarray:
    K, N = x.shape
    keep, ptrs = _rows(x, aligned, dev)
    out = _Out(N, torch.int64, 0 if aligned else 1, dev)
    nat.check(nat.lib().fedagg_sum_mod_i64(ptrs.data_ptr(), K, N, p, out.ptr, _flags(aligned), nat.stream_handle()),
              "sum_mod_i64")
    return out.result(f"sum N={N} K={K} p={p} aligned={aligned}")


def gpu_reconstruct(x: np.ndarray, mask: np.ndarray, p: int, q: int, w: float, aligned: bool, dev,
                    shift=None) -> np.ndarray:
    """The fp32 output as int32 bits.  Without the flag the output sits 8 bytes
    (shift = 2 floats) off its boundary unless told otherwise."""
    K, N = x.shape
    keep, ptrs = _rows(x, aligned, dev)
    mkeep, mptr = _vector(mask, aligned, dev)
    out = _Out(N, torch.float32, (0 if aligned else 2) if shift is None else shift, dev)
    nat.check(nat.lib().fedagg_lsa_reconstruct_f32(ptrs.data_ptr(), K, N, mptr, p, q, w, out.ptr, _flags(aligned),
                                                   nat.stream_handle()), "lsa_reconstruct_f32")
    return out.result(f"reconstruct N={N} K={K} p={p} q={q} aligned={aligned}")


def _w(K: int) -> float:
    return float(np.float32(1 / K))


@functools.lru_cache(maxsize=None)
def _small_sum(K: int, N: int, p: int):
    x = ref.sum_inputs(K, N, p, seed=N + K)
    return x, np.array(ref.ref_sum(ref.columns(x), p), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _small_reconstruct(K: int, N: int, p: int, q: int, Kw: int):
    x, mask = ref.reconstruct_inputs(K, N, p, seed=1000 + N + K)
    return x, mask, ref.ref_reconstruct(ref.columns(x), mask.tolist(), p, q, Kw).view(np.int32)


def _check(got: np.ndarray, want: np.ndarray, what: str) -> None:
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at column {bad[0]}: " \
                          f"got {got[bad[0]]}, want {want[bad[0]]}"


# ---------------------------------------------------------------------------
# Small tile: every block edge, every client-loop shape, every modulus

# one lane, one pack, a pack and a half, a block less one element, one block,
# one block and a half-filled pack, two blocks, two blocks and a half-filled pack
SMALL_N = [1, 2, 3, 127, 128, 129, 256, 257]
SMALL_K = [1, 2, 16, 17, 18, 33, 300]


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset8"])
@pytest.mark.parametrize("K", SMALL_K)
@pytest.mark.parametrize("N", SMALL_N)
def test_small_tile_sizes_and_clients(N, K, aligned, cuda_device):
    """With the flag, N >= 128 has fast-path blocks (N = 128, 256: nothing
    else; 129, 257: and a ragged block holding half a pack); below, and
    without the flag, reduce_edge alone.  The modulus and q rotate with the case."""
    i = SMALL_N.index(N) + SMALL_K.index(K)
    p, q = ref.MODULI[i % len(ref.MODULI)], ref.Q_BITS[i % len(ref.Q_BITS)]
    x, want = _small_sum(K, N, p)
    _check(gpu_sum(x, p, aligned, cuda_device), want, f"sum p={p}")
    x, mask, want = _small_reconstruct(K, N, p, q, K)
    _check(gpu_reconstruct(x, mask, p, q, _w(K), aligned, cuda_device), want, f"reconstruct p={p} q={q}")


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset8"])
@pytest.mark.parametrize("p", ref.MODULI)
def test_small_tile_every_modulus(p, aligned, cuda_device):
    """Three fast-path blocks and a ragged one, one client batch and a
    remainder, all directed columns, every q_bits."""
    K, N = 18, 385
    x, want = _small_sum(K, N, p)
    _check(gpu_sum(x, p, aligned, cuda_device), want, "sum")
    for q in ref.Q_BITS:
        x, mask, want = _small_reconstruct(K, N, p, q, K)
        _check(gpu_reconstruct(x, mask, p, q, _w(K), aligned, cuda_device), want, f"reconstruct q={q}")


@pytest.mark.parametrize("p", [2 ** 53 + 1, 2 ** 53 + 3])
def test_sign_threshold_above_2_53(p, cuda_device):
    """(p - 1) / 2 is no float64 here; the threshold is its correctly rounded
    value, as the reference's Python quotient.  (double(p) - 1) / 2 is an ulp
    off and flips the sign at the residue 2^52 resp. (p + 1) / 2: client 0
    carries the residues around h = (p - 1) // 2, mask and other clients zero."""
    h = (p - 1) // 2
    res = [h - 2, h - 1, h, h + 1, h + 2, h + 3]
    for K in (1, 3):
        x = np.zeros((K, len(res)), dtype=np.int64)
        x[0] = res
        mask = np.zeros(len(res), dtype=np.int64)
        for q in (0, 10):
            want = ref.ref_reconstruct(ref.columns(x), mask.tolist(), p, q, K)
            assert [bool(v > 0) for v in want] == [r <= h for r in res]  # every p here is odd: h is exact
            for aligned in (True, False):
                got = gpu_reconstruct(x, mask, p, q, _w(K), aligned, cuda_device)
                _check(got, want.view(np.int32), f"K={K} q={q} aligned={aligned}")


@pytest.mark.parametrize("Kw", [1, 3, 5, 17])
@pytest.mark.parametrize("q", ref.Q_BITS)
def test_reconstruct_scalars(q, Kw, cuda_device):
    """2^-q_bits is exact at both ends of [0, 62]; w = fl32(1 / Kw) has a full
    mantissa for 3, 5 and 17, so the last multiply rounds."""
    K, N = 3, 257
    for p in (2 ** 31 - 1, 2 ** 61 - 1):
        x, mask, want = _small_reconstruct(K, N, p, q, Kw)
        for aligned in (True, False):
            _check(gpu_reconstruct(x, mask, p, q, _w(Kw), aligned, cuda_device), want, f"p={p} aligned={aligned}")


def test_reconstruct_output_four_bytes_off(cuda_device):
    """The scalar stores of LsaEpi::one need only the element's own alignment."""
    K, N, p, q = 5, 129, 32749, 10
    x, mask, want = _small_reconstruct(K, N, p, q, K)
    for shift in (1, 3):
        _check(gpu_reconstruct(x, mask, p, q, _w(K), False, cuda_device, shift=shift), want, f"shift={shift}")


# ---------------------------------------------------------------------------
# The first and last sizes of the tiles

_B = 2048  # elements of a 256-lane block
# (N, K, p, q_bits, aligned).  N = blocks * _B has a full last block (fast path
# in every lane); blocks * _B + 1 adds a block of one half-filled pack, so that
# block alone takes reduce_edge.  255 * _B is the last Small size; 255 * _B + 1,
# 511 * _B + 1 and 4096 * _B + 1 are the first sizes of Mid2, Mid and Cfg.
TILE_CASES = [
    ("small-last-full", 255 * _B, 2, 2 ** 31 - 1, 16, True),
    ("mid2-first-ragged", 255 * _B + 1, 2, 32749, 10, True),
    ("mid2-full", 256 * _B, 3, 2 ** 62 + 1, 0, True),
    ("mid2-full-k4", 256 * _B, 4, 2 ** 53 + 1, 16, True),
    ("mid2-full-k5", 256 * _B, 5, 2 ** 61 - 1, 62, True),
    ("mid2-ragged-offset8", 255 * _B + 1, 4, 2 ** 63 - 25, 10, False),
    ("mid2-ragged-offset8-k10", 255 * _B + 1, 10, 2 ** 31 - 1, 16, False),
    ("mid-first-ragged", 511 * _B + 1, 2, 2 ** 62, 62, True),
    ("mid-full", 512 * _B, 3, 2 ** 53 + 1, 10, True),
    ("mid-ragged-offset8", 511 * _B + 1, 3, 32749, 0, False),
    ("cfg-first-ragged", 4096 * _B + 1, 4, 2 ** 61 - 1, 16, True),
    ("cfg-full", 4097 * _B, 5, 2 ** 62 + 1, 10, True),
    ("cfg-full-k6", 4097 * _B, 6, 2 ** 63 - 25, 62, True),
    ("cfg-ragged-offset8", 4096 * _B + 1, 5, 2 ** 53 + 3, 0, False),
]


@pytest.mark.parametrize("name,N,K,p,q,aligned", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_tile_bounds(name, N, K, p, q, aligned, cuda_device):
    assert K * N > _EXACT_BELOW
    x = ref.sum_inputs(K, N, p, seed=N % 1000 + K)
    _check(gpu_sum(x, p, aligned, cuda_device), ref.oracle_sum(orc, x, p), "sum")
    x, mask = ref.reconstruct_inputs(K, N, p, seed=N % 1000 + K + 50)
    want = ref.oracle_reconstruct(orc, x, mask, p, q).view(np.int32)
    _check(gpu_reconstruct(x, mask, p, q, _w(K), aligned, cuda_device), want, "reconstruct")


# ---------------------------------------------------------------------------
# Argument checks

def test_argument_checks(cuda_device):
    """FEDAGG_EINVAL (-1) for K < 1, N < 0, p <= 0, q_bits outside [0, 62] and
    null pointers, before anything is launched; N == 0 is FEDAGG_OK and writes
    nothing."""
    lib = nat.lib()
    x = ref.sum_inputs(2, 8, 32749, seed=1)
    keep, ptrs = _rows(x, True, cuda_device)
    mkeep, mptr = _vector(np.zeros(8, dtype=np.int64), True, cuda_device)
    oi, of = _Out(8, torch.int64, 0, cuda_device), _Out(8, torch.float32, 0, cuda_device)
    st = nat.stream_handle()
    A = nat.FEDAGG_ALIGNED16
    src = ptrs.data_ptr()

    def s(src=src, K=2, N=8, p=32749, out=oi.ptr):
        return lib.fedagg_sum_mod_i64(src, K, N, p, out, A, st)

    def r(src=src, K=2, N=8, mask=mptr, p=32749, q=10, out=of.ptr):
        return lib.fedagg_lsa_reconstruct_f32(src, K, N, mask, p, q, 0.5, out, A, st)

    for call in (s, r):
        for bad in (dict(K=0), dict(K=-1), dict(N=-1), dict(p=0), dict(p=-32749), dict(p=-(2 ** 63)),
                    dict(src=None), dict(out=None)):
            assert call(**bad) == -1, (call.__name__, bad)
            assert lib.fedagg_last_error()
    for bad in (dict(q=-1), dict(q=63), dict(mask=None)):
        assert r(**bad) == -1, bad
    assert s(N=0) == 0 and r(N=0) == 0
    assert r(q=0) == 0 and r(q=62) == 0 and s(p=2 ** 63 - 1) == 0  # the ends of the accepted ranges
    torch.cuda.synchronize()
    # every rejected call and the two empty ones left both outputs alone; the
    # accepted ones wrote their 8 elements and nothing else
    oi.result("sum"), of.result("reconstruct")
    oi2, of2 = _Out(8, torch.int64, 0, cuda_device), _Out(8, torch.float32, 0, cuda_device)
    assert s(N=0, out=oi2.ptr) == 0 and r(N=0, out=of2.ptr) == 0
    oi2.N = of2.N = 0  # the whole buffer counts as sentinel
    oi2.result("sum N=0"), of2.result("reconstruct N=0")


# ---------------------------------------------------------------------------
# fedml_amd.secagg: the per-key cut of the mask, the padding, the client subset

# a single element, a short odd key, a key ending before a pack boundary, one
# longer than two Small blocks, an empty key and a 0-d key
_KEYS = [("one", (1,)), ("five", (5,)), ("k1023", (1023,)), ("k4099", (4099,)), ("empty", (0,)), ("scalar", ()),
         ("mat", (3, 7))]


def _models(n: int, p: int, seed: int):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = OrderedDict()
        for k, shape in _KEYS:
            a = rng.integers(0, p, size=shape, dtype=np.int64)
            if a.ndim == 1 and a.size > 4:
                a[1::3] = rng.integers(-3 * p, 3 * p, size=a[1::3].shape, dtype=np.int64)
            d[k] = a
        out.append(d)
    dim = sum(int(np.prod(s)) for _, s in _KEYS)
    return out, rng.integers(0, p, size=(dim, 1), dtype=np.int64)


def _same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())


@pytest.mark.parametrize("K", [1, 4])
def test_aggregate_models_in_finite_ragged_keys(K, cuda_device):
    p = 2 ** 31 - 1
    dicts, _ = _models(K, p, seed=K)
    before = copy.deepcopy(dicts)
    want = orc.finite_sum(dicts, p)
    got = secagg.aggregate_models_in_finite(dicts, p)
    assert list(got) == [k for k, _ in _KEYS] and got is not dicts[0]
    for k in want:
        assert _same(got[k], want[k]), k
    for d, b in zip(dicts, before):  # the inputs are left as they were
        assert list(d) == list(b) and all(_same(d[k], b[k]) for k in b)


@pytest.mark.parametrize("active", [[4, 1, 3], [2]], ids=["subset-4-1-3", "single"])
def test_model_reconstruction_active_subset(active, cuda_device):
    """Only the active clients are summed, in the order given; w = 1 / len(active);
    the result is the first active client's dict, a 0-d key comes back (1,)."""
    p, q = 2 ** 31 - 1, 16
    dicts, mask = _models(6, p, seed=9)
    md = {i: d for i, d in enumerate(dicts)}
    before = copy.deepcopy(md)
    want = orc.lsa_reconstruct([copy.deepcopy(md[c]) for c in active], mask, p, q)
    got = secagg.model_reconstruction(md, active, mask, p, q)
    assert got is md[active[0]]
    assert list(got) == [k for k, _ in _KEYS]
    for (k, shape) in _KEYS:
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == (shape if shape else (1,)), k
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    for c in range(6):
        if c != active[0]:
            assert all(_same(md[c][k], before[c][k]) for k in before[c]), c
    # every active client matters: the reference over one fewer is another result
    if len(active) > 1:
        other = orc.lsa_reconstruct([before[c] for c in active[:-1]], mask, p, q)
        assert not torch.equal(other["k4099"], want["k4099"])


def test_non_int64_key_is_a_type_error_before_gpu_work(monkeypatch):
    def no_device(device):
        raise AssertionError("reached the device")

    monkeypatch.setattr(secagg, "_device", no_device)
    dicts, mask = _models(2, 32749, seed=3)
    dicts[0]["five"] = dicts[0]["five"].astype(np.int32)
    with pytest.raises(TypeError):
        secagg.aggregate_models_in_finite(dicts, 32749)
    with pytest.raises(TypeError):
        secagg.model_reconstruction({0: dicts[0], 1: dicts[1]}, [0, 1], mask, 32749, 10)
