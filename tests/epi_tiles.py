"""Where a reduction of csrc/fedagg.hip that goes through launch_epi or
launch_fused lands, restated without the library, and the placement of test
inputs around it: the tile table per element size, the client-loop shapes of
the fast and the element path, K lists that walk them, rows and guarded
buffers on or off a 16-byte boundary, and the special input values.

A 16-byte pack holds E = 16 / elem_bytes elements; a shipped block is 256
lanes x 4 packs = 1,024 packs.  The tile is picked from
blocks_for(N) = ceil(ceil(N / E) / 1024):

  tile   blocks        U  V  lanes   elements per block
  Small  < 256        16  1    64    64 E
  Mid2   256 .. 511    2  4   256    1,024 E
  Mid    512 .. 4,096  1  4   256    1,024 E
  Cfg    > 4,096       4  4   256    1,024 E

test_epi_tiles.py pins this table to the library's fedagg_epi_tile."""
from __future__ import annotations

import numpy as np
import torch

SMALL, MID2, MID, CFG = 0, 1, 2, 3
TILE_NAMES = ("small", "mid2", "mid", "cfg")
SMALL_BELOW_BLOCKS, MID2_BELOW_BLOCKS, MID_UPTO_BLOCKS = 256, 512, 4096
PACKS_PER_BLOCK = 256 * 4  # the shipped block
# (U clients in flight on the fast path, V packs per lane, lanes)
UVL = {SMALL: (16, 1, 64), MID2: (2, 4, 256), MID: (1, 4, 256), CFG: (4, 4, 256)}


def pack_elems(elem_bytes: int) -> int:
    return 16 // elem_bytes


def block_elems(elem_bytes: int) -> int:
    """Elements of one shipped block: 4,096 fp32, 8,192 16-bit, 2,048 8-byte."""
    return PACKS_PER_BLOCK * pack_elems(elem_bytes)


def blocks_for(elem_bytes: int, N: int) -> int:
    E = pack_elems(elem_bytes)
    packs = (N + E - 1) // E
    return (packs + PACKS_PER_BLOCK - 1) // PACKS_PER_BLOCK


def tile_of(elem_bytes: int, N: int) -> int:
    b = blocks_for(elem_bytes, N)
    if b < SMALL_BELOW_BLOCKS:
        return SMALL
    if b < MID2_BELOW_BLOCKS:
        return MID2
    if b <= MID_UPTO_BLOCKS:
        return MID
    return CFG


def table(elem_bytes: int):
    """[(tile, first N, last N)]; Cfg has no last N."""
    B = block_elems(elem_bytes)
    return [(SMALL, 1, (SMALL_BELOW_BLOCKS - 1) * B),
            (MID2, (SMALL_BELOW_BLOCKS - 1) * B + 1, (MID2_BELOW_BLOCKS - 1) * B),
            (MID, (MID2_BELOW_BLOCKS - 1) * B + 1, MID_UPTO_BLOCKS * B),
            (CFG, MID_UPTO_BLOCKS * B + 1, None)]


# a whole number of shipped blocks inside each tile (every lane on the fast path)
WHOLE_BLOCKS = {SMALL: 1, MID2: 300, MID: 600, CFG: 4098}


def sizes(elem_bytes: int, tile: int):
    """The tile's ragged variants as {name: N}: its first N (N = 1, or one
    element in a last block of its own), first N + 3 (fp32: exactly one more
    pack), a whole number of shipped blocks, and its last N (a whole number of
    blocks as well: the largest launch of the tile)."""
    _, first, last = table(elem_bytes)[tile]
    out = {"first": first, "first+3": first + 3, "whole": WHOLE_BLOCKS[tile] * block_elems(elem_bytes)}
    if last is not None:
        out["last"] = last
    assert all(tile_of(elem_bytes, n) == tile for n in out.values())
    return out


def fast_loop(K: int, tile: int):
    """(batches of U clients, clients of the predicated remainder block) after
    client 0 seeded the chain.  U = 1 (Mid) has no remainder block."""
    U = UVL[tile][0]
    return (K - 1) // U, (K - 1) % U


def edge_clients(elem_bytes: int, tile: int) -> int:
    """SU of reduce_edge<OP, V * E, BS>: clamp(64 / (V * E), 1, 16)."""
    m = UVL[tile][1] * pack_elems(elem_bytes)
    return max(1, min(16, 64 // m))


def edge_loop(K: int, elem_bytes: int, tile: int):
    """(batches of SU clients, clients taken one by one) of the element path."""
    su = edge_clients(elem_bytes, tile)
    return (K - 1) // su, (K - 1) % su


# K lists that walk the client loop of each tile.  Fast path, then the lists
# for launches without the flag (the element path; Small's SU is 16 = its U).
K_FAST = {SMALL: [1, 2, 16, 17, 18, 33, 300], MID2: [2, 3, 4, 5], MID: [2, 3], CFG: [4, 5, 6]}
K_EDGE = {SMALL: [1, 2, 16, 17, 18, 33, 300], MID2: [5, 6], MID: [5, 6], CFG: [5, 6]}
K_DEVICE_WEIGHTS_ONLY = 300  # past the 256 weights a launch takes by value
N_FOR_K300 = 4097  # the only size K = 300 runs at

# ---------------------------------------------------------------------------
# Special values

SPECIALS = [float("nan"), float("inf"), -float("inf"), 1e-40, -0.0, 3e38]


def special_columns(elem_bytes: int, N: int):
    """Where client 1 carries SPECIALS: columns 0-5, the last six columns and,
    where N holds two or more shipped blocks, the first six columns of the last
    full block.  [(column, index into SPECIALS)], columns below N only."""
    B = block_elems(elem_bytes)
    starts = [0, max(0, N - 6)]
    if N >= 2 * B:
        starts.append((N // B - 1) * B)
    out = {}
    for s in starts:
        for j in range(6):
            if 0 <= s + j < N:
                out[s + j] = j
    return sorted(out.items())


# ---------------------------------------------------------------------------
# Placement

PAD = 64  # sentinel elements on either side of a written buffer
SENT_F32 = 0x7FC0BEEF  # a quiet NaN with a payload: equal only as bits
#                                       0x7FD5 is a NaN as bf16 and as f16
_SENT = {4: (torch.int32, SENT_F32), 2: (torch.int16, 0x7FD5), 8: (torch.int64, 0x7FF8BEEF0BADF00D)}


def place_rows(x: torch.Tensor, off_bytes: int):
    """The K rows of x (K, N) in one device buffer, every row `off_bytes`
    (0 or 4; a multiple of the element size) past a 16-byte boundary:
    (the buffer, the rows' addresses, the rows as views of the buffer)."""
    K, N = x.shape
    es = x.element_size()
    assert off_bytes % es == 0 and 0 <= off_bytes < 16
    per16 = 16 // es
    stride = (N + per16 - 1) // per16 * per16 + per16  # a multiple of 16 bytes: rows keep the first one's offset
    off = off_bytes // es
    buf = torch.zeros(K * stride + per16, dtype=x.dtype, device=x.device)
    view = buf[off:off + K * stride].view(K, stride)[:, :N]
    view.copy_(x)
    ptrs = [buf.data_ptr() + es * (off + i * stride) for i in range(K)]
    assert all(p % 16 == off_bytes for p in ptrs)
    return buf, ptrs, view


class Guarded:
    """N elements of `dtype` between PAD sentinel elements, the first one
    `off_bytes` past a 16-byte boundary.  `.t` is the N-element view (what a
    kernel writes), `check()` asserts that both sentinel ranges are intact."""

    def __init__(self, N: int, dtype: torch.dtype, off_bytes: int, device, fill=None):
        es = torch.empty(0, dtype=dtype).element_size()
        assert off_bytes % es == 0 and 0 <= off_bytes < 16
        self.bits, self.sent = _SENT[es]
        self.N, self.lead = N, PAD + off_bytes // es
        self.buf = torch.full((self.lead + N + PAD,), self.sent, dtype=self.bits, device=device)
        self.t = self.buf[self.lead:self.lead + N].view(dtype)
        assert N == 0 or self.t.data_ptr() % 16 == off_bytes
        if fill is not None:
            self.t.copy_(fill) if isinstance(fill, torch.Tensor) else self.t.fill_(fill)

    def poison(self) -> "Guarded":
        """Fill the written range with the sentinel as well."""
        self.buf.fill_(self.sent)
        return self

    def untouched(self) -> bool:
        return bool((self.buf == self.sent).all())

    def check(self, what: str) -> None:
        assert bool((self.buf[:self.lead] == self.sent).all()), f"{what}: wrote before the buffer"
        assert bool((self.buf[self.lead + self.N:] == self.sent).all()), f"{what}: wrote past the buffer"


def bits_of(t: torch.Tensor) -> torch.Tensor:
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bits(got: torch.Tensor, want, what: str) -> None:
    """Every element of the device tensor `got` has the bits of `want` (a
    numpy array or tensor of the same format; bf16 as uint16 bits), any NaN
    matching any NaN as in golden_util.assert_same.  Compared on the device."""
    if isinstance(want, np.ndarray):
        if want.dtype == np.uint16:
            want = torch.from_numpy(want.view(np.int16)).view(torch.bfloat16)
        else:
            want = torch.from_numpy(np.ascontiguousarray(want))
    want = want.reshape(-1).to(got.device)
    got = got.reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = bits_of(got) != bits_of(want)
    if got.is_floating_point():
        bad &= ~(torch.isnan(got) & torch.isnan(want))
    if bool(bad.any()):
        idx = torch.nonzero(bad).flatten()
        i = int(idx[0])
        raise AssertionError(f"{what}: {idx.numel()} of {got.numel()} differ, first at column {i}: "
                             f"got {got[i].item()!r} ({int(bits_of(got)[i]):#x}), "
                             f"want {want[i].item()!r} ({int(bits_of(want)[i]):#x})")
