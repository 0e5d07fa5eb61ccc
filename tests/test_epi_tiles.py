"""CPU checks behind test_gpu_fused_tiles.py and test_gpu_epi_tiles.py: the
tile table of epi_tiles.py equals the library's fedagg_epi_tile (the constants
launch_epi and launch_fused switch on), every K list walks the client-loop
shapes it claims, and the argument checks of the entries that launch through
them return FEDAGG_EINVAL before any GPU call."""
from __future__ import annotations

import ctypes

import pytest

import epi_tiles as et
from fedml_amd import _native as nat
from fedml_amd import build as fbuild


@pytest.fixture(scope="module")
def lib():
    fbuild.build()
    return nat.lib()


# the issue's table, written out: last N of Small, Mid2 and Mid per element size
LAST_N = {4: (1_044_480, 2_093_056, 16_777_216), 2: (2_088_960, 4_186_112, 33_554_432),
          8: (522_240, 1_046_528, 8_388_608)}


@pytest.mark.parametrize("elem_bytes", [2, 4, 8])
def test_table_matches_the_library(lib, elem_bytes):
    tab = et.table(elem_bytes)
    assert [t for t, _, _ in tab] == [et.SMALL, et.MID2, et.MID, et.CFG]
    assert tuple(last for _, _, last in tab[:3]) == LAST_N[elem_bytes]
    assert tab[0][1] == 1 and all(tab[i + 1][1] == tab[i][2] + 1 for i in range(3)) and tab[3][2] is None
    for tile, first, last in tab:
        for n in (first - 1, first, first + 1) + (() if last is None else (last - 1, last, last + 1)):
            if n >= 0:
                assert lib.fedagg_epi_tile(elem_bytes, n) == et.tile_of(elem_bytes, n), (elem_bytes, n)
        assert lib.fedagg_epi_tile(elem_bytes, first) == tile
        if first > 1:
            assert lib.fedagg_epi_tile(elem_bytes, first - 1) == tile - 1
        if last is not None:
            assert lib.fedagg_epi_tile(elem_bytes, last) == tile
        for name, n in et.sizes(elem_bytes, tile).items():
            assert lib.fedagg_epi_tile(elem_bytes, n) == tile, (name, n)
    assert lib.fedagg_epi_tile(elem_bytes, 0) == et.SMALL
    assert lib.fedagg_epi_tile(elem_bytes, 2 ** 40) == et.CFG
    assert lib.fedagg_epi_tile(elem_bytes, -1) == -1


def test_tile_query_rejects_other_element_sizes(lib):
    for eb in (0, 1, 3, 16, -4):
        assert lib.fedagg_epi_tile(eb, 100) == -1


def test_sizes_are_the_ragged_variants():
    for eb in (2, 4, 8):
        B, E = et.block_elems(eb), et.pack_elems(eb)
        for tile in (et.SMALL, et.MID2, et.MID, et.CFG):
            s = et.sizes(eb, tile)
            assert s["first+3"] == s["first"] + 3 and s["whole"] % B == 0
            if tile != et.SMALL:
                assert s["first"] % B == 1  # one element in a last block of its own
                assert s["last"] % B == 0 if "last" in s else tile == et.CFG
            if eb == 4 and tile != et.SMALL:
                assert s["first+3"] % B == E  # exactly one whole pack in the last block


# (batches of U, remainder) on the fast path
FAST_SHAPES = {
    et.SMALL: {1: (0, 0), 2: (0, 1), 16: (0, 15), 17: (1, 0), 18: (1, 1), 33: (2, 0), 300: (18, 11)},
    et.MID2: {2: (0, 1), 3: (1, 0), 4: (1, 1), 5: (2, 0)},
    et.MID: {2: (1, 0), 3: (2, 0)},  # U = 1: one step per client, no remainder block
    et.CFG: {4: (0, 3), 5: (1, 0), 6: (1, 1)},
}
# (batches of SU, one by one) on the element path of fp32 rows (SU = 16, 4, 4, 4)
EDGE_SHAPES_F32 = {
    et.SMALL: FAST_SHAPES[et.SMALL],
    et.MID2: {5: (1, 0), 6: (1, 1)},
    et.MID: {5: (1, 0), 6: (1, 1)},
    et.CFG: {5: (1, 0), 6: (1, 1)},
}


def test_k_lists_walk_the_client_loops():
    assert [et.edge_clients(4, t) for t in range(4)] == [16, 4, 4, 4]
    assert [et.edge_clients(2, t) for t in range(4)] == [8, 2, 2, 2]  # 16-bit: E = 8
    assert [et.edge_clients(8, t) for t in range(4)] == [16, 8, 8, 8]  # 8-byte: E = 2
    for tile in range(4):
        assert sorted(FAST_SHAPES[tile]) == et.K_FAST[tile]
        assert sorted(EDGE_SHAPES_F32[tile]) == et.K_EDGE[tile]
        for K, shape in FAST_SHAPES[tile].items():
            assert et.fast_loop(K, tile) == shape, (tile, K)
        for K, shape in EDGE_SHAPES_F32[tile].items():
            assert et.edge_loop(K, 4, tile) == shape, (tile, K)
        fast = set(FAST_SHAPES[tile].values())
        assert any(b > 0 and r == 0 for b, r in fast)  # whole batches only
        if et.UVL[tile][0] > 1:
            assert any(b == 0 and r > 0 for b, r in fast)  # the remainder block alone
            assert any(b > 0 and r > 0 for b, r in fast)  # a batch, then the remainder block
            assert max(r for _, r in fast) == et.UVL[tile][0] - 1  # its last slot
        edge = set(EDGE_SHAPES_F32[tile].values())
        assert any(b > 0 and r == 0 for b, r in edge) and any(b > 0 and r > 0 for b, r in edge)
    assert et.K_DEVICE_WEIGHTS_ONLY > 256


def test_special_columns():
    assert et.special_columns(4, 1) == [(0, 0)]
    assert [c for c, _ in et.special_columns(4, 4)] == [0, 1, 2, 3]
    assert [c for c, _ in et.special_columns(4, 4097)] == list(range(6)) + list(range(4091, 4097))
    cols = dict(et.special_columns(4, 2 * 4096 + 5))
    assert [cols[4096 + j] for j in range(6)] == list(range(6))  # first columns of the last full block
    assert all(c in cols for c in range(2 * 4096 - 1, 2 * 4096 + 5))  # the ragged tail


# ---------------------------------------------------------------------------
# Argument checks: a rejected call reaches no GPU call (this module runs
# without one), so every pointer below is a number that is never dereferenced.

P = 4096  # stands for any non-null pointer
H = nat.FEDAGG_HOST_WEIGHTS


def _fused(lib, scal6, scal9):
    """name -> call(K, flags, param, state0, state1) for every fused entry."""
    s6, s9 = ctypes.addressof(scal6), ctypes.addressof(scal9)
    calls = {
        "sgd": lambda K, f, p, a, b: lib.fedagg_wsum_fedopt_sgd_f32(P, P, K, 100, p, a, 0.1, 0.9, 1, f, None),
        "adam": lambda K, f, p, a, b: lib.fedagg_wsum_fedopt_adam_f32(P, P, K, 100, p, a, b, s6, 1, f, None),
        "adamw": lambda K, f, p, a, b: lib.fedagg_wsum_fedopt_adamw_f32(P, P, K, 100, p, a, b, s6, 0.99, 1, f, None),
        "adagrad": lambda K, f, p, a, b: lib.fedagg_wsum_fedopt_adagrad_f32(P, P, K, 100, p, a, 0.1, 1e-10, f, None),
        "rmsprop": lambda K, f, p, a, b: lib.fedagg_wsum_fedopt_rmsprop_f32(P, P, K, 100, p, a, 0.1, 0.99, 1e-8, f,
                                                                            None),
    }
    for name, code in nat.OPT_CODES.items():
        calls[name] = (lambda K, f, p, a, b, code=code:
                       lib.fedagg_wsum_fedopt_optrepo_f32(code, P, P, K, 100, p, a, b, s9, f, None))
    return calls


ONE_STATE = ("sgd", "adagrad", "rmsprop")


def test_host_weights_limit_is_checked_before_the_gpu(lib):
    """FEDAGG_HOST_WEIGHTS copies K <= 256 weights into the launch: K = 257 is
    FEDAGG_EINVAL in all twelve fused entries and fedagg_wsum_rlr_f32;
    fedagg_wsum_muldiv takes device weights only."""
    calls = _fused(lib, (ctypes.c_float * 6)(), (ctypes.c_float * 9)())
    assert len(calls) == 11  # twelve steps: SGD with and without momentum share an entry
    for name, call in calls.items():
        assert call(257, H, P, P, P) == -1, name
        assert b"K <= 256" in lib.fedagg_last_error(), name
    assert lib.fedagg_wsum_rlr_f32(P, P, 257, 100, 1.0, P, H, None) == -1
    assert b"K <= 256" in lib.fedagg_last_error()
    for dt in (nat.DT_F32, nat.DT_BF16, nat.DT_F16, nat.DT_F64, nat.DT_I64):
        assert lib.fedagg_wsum_muldiv(dt, P, P, 2, 100, P, H, None) == -1
        assert b"device weights only" in lib.fedagg_last_error()


def test_null_state_pointers(lib):
    """A null parameter or state pointer is FEDAGG_EINVAL; ASGD has no second
    state buffer, so its state1 may be null: that call gets past the pointer
    check (and here stops at the host-weights limit instead)."""
    calls = _fused(lib, (ctypes.c_float * 6)(), (ctypes.c_float * 9)())
    for name, call in calls.items():
        assert call(2, 0, None, P, P) == -1 and b"null pointer" in lib.fedagg_last_error(), name
        assert call(2, 0, P, None, P) == -1 and b"null pointer" in lib.fedagg_last_error(), name
        if name in ONE_STATE:
            continue
        rc = call(257, H, P, P, None)
        assert rc == -1, name
        if name == "asgd":
            assert b"K <= 256" in lib.fedagg_last_error()
        else:
            assert b"null pointer" in lib.fedagg_last_error(), name
    # SGD without momentum takes no buffer
    assert lib.fedagg_wsum_fedopt_sgd_f32(P, P, 257, 100, P, None, 0.1, 0.0, 1, H, None) == -1
    assert b"K <= 256" in lib.fedagg_last_error()
    assert lib.fedagg_wsum_fedopt_adam_f32(P, P, 2, 100, P, P, P, None, 1, 0, None) == -1  # the scalars
    assert lib.fedagg_wsum_fedopt_optrepo_f32(1, P, P, 2, 100, P, P, P, None, 0, None) == -1
    assert lib.fedagg_wsum_rlr_f32(P, P, 2, 100, 1.0, None, 0, None) == -1
    assert lib.fedagg_wsum_muldiv(nat.DT_F32, P, None, 2, 100, P, 0, None) == -1


def test_unknown_optimizer_code(lib):
    s9, carry = (ctypes.c_float * 9)(), (ctypes.c_float * 2)()
    for code in (0, 7, -1, nat.FEDOPT_SGD):
        assert lib.fedagg_wsum_fedopt_optrepo_f32(code, P, P, 2, 100, P, P, P, ctypes.addressof(s9), 0, None) == -1
        assert b"unknown optimizer" in lib.fedagg_last_error()
        assert lib.fedagg_optrepo_scalars(code, 0.1, 1, ctypes.addressof(carry), ctypes.addressof(s9)) == -1
        assert b"unknown optimizer" in lib.fedagg_last_error()
    assert lib.fedagg_wsum_muldiv(nat.DT_I32, P, P, 2, 100, P, 0, None) == -1
    assert b"unsupported dtype" in lib.fedagg_last_error()
