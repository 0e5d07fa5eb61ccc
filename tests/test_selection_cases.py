"""The builders of tests/selection_cases.py against the references, and the
torch slow path of the trimmed mean (defense.trimmed_mean_rows_torch) on the
inputs the GPU kernels get in test_gpu_selection_exhaustive.py; no GPU."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import selection_cases as sc
import trimmed_mean_ref as tmr
from fedml_amd import defense as dfn
from oracle import fedavg_oracle as orc

DT16 = [torch.bfloat16, torch.float16]
DT_IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
ids16 = [DT_IDS[d] for d in DT16]


def _oracle_median(rows: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(orc.lower_median_cols(rows.float().numpy())).to(rows.dtype)


@pytest.mark.parametrize("dtype", DT16, ids=ids16)
def test_ordered_patterns_are_the_total_order(dtype):
    o = sc.ordered_patterns(dtype)
    assert o.numel() == {torch.bfloat16: 65_282, torch.float16: 63_490}[dtype]
    v = sc.from_bits(o, dtype).float()
    assert not bool(torch.isnan(v).any())
    assert v[0] == -float("inf") and v[-1] == float("inf")
    keys = torch.from_numpy(tmr.order_keys(v.numpy()).astype(np.int64))
    assert bool((keys[1:] > keys[:-1]).all())  # strictly ascending: -0 before +0, no pattern twice
    n = sc.nan_patterns(dtype)
    assert bool(torch.isnan(sc.from_bits(n, dtype).float()).all())
    assert o.numel() + n.numel() == 1 << 16 and torch.unique(torch.cat([o, n])).numel() == 1 << 16


@pytest.mark.parametrize("dtype", DT16, ids=ids16)
def test_boundary_ranks(dtype):
    o = sc.ordered_patterns(dtype)
    assert torch.equal(sc.boundary_ranks(dtype, 1024), torch.arange(o.numel()))
    r = sc.boundary_ranks(dtype, 1025)
    assert r.numel() < o.numel() // 8 and int(r.min()) == 0 and int(r.max()) == o.numel() - 1
    v = sc.from_bits(o[r], dtype).float()
    tiny = torch.finfo(dtype).tiny
    for want in (-float("inf"), float("inf"), torch.finfo(dtype).max, -torch.finfo(dtype).max, tiny, -tiny):
        assert bool((v == want).any()), want
    bits = o[r] & 0xFFFF
    for b in (0x0000, 0x8000, 0x0001, 0x8001):  # both zeros and the smallest subnormals
        assert bool((bits == b).any()), hex(b)
    a = v.abs()
    assert int(((a > 0) & (a < tiny)).sum()) >= 2 * 64  # subnormals of both signs below the boundary


@pytest.mark.parametrize("spread", ["wide", "narrow"])
@pytest.mark.parametrize("dtype", DT16, ids=ids16)
@pytest.mark.parametrize("K", [1, 2, 3, 9, 33, 129])
def test_median_columns_match_the_oracle(K, dtype, spread):
    o = sc.ordered_patterns(dtype)
    ranks = torch.arange(0, o.numel(), 7 if K > 9 else 1)
    rows = sc.median_columns(dtype, K, ranks, spread, seed=K)
    assert rows.shape == (K, ranks.numel()) and rows.dtype == dtype
    want = sc.from_bits(o[ranks], dtype)
    assert torch.equal(tmr.bits(_oracle_median(rows)), tmr.bits(want))
    if spread == "narrow" and K >= 9:  # the window shares high bits and repeats values
        top = sc.to_bits(rows) >> 8
        assert float((top == top[0]).all(dim=0).float().mean()) > 0.5
    if K >= 9:
        assert not torch.equal(rows[:, 5], torch.sort(rows[:, 5].float()).values.to(dtype))  # permuted


@pytest.mark.parametrize("dtype", DT16, ids=ids16)
@pytest.mark.parametrize("K", [2, 20, 130])
def test_nan_columns_first_nan(K, dtype):
    rows, pats = sc.nan_columns(dtype, K, seed=K)
    assert pats.numel() == {torch.bfloat16: 254, torch.float16: 2046}[dtype]
    isn = torch.isnan(rows.float())
    assert bool((isn.sum(dim=0) == 2).all())
    first = isn.int().argmax(dim=0)
    got = sc.to_bits(rows)[first, torch.arange(pats.numel())]
    assert torch.equal(got, pats.to(torch.int64))
    wide = rows.float()  # the oracle selects among the widened values: compare there, payload included
    med = torch.from_numpy(orc.lower_median_cols(wide.numpy()))
    assert torch.equal(sc.to_bits(med), sc.to_bits(wide[first, torch.arange(pats.numel())]))
    if K > 2:
        assert first.unique().numel() > 1


def test_binary_closed_forms_K12():
    K = 12
    rows, ones = sc.binary_columns(K, torch.float32)
    assert rows.shape == (K, 1 << K) and torch.equal(ones, rows.sum(dim=0).long())
    assert torch.unique(rows.T.contiguous(), dim=0).shape[0] == 1 << K
    med = sc.binary_median(K, ones, torch.float32)
    assert torch.equal(tmr.bits(med), tmr.bits(_oracle_median(rows)))
    for trim in range(0, (K - 1) // 2 + 1):
        want = torch.from_numpy(tmr.trimmed_mean_f32(rows.numpy(), trim))
        assert torch.equal(tmr.bits(sc.binary_trimmed_mean(K, trim, ones, torch.float32)), tmr.bits(want)), trim
        for dtype in DT16:
            ref = tmr.trimmed_mean_ref(rows.to(dtype), trim)
            assert torch.equal(tmr.bits(sc.binary_trimmed_mean(K, trim, ones, dtype)), tmr.bits(ref)), (trim, dtype)


@pytest.mark.parametrize("K", [1, 5, 33, 100])
def test_placed_ones_and_orders(K):
    for ones in {0, 1, K // 2, K}:
        p = sc.placed_ones(K, ones, seed=1, n_random=64)
        assert p.shape == (K, 4 * K + 1 + 64)
        assert bool((p.sum(dim=0) == ones).all())
    if K == 33:
        p = sc.placed_ones(K, 3, seed=1, n_random=8)
        assert torch.nonzero(p[:, 2]).flatten().tolist() == [2, 3, 4]  # the run from offset 2
        assert torch.nonzero(p[:, K - 1]).flatten().tolist() == [0, 1, K - 1]  # wraps round
        assert torch.nonzero(p[:, K + 1]).flatten().tolist() == [1, 5, 9]  # 3 divides 33: the stride is 4
    o = sc.structured_orders(K, seed=2, n_random=16)
    assert bool((torch.sort(o, dim=0).values == torch.arange(K)[:, None]).all())  # permutations, every column
    assert o[:, 0].tolist() == list(range(K)) and o[:, 1].tolist() == list(range(K))[::-1]
    if K == 5:
        assert o[:, 2].tolist() == [0, 2, 4, 3, 1] and o[:, 3].tolist() == [4, 2, 0, 1, 3]
        assert o[:, 4].tolist() == [0, 2, 4, 1, 3] and o[:, 5].tolist() == [0, 4, 2, 1, 3]


@pytest.mark.parametrize("dtype", list(DT_IDS), ids=list(DT_IDS.values()))
def test_value_sets_ascend(dtype):
    for K in (2, 33, 512, 4097):
        for name, fn in sc.VALUE_SETS.items():
            v = fn(dtype, K)
            keys = torch.from_numpy(tmr.order_keys(v.float().numpy()).astype(np.int64))
            strict = name != "quarter" or dtype == torch.float32 or K <= 512
            assert bool((keys[1:] > keys[:-1]).all() if strict else (keys[1:] >= keys[:-1]).all()), (name, K)
        s = sc.seam_band(dtype, K).float()
        assert bool(torch.signbit(s[K // 2 - 1])) and s[K // 2 - 1] == 0 and not bool(torch.signbit(s[K // 2]))
    if dtype == torch.float32:
        assert bool((sc.seam_band(dtype, 4097).abs() < torch.finfo(dtype).tiny).all())  # denormals only


def test_radix_prefix_columns():
    K = 129
    x = sc.radix_prefix_columns(K, seed=3)
    assert x.shape[0] == K and 1_500 < x.shape[1] < 2_500
    assert not bool(torch.isnan(x).any())
    b = sc.to_bits(x)
    spread = b.max(dim=0).values ^ b.min(dim=0).values
    assert int((spread < 0x100).sum()) >= 5 * 64 and int(((spread & 0xFFFF00FF) == 0).sum()) >= 5 * 64
    assert bool(((x > 0) & (x < torch.finfo(torch.float32).tiny)).any()) and bool((x < 0).any())
    two = torch.tensor([torch.unique(b[:, c]).numel() == 2 for c in range(x.shape[1])])
    copies = {int((x[:, c] == x[:, c].min()).sum()) for c in torch.nonzero(two).flatten().tolist()}
    assert {1, K - 1, 64, 65, 66} <= copies  # one odd value; m, m + 1, m + 2 copies of the smaller


@pytest.mark.parametrize("dtype", DT16, ids=ids16)
def test_rounding_inputs(dtype):
    x = sc.rounding_inputs(dtype)
    n = sc.INF_BITS[dtype]
    assert x.numel() == 8 * n and bool(torch.isfinite(x).all())
    exact, mid, below, above = x[:n], x[n:2 * n], x[2 * n:3 * n], x[3 * n:4 * n]
    assert torch.equal(exact.to(dtype).float(), exact)  # the 16-bit values themselves
    assert bool((below < mid).all()) and bool((mid < above).all())
    lo = below.to(dtype).float()
    hi = above.to(dtype).float()
    assert torch.equal(lo, exact)  # just under the midpoint rounds down, just over it up, the tie to even
    assert bool((hi > exact).all()) and bool(torch.isinf(hi[-1]))
    tie = mid.to(dtype)
    assert bool(((tie.float() == lo) | (tie.float() == hi)).all())
    assert bool(((sc.to_bits(tie) & 1) == 0).all())
    assert torch.equal(x[4 * n:], -x[:4 * n])
    if dtype == torch.float16:
        assert mid[-1] == 65_520.0 and mid[0] == 2.0 ** -25
    nan = sc.nan_inputs(4_000, seed=0)
    assert bool(torch.isnan(nan).all()) and torch.unique(sc.to_bits(nan)).numel() > 3_900
    assert bool(torch.signbit(nan).any()) and not bool(torch.signbit(nan).all())


# ---- the torch slow path on the GPU tests' inputs ---------------------------------

def _slow(rows: torch.Tensor, trim: int, what: str) -> torch.Tensor:
    got = dfn.trimmed_mean_rows_torch(rows, trim)
    tmr.assert_same(got, tmr.trimmed_mean_ref(rows, trim), what)
    return got


@pytest.mark.parametrize("dtype", DT16, ids=ids16)
@pytest.mark.parametrize("K,trim", [(3, 1), (9, 4), (100, 49)])
def test_slow_path_identity_columns(K, trim, dtype):
    rows, want = sc.identity_columns(dtype, K, trim, "narrow", seed=K)
    if K == 100:  # the reference's stable argsort of 100 x 65,000 keys: a sample keeps the test quick
        pick = torch.arange(0, rows.shape[1], 16)
        rows, want = rows[:, pick].contiguous(), want[pick]
    got = _slow(rows, trim, f"identity K={K} {dtype}")
    M = K - 2 * trim
    exp = want if M == 1 else ((want.float() * M) / M).to(dtype)  # M equal values: exact until the sum overflows
    assert torch.equal(tmr.bits(got), tmr.bits(exp))
    zeros = torch.full((K, 4), -0.0, dtype=dtype)
    assert tmr.bits(_slow(zeros, trim, "all -0")).tolist() == tmr.bits(zeros[0]).tolist()


@pytest.mark.parametrize("dtype", DT16, ids=ids16)
def test_slow_path_tie_columns(dtype):
    rows = sc.tie_columns(dtype, seed=4)
    assert rows.shape == (4, sc.ordered_patterns(dtype).numel() - 3)
    got = _slow(rows, 1, f"ties {dtype}")
    over = torch.isinf(got.float())  # bf16: the pairs whose fp32 sum overflows; f16's largest pair ties down to even
    assert int(over.sum()) == (0 if dtype == torch.float16 else 2 * 127)  # both of the pair at 2^127 or above
    pair = torch.sort(rows.float(), dim=0).values[1:3]
    halfway = (got.float() != pair[0]) & (got.float() != pair[1])
    assert torch.equal(halfway, over)  # else a 16-bit mean of neighbours is one of the two


@pytest.mark.parametrize("dtype", list(DT_IDS), ids=list(DT_IDS.values()))
@pytest.mark.parametrize("K", list(range(1, 13)))
def test_slow_path_all_binary_columns(K, dtype):
    rows, ones = sc.binary_columns(K, dtype)
    for trim in range(0, (K - 1) // 2 + 1):
        got = _slow(rows, trim, f"0/1 K={K} trim={trim} {dtype}")
        assert torch.equal(tmr.bits(got), tmr.bits(sc.binary_trimmed_mean(K, trim, ones, dtype)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [130, 200])
def test_slow_path_structured_orders(K, dtype):
    order = sc.structured_orders(K, seed=K, n_random=128)
    for name, fn in sc.VALUE_SETS.items():
        rows = fn(dtype, K)[order]
        for trim in tmr.trims(K, extra=(K // 4,)):
            got = _slow(rows, trim, f"{name} K={K} trim={trim} {dtype}")
            assert bool((tmr.bits(got) == tmr.bits(got)[0]).all())  # one multiset of values: one result
