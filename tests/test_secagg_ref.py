"""The numpy oracle of the LightSecAgg field arithmetic (oracle.finite_sum,
oracle.lsa_reconstruct) pinned, bit for bit, to the Python-integer restatement
in secagg_ref.py over the moduli, client counts and inputs that
test_gpu_secagg.py runs: a GPU failure there then points at the kernel."""
from __future__ import annotations

import numpy as np
import pytest

import secagg_ref as ref
from oracle import fedavg_oracle as orc

N = 300  # the directed columns and ~280 random ones, half of them full-range int64
CLIENTS = [1, 2, 3, 5, 17, 18]


@pytest.mark.parametrize("K", CLIENTS)
@pytest.mark.parametrize("p", ref.MODULI)
def test_finite_sum_oracle_is_the_integer_reference(p, K):
    x = ref.sum_inputs(K, N, p, seed=K)
    want = ref.ref_sum(ref.columns(x), p)
    got = ref.oracle_sum(orc, x, p)
    assert got.dtype == np.int64
    assert got.tolist() == want
    if K > 1:
        assert all(0 <= v < p for v in want)


@pytest.mark.parametrize("K", CLIENTS)
@pytest.mark.parametrize("p", ref.MODULI)
def test_lsa_reconstruct_oracle_is_the_integer_reference(p, K):
    x, mask = ref.reconstruct_inputs(K, N, p, seed=100 + K)
    cols = ref.columns(x)
    for q in ref.Q_BITS:
        want = ref.ref_reconstruct(cols, mask.tolist(), p, q, K)
        got = ref.oracle_reconstruct(orc, x, mask, p, q)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg=f"q={q}")


def test_directed_columns_hold_what_they_name():
    """The directed columns reach the sums and residues their comments claim."""
    for p in ref.MODULI:
        for K in (2, 5, 18):
            s = ref.directed_sum(K, p)
            assert [sum(c) for c in s[:4]] == [p, p - 1, p + 1, p]
            assert all(0 <= v < p for c in s[:6] for v in c)
            assert sum(s[3][:-1]) < p  # exactly p only at the last client
            cols, mk = ref.directed_reconstruct(K, p)
            h = (p - 1) // 2
            got = [ref.wrap(ref.wrap(sum(c)) - m) % p for c, m in zip(cols[:13], mk[:13])]
            assert got == [0, 1, h - 1, h, h + 1, h + 2, p - 2, p - 1, h, h + 1, h + 2, p - 2, 1]


def _half_twice_rounded(p: int) -> float:
    return (float(p) - 1.0) / 2.0


def test_sign_threshold_is_rounded_once():
    """fl64((p-1)/2) is float(p - 1) / 2 (one rounding, exact halving), the form
    the host code uses.  (float(p) - 1) / 2 rounds twice: equal up to p = 2^53,
    off by an ulp at 2^53+1 and 2^53+3, where the residue 2^52 resp. (p+1)/2
    then lands on the other side of the threshold."""
    rng = np.random.default_rng(7)
    ps = ref.MODULI + [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 2, 2 ** 63 - 1] + \
        [int(v) for v in rng.integers(1, ref.I64_MAX, size=2000, dtype=np.int64)]
    for p in ps:
        assert float(p - 1) / 2.0 == (p - 1) / 2, p
        if p <= 2 ** 53:
            assert _half_twice_rounded(p) == (p - 1) / 2, p
    p = 2 ** 53 + 1
    assert float(2 ** 52) > _half_twice_rounded(p) and not float(2 ** 52) > (p - 1) / 2
    p = 2 ** 53 + 3
    m = (p + 1) // 2
    assert not float(m) > _half_twice_rounded(p) and float(m) > (p - 1) / 2
    # both residues are among the directed columns: h resp. h + 1 with h = (p - 1) // 2
    assert ref.directed_reconstruct(3, 2 ** 53 + 1)[0][3][0] == 2 ** 52
    assert ref.directed_reconstruct(3, 2 ** 53 + 3)[0][4][0] == m
