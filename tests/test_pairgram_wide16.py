"""The 16-bit wide Gram, the checks that need no device: argument errors of
fedagg_pairgram2_wide_16 and of pairdist2_rows, and the tier table."""
from __future__ import annotations

import pytest
import torch

from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn

P = 64  # a non-null placeholder: every call below fails before anything is read


@pytest.mark.parametrize("args", [
    (nat.DT_F32, P, 200, P, P, 1, P, P, None),       # a dtype that is not 16-bit
    (7, P, 200, P, P, 1, P, P, None),
    (nat.DT_BF16, P, 0, P, P, 1, P, P, None),        # K < 1
    (nat.DT_BF16, P, 1025, P, P, 1, P, P, 1 << 40),  # K > 1024
    (nat.DT_F16, P, 200, P, P, -1, P, P, None),      # n_chunks < 0
    (nat.DT_F16, None, 200, P, P, 1, P, P, None),    # null rows
    (nat.DT_F16, P, 200, None, P, 1, P, P, None),    # null centre
    (nat.DT_F16, P, 200, P, None, 1, P, P, None),    # null chunk table
    (nat.DT_BF16, P, 200, P, P, 1, None, P, None),   # null output
    (nat.DT_BF16, P, 200, P, P, 1, P, None, None),   # null workspace
    (nat.DT_BF16, P, 200, P, P, 1, P, P, 1),         # short workspace
])
def test_entry_rejects_bad_arguments_before_any_device_call(args):
    fbuild.build()
    *head, wl = args
    if wl is None:
        wl = nat.lib().fedagg_robust_work_len(nat.WORK_PAIRGRAM_WIDE, 200, 1)
    assert nat.lib().fedagg_pairgram2_wide_16(*head, wl, None) == -1
    if wl == 1:
        assert b"workspace" in nat.lib().fedagg_last_error()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pairdist2_rows_argument_checks(dtype):
    with pytest.raises(ValueError, match="1024"):
        dfn.pairdist2_rows(None, 1025, None, 0, "cpu", "gram_wide", length=8, dtype=dtype)
    with pytest.raises(ValueError, match="length or a centre"):
        dfn.pairdist2_rows(None, 200, None, 0, "cpu", "gram_wide", dtype=dtype)
    assert dfn.PAIRGRAM_WIDE16_AUTO.keys() == {torch.bfloat16, torch.float16}
    assert dfn.PAIRGRAM_WIDE16_AUTO[dtype].keys() == {256, 512, 1024}
