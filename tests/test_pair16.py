"""Krum's 16-bit pair distances, the checks that need no device: argument
errors of pairdist2_rows and of the two C entries, and who may take 16-bit
weight keys."""
from __future__ import annotations

from collections import OrderedDict

import pytest
import torch

from fedml_amd import _native as nat
from fedml_amd import build as fbuild
from fedml_amd import defense as dfn


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pairdist2_rows_argument_checks(dtype):
    with pytest.raises(ValueError):
        dfn.pairdist2_rows(None, 16, None, 0, "cpu", "gram_wide", dtype=dtype)
    with pytest.raises(ValueError):
        dfn.pairdist2_rows(None, 129, None, 0, "cpu", "gram", dtype=dtype)
    assert dfn.PAIRGRAM16_AUTO.keys() == {torch.bfloat16, torch.float16}


def test_norm_diff_clipping_still_refuses_bf16():
    d = OrderedDict(w=torch.zeros(8, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="fp32 weight keys"):
        dfn._weight_bucket([d, d], "norm_diff_clipping")


@pytest.mark.parametrize("name", ["fedagg_pairgram2_16", "fedagg_pairdist2_16"])
def test_entries_reject_bad_arguments_before_any_device_call(name):
    fbuild.build()
    fn = getattr(nat.lib(), name)
    P = 64  # a non-null placeholder: every call below fails before anything is read
    ok = nat.lib().fedagg_robust_work_len(nat.WORK_PAIRGRAM, 4, 1)
    assert fn(nat.DT_BF16, P, 0, P, 1, P, P, ok, None) == -1          # K < 1
    assert fn(nat.DT_F32, P, 4, P, 1, P, P, ok, None) == -1           # a dtype that is not 16-bit
    assert fn(7, P, 4, P, 1, P, P, ok, None) == -1
    assert fn(nat.DT_F16, P, 4, P, -1, P, P, ok, None) == -1          # n_chunks < 0
    assert fn(nat.DT_F16, None, 4, P, 1, P, P, ok, None) == -1        # null rows
    assert fn(nat.DT_F16, P, 4, P, 1, None, P, ok, None) == -1        # null output
    assert fn(nat.DT_BF16, P, 4, None, 1, P, P, ok, None) == -1       # null chunk table
    assert fn(nat.DT_BF16, P, 4, P, 1, P, None, ok, None) == -1       # null workspace
    assert fn(nat.DT_BF16, P, 4, P, 1, P, P, 1, None) == -1           # short workspace
    assert b"workspace" in nat.lib().fedagg_last_error()
    if name == "fedagg_pairgram2_16":
        assert fn(nat.DT_BF16, P, 129, P, 1, P, P, 1 << 30, None) == -1   # K > 128
