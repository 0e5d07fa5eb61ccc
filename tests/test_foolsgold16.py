"""The host side of "foolsgold_cos" on bf16 / f16 models: the specification on
16-bit rows, the refusals and fedagg_histgram_16's argument checks, none of
which needs a GPU."""
from collections import OrderedDict
from types import SimpleNamespace

import pytest
import torch

from fedml_amd import _native as nat
from fedml_amd import defense as dfn

DTS = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dt", DTS)
def test_specification_widens_first(dt):
    gen = torch.Generator().manual_seed(3)
    x, r = torch.randn((5, 300), generator=gen).to(dt), torch.randn(300, generator=gen).to(dt)
    h = torch.randn((5, 300), generator=gen)
    cols = torch.arange(7, 290)
    h16, h32 = h.clone(), h.clone()
    G16 = dfn.histgram_rows_torch(x, r, h16, cols)
    G32 = dfn.histgram_rows_torch(x.float(), r.float(), h32, cols)
    assert torch.equal(G16, G32) and torch.equal(h16, h32) and not torch.equal(h16, h)
    assert torch.equal(h16[:, :7], h[:, :7]) and torch.equal(h16[:, 290:], h[:, 290:])
    assert not dfn.histgram16_auto(dt, 129) and dfn.histgram16_auto(dt, 128) == dfn.HISTGRAM16_AUTO[dt][128]


@pytest.mark.parametrize("dt", DTS)
def test_refusals(dt):
    d32, d16 = OrderedDict(w=torch.zeros(3)), OrderedDict(w=torch.zeros(3, dtype=dt))
    with pytest.raises(TypeError, match="global_model"):
        dfn.foolsgold([(1.0, d32)] * 3, d16, dfn.FoolsGoldState())
    with pytest.raises(TypeError, match="global_model"):
        dfn.foolsgold([(1.0, d16)] * 3, d32, dfn.FoolsGoldState())
    with pytest.raises(NotImplementedError, match="takes fp32 models"):  # host dicts of a 16-bit model
        dfn.foolsgold([(1.0, d16)] * 3, d16, dfn.FoolsGoldState())
    state = dfn.FoolsGoldState()

    def group(t):
        return SimpleNamespace(keys=["w"], offsets=[0], numels=[3], rows=torch.zeros((1, 64), dtype=t), dtype=t)

    state.bind(group(torch.float32), "cpu")
    state.bind(group(torch.float32), "cpu")
    with pytest.raises(ValueError, match="new FoolsGoldState"):
        state.bind(group(dt), "cpu")
    state = dfn.FoolsGoldState()
    state.bind(group(dt), "cpu")
    with pytest.raises(ValueError, match="new FoolsGoldState"):
        state.bind(group(torch.float32), "cpu")


@pytest.mark.parametrize("dtype,K,src,work_len", [(1, 0, 8, 1 << 20), (2, 129, 8, 1 << 20), (1, 4, None, 1 << 20),
                                                  (2, 4, 8, 255), (7, 4, 8, 1 << 20), (0, 4, 8, 1 << 20)])
def test_einval_before_any_hip_call(dtype, K, src, work_len):
    # the pointers are never followed: the checks come first
    assert nat.lib().fedagg_histgram_16(dtype, src, K, 8, None, 8, 1, 8, 8, work_len, None) == -1
    assert b"fedagg_histgram_16" in nat.lib().fedagg_last_error()
