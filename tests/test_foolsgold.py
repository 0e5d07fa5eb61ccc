"""The host side of the "foolsgold_cos" defense: the weights from hand-made
Grams, the flags, the workspace arithmetic and the argument checks that need no GPU."""
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fedml_amd import _native as nat
from fedml_amd import defense as dfn
from fedml_amd.server_aggregator import _check_flags


def _gram(kind):
    G = np.eye(5)
    if kind == "copies":
        G[0, 1] = G[1, 0] = 1.0
    elif kind == "empty":
        G[2, 2] = 0.0
    elif kind == "nan":
        G[3, :] = G[:, 3] = np.nan
    return G


@pytest.mark.parametrize("kind,want", [("identity", [1, 1, 1, 1, 1]), ("copies", [0, 0, 1, 1, 1]),
                                       ("empty", [1, 1, 1, 1, 1]), ("nan", [1, 1, 1, 0, 1])])
def test_weights(kind, want):
    alpha, cs = dfn.foolsgold_weights(_gram(kind))
    assert alpha.tolist() == want
    assert cs[0, 1] == (1.0 if kind == "copies" else 0.0) and not cs.diagonal().any()


def test_weights_single_and_all_copies():
    assert dfn.foolsgold_weights(np.array([[2.5]]))[0].tolist() == [1.0]
    assert dfn.foolsgold_weights(np.full((3, 3), 7.3))[0].tolist() == [0.0, 0.0, 0.0]


def test_flags():
    assert dfn.DEFENSE_FOOLSGOLD_COS == "foolsgold_cos" and "foolsgold_cos" in dfn.SUPPORTED
    _check_flags(SimpleNamespace(enable_defense=True, defense_type="foolsgold_cos"))
    with pytest.raises(NotImplementedError):
        _check_flags(SimpleNamespace(enable_defense=True, defense_type="foolsgold"))


@pytest.mark.parametrize("K", [16, 128])
def test_work_len(K):
    wl = nat.lib().fedagg_robust_work_len
    nb = (K + 15) // 16
    kind = nat.WORK_HISTGRAM  # 8: test_fltrust.py and test_dist_defenses.py pin kinds 6 and 7 as unknown
    assert kind == 8 and wl(6, K, 4) == -1 and wl(7, K, 4) == -1
    assert [wl(kind, K, n) for n in (0, 1, 7, 256, 1000)] == [n * nb * (nb + 1) // 2 * 256 for n in (0, 1, 7, 256, 256)]
    assert wl(kind, 129, 4) == -1


@pytest.mark.parametrize("K,src,work_len", [(0, 8, 1 << 20), (129, 8, 1 << 20), (4, None, 1 << 20), (4, 8, 255)])
def test_einval_before_any_hip_call(K, src, work_len):
    # the pointers are never followed: the checks come first
    assert nat.lib().fedagg_histgram_f32(src, K, 8, None, 8, 1, 8, 8, work_len, None) == -1
    assert b"fedagg_histgram_f32" in nat.lib().fedagg_last_error()


def test_refused_before_device_work():
    d = OrderedDict(w=torch.zeros(3))
    with pytest.raises(ValueError, match="128"):
        dfn.foolsgold([(1.0, d)] * 129, d, dfn.FoolsGoldState(), method="fused")
    with pytest.raises(ValueError, match="duplicate"):
        dfn.foolsgold([(1.0, d)] * 3, d, dfn.FoolsGoldState(), client_ids=[4, 5, 4])
