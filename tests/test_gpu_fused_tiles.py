"""The twelve fused FedOpt server steps (fedagg_wsum_fedopt_*_f32 in
csrc/fedagg.hip) at every tile, alignment form and client-loop shape, bit for
bit against the oracle with the IEEE sqrt (any NaN matches any
NaN, as golden_util.assert_same has it): the parameters and every state
buffer, on every column.

Which launch a case reaches (launch_fused, launch_fused_cfg, reduce_block and
reduce_edge at this commit).  fp32 rows hold E = 4 elements per 16-byte pack;
epi_tiles.py has the tile table (a shipped block is 4,096 elements):

  tile   N                           kernel with the flag   without the flag
  Small  1 .. 1,044,480              U16 V1, 64 lanes       reduce_edge, 16 clients in flight
  Mid2   1,044,481 .. 2,093,056      U2 V4, 256 lanes       reduce_edge,  4 clients in flight
  Mid    2,093,057 .. 16,777,216     U1 V4                  the same
  Cfg    16,777,217 ..               U4 V4                  the same

With FEDAGG_ALIGNED16 the launch is reduce_fused_kernel (the 128-VGPR cap;
Adagrad and RMSprop: reduce_kernel): a block whose packs are all whole runs
EPI::pre, the client loop on 16-byte loads and EPI::pack; a ragged last block
runs reduce_edge and EPI::one.  Without the flag the launch is
reduce_kernel<..., false, ...>: every block runs reduce_edge and EPI::one.

Sizes per tile (epi_tiles.sizes): "first" has one element in a last block of
its own (Small: N = 1), "first+3" one whole pack there (a block that is not
full still runs reduce_edge), "whole" and "last" are whole numbers of blocks:
no element path with the flag.  Small also runs 4,097 = sixteen 256-element
blocks and one element.

Client 0 seeds the chain; the fast path then takes (K - 1) // U batches of U
clients and one predicated block for the other (K - 1) % U, reduce_edge
batches of 16 (Small) or 4 and the rest one by one (test_epi_tiles.py checks
these shapes):

  K at Small (either path): 1 nothing, 2 remainder 1, 16 remainder 15, 17 one
      batch, 18 one batch + 1, 33 two batches; 300 (N = 4,097 only, device
      weights: past the 256 a launch takes by value) eighteen batches + 11
  K at Mid2 (U = 2): 2 remainder 1, 3 one batch, 4 one batch + 1, 5 two batches
  K at Mid (U = 1, no remainder block): 2 one step, 3 two steps
  K at Cfg (U = 4): 4 remainder 3, 5 one batch, 6 one batch + 1
  K without the flag on the 256-lane tiles: 5 one batch of 4, 6 one batch + 1

Forms: A everything on a 16-byte boundary, flag set; B the same, flag clear;
C rows, parameter and states 4 bytes past a boundary, flag clear; D (Small)
the rows, the parameter or the first state buffer off alone, flag clear.

Client 1 (client 0 where K = 1) carries NaN, +inf, -inf, 1e-40, -0.0 and 3e38
in columns 0-5, in the last six columns and, from two shipped blocks on, in
the first six columns of the last full block.

Each case runs step 1 (first_step = 1) and step 2 on the carried state; RAdam
also step 6 (rho_t > 5: the rectified branch) where marked.  Before step 1
the state of SGD with momentum, Adam and AdamW and ASGD's ax (mu = 1) hold the
sentinel NaN: a step that read them would leave a NaN in a finite column."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import epi_tiles as et
from fedml_amd import _native as nat
from fedml_amd import fedopt as fo
from fedml_amd import kernels as kn
from oracle import fedavg_oracle as orc

pytestmark = pytest.mark.gpu

VARIANTS = ["sgd0", "sgd9", "adam", "adamw", "adagrad", "rmsprop", "adamax", "nadam", "radam", "adadelta", "asgd",
            "rprop"]
LR, SGD_LR, WD = 0.01, 0.5, 0.01
N_STATES = {"sgd0": 0, "sgd9": 1, "adam": 2, "adamw": 2, "adagrad": 1, "rmsprop": 1, "adamax": 2, "nadam": 2,
            "radam": 2, "adadelta": 2, "asgd": 1, "rprop": 2}
IGNORED_ON_STEP_1 = {"sgd9": (0,), "adam": (0, 1), "adamw": (0, 1), "asgd": (0,)}  # state the first step must not read
# form: byte offsets of (rows, parameter, state 0, state 1), FEDAGG_ALIGNED16
FORMS = {"A": (0, 0, 0, 0, True), "B": (0, 0, 0, 0, False), "C": (4, 4, 4, 4, False),
         "Drows": (4, 0, 0, 0, False), "Dparam": (0, 4, 0, 0, False), "Dstate": (0, 0, 4, 0, False)}


def _weights(K: int):
    ws = [i + 3.0 for i in range(K)]
    return [w / sum(ws) for w in ws]


class _Data:
    """The rows of one (N, K), built once for every optimizer and form: the
    placed rows, the starting parameters, the oracle's average."""

    def __init__(self, N: int, K: int, dev):
        g = torch.Generator(device=dev).manual_seed(N % 1009 + 7 * K)
        x = torch.randn(K, N, generator=g, device=dev) * 0.02
        sp = et.special_columns(4, N)
        x[min(1, K - 1), torch.tensor([c for c, _ in sp], device=dev)] = \
            torch.tensor([et.SPECIALS[j] for _, j in sp], device=dev)
        self.N, self.K, self.dev = N, K, dev
        self.p0 = torch.randn(N, generator=g, device=dev) * 0.02
        self.hp0 = self.p0.cpu().numpy()
        self.ws = _weights(K)
        host = x.cpu()
        self.avg = orc.wsum([host[i] for i in range(K)], self.ws).numpy()
        self.finite = torch.isfinite(x).all(dim=0)
        self._placed = {0: et.place_rows(x, 0)}
        self._tables = {}

    def table(self, off: int) -> torch.Tensor:
        if off not in self._placed:
            self._placed[off] = et.place_rows(self._placed[0][2], off)
        if off not in self._tables:
            self._tables[off] = kn.upload_i64(self._placed[off][1], self.dev)
        return self._tables[off]

    def weights(self, src: str):
        return kn.HostWeights(self.ws) if src == "host" else kn.upload_f32(self.ws, self.dev)


@functools.lru_cache(maxsize=2)
def _data(N: int, K: int, dev) -> _Data:
    return _Data(N, K, dev)


class _Oracle:
    def __init__(self, v: str, hp: np.ndarray, N: int):
        self.v, self.p, self.s = v, hp.copy(), [None, None]
        self.st = orc.optrepo_init(v, N, LR) if v in orc.OPTREPO_STATE else None

    def step(self, avg: np.ndarray, step: int) -> None:
        v = self.v
        if v in ("sgd0", "sgd9"):
            self.p, self.s[0] = orc.fedopt_sgd(self.p, avg, self.s[0], SGD_LR, 0.9 if v == "sgd9" else 0.0, step == 1)
        elif v in ("adam", "adamw"):
            self.p, self.s[0], self.s[1] = orc.fedopt_adam(self.p, avg, self.s[0], self.s[1], LR, step, sqrt="ieee",
                                                           weight_decay=WD if v == "adamw" else 0.0)
        elif v == "adagrad":
            self.p, self.s[0] = orc.fedopt_adagrad(self.p, avg, self.s[0], 0.1, sqrt="ieee")
        elif v == "rmsprop":
            self.p, self.s[0] = orc.fedopt_rmsprop(self.p, avg, self.s[0], LR, sqrt="ieee")
        else:
            self.p = orc.fedopt_step(v, self.p, avg, self.st, LR, step, sqrt="ieee")
            names = orc.OPTREPO_STATE[v]
            self.s = [self.st[names[0]], self.st[names[1]] if len(names) > 1 else None]


def _launch(v, d_ptrs, w, K, N, p, s0, s1, step, aligned, carry) -> None:
    """One fused step through the wrappers of fedml_amd.kernels; `aligned`
    sets FEDAGG_ALIGNED16 (the wrappers clear it for an offset buffer)."""
    first = step == 1
    if v in ("sgd0", "sgd9"):
        kn.wsum_fedopt_sgd(d_ptrs, w, K, N, p, s0, SGD_LR, 0.9 if v == "sgd9" else 0.0, first, aligned)
    elif v == "adam":
        kn.wsum_fedopt_adam(d_ptrs, w, K, N, p, s0, s1, kn.adam_scalars(LR, 0.9, 0.999, 1e-8, step), first, aligned)
    elif v == "adamw":
        kn.wsum_fedopt_adamw(d_ptrs, w, K, N, p, s0, s1, kn.adam_scalars(LR, 0.9, 0.999, 1e-8, step), 1 - LR * WD,
                             first, aligned)
    elif v == "adagrad":
        kn.wsum_fedopt_adagrad(d_ptrs, w, K, N, p, s0, 0.1, 1e-10, aligned)
    elif v == "rmsprop":
        kn.wsum_fedopt_rmsprop(d_ptrs, w, K, N, p, s0, LR, 0.99, 1e-8, aligned)
    else:
        kn.wsum_fedopt_optrepo(v, d_ptrs, w, K, N, p, s0, s1, kn.optrepo_scalars(v, LR, step, carry), aligned)


def _states(v: str, N: int, offs, dev, poison: bool = True):
    """The variant's state buffers as torch creates them before the first step
    (zeros; Rprop's step_size = lr), the ones step 1 must ignore poisoned."""
    out = []
    for i in range(N_STATES[v]):
        s = et.Guarded(N, torch.float32, offs[i], dev, fill=LR if (v == "rprop" and i == 1) else 0.0)
        if poison and i in IGNORED_ON_STEP_1.get(v, ()):
            s.poison()
        out.append(s)
    return out


def _run(v: str, N: int, K: int, form: str, wsrc: str, dev, steps=(1, 2), sgd0_buffer: bool = False,
         wrapper_flag: bool = False) -> None:
    d = _data(N, K, dev)
    r_off, p_off, s0_off, s1_off, flag = FORMS[form]
    table, w = d.table(r_off), d.weights(wsrc)
    P = et.Guarded(N, torch.float32, p_off, dev, fill=d.p0)
    S = _states(v, N, (s0_off, s1_off), dev)
    spare = et.Guarded(N, torch.float32, s0_off, dev).poison() if sgd0_buffer else None  # momentum 0: never touched
    ts = [s.t for s in S] + [None, None]
    if spare is not None:
        ts[0] = spare.t
    carry = fo.optrepo_carry(v, LR) if v in orc.OPTREPO_STATE else None
    oracle = _Oracle(v, d.hp0, N)
    for step in steps:
        _launch(v, table, w, K, N, P.t, ts[0], ts[1], step, flag or wrapper_flag, carry)
        oracle.step(d.avg, step)
        what = f"{v} N={N} K={K} form {form} weights {wsrc} step {step}"
        P.check(what + " param")
        et.assert_bits(P.t, oracle.p, what + " param")
        for i, s in enumerate(S):
            s.check(f"{what} state {i}")
            et.assert_bits(s.t, oracle.s[i], f"{what} state {i}")
            assert not bool((torch.isnan(s.t) & d.finite).any()), f"{what} state {i}: NaN in a finite column"
        if spare is not None:
            assert spare.untouched(), what + ": the buffer of momentum 0 was written"


# ---------------------------------------------------------------------------
# Cases: (N, K, form, weights)

_S = et.sizes(4, et.SMALL)
_M2, _M, _C = et.sizes(4, et.MID2), et.sizes(4, et.MID), et.sizes(4, et.CFG)


def _small_cases():
    out = []
    ns = [_S["first"], _S["first+3"], _S["whole"], et.N_FOR_K300]
    for i, N in enumerate(ns):
        for j, K in enumerate(k for k in et.K_FAST[et.SMALL] if k != et.K_DEVICE_WEIGHTS_ONLY):
            out.append((N, K, "A", "host" if (i + j) % 2 else "dev"))
            out.append((N, K, "C", "dev" if (i + j) % 2 else "host"))
    for K in (2, 17, 18):
        out.append((et.N_FOR_K300, K, "B", "host" if K % 2 else "dev"))
    for form in ("A", "B", "C"):  # 300 clients: eighteen batches and eleven, device weights
        out.append((et.N_FOR_K300, et.K_DEVICE_WEIGHTS_ONLY, form, "dev"))
    for form in ("Drows", "Dparam", "Dstate"):
        out.append((et.N_FOR_K300, 18, form, "host"))
    out += [(_S["last"], 2, "A", "host"), (_S["last"], 18, "B", "host"), (_S["last"], 17, "C", "dev")]
    return out


def _crossed(tile: int, names):
    """Every size in `names` with every K of the tile: the fast-path list with
    the flag, the element-path list 4 bytes off; the weight source alternates."""
    s, out = et.sizes(4, tile), []
    for i, name in enumerate(names):
        out += [(s[name], K, "A", "host" if (i + j) % 2 else "dev") for j, K in enumerate(et.K_FAST[tile])]
        out += [(s[name], K, "C", "dev" if (i + j) % 2 else "host") for j, K in enumerate(et.K_EDGE[tile])]
    return out


# The sizes of 16.8 M columns (Mid's last, all of Cfg) differ in their last
# block only, which runs the element path's own client loop whatever the fast
# path's K: there every size, every K and both forms occur, not every pair.
CASES = {
    "small": _small_cases(),
    "mid2": _crossed(et.MID2, ("first", "first+3", "whole", "last")) +
            [(_M2["first+3"], 5, "B", "host"), (_M2["whole"], 6, "B", "dev")],
    "mid": _crossed(et.MID, ("first", "first+3", "whole")) +
           [(_M["last"], 3, "A", "host"), (_M["last"], 5, "C", "dev")],
    "cfg": [(_C["first"], 4, "A", "host"), (_C["first+3"], 5, "A", "dev"), (_C["whole"], 6, "A", "host"),
            (_C["first"], 5, "C", "dev"), (_C["whole"], 6, "C", "host")],
}
# RAdam's step 6 at one size per tile
RADAM_STEP6 = {("small", et.N_FOR_K300, 18, "A"), ("mid2", _M2["first"], 2, "A"), ("mid", _M["first"], 2, "A"),
               ("cfg", _C["first"], 4, "A")}


def _params():
    out = []
    for tile, cases in CASES.items():
        for (N, K, form, wsrc) in cases:  # the variants of one case run back to back: its rows are built once
            for v in VARIANTS:
                if form == "Dstate" and N_STATES[v] == 0:
                    continue
                out.append(pytest.param(tile, v, N, K, form, wsrc, id=f"{tile}-N{N}-K{K}-{form}-{wsrc}-{v}"))
    return out


@pytest.mark.parametrize("tile,v,N,K,form,wsrc", _params())
def test_fused_step(tile, v, N, K, form, wsrc, cuda_device):
    assert et.tile_of(4, N) == et.TILE_NAMES.index(tile) == nat.lib().fedagg_epi_tile(4, N)
    steps = (1, 2, 6) if v == "radam" and (tile, N, K, form) in RADAM_STEP6 else (1, 2)
    _run(v, N, K, form, wsrc, cuda_device, steps)


@pytest.mark.parametrize("form", ["A", "C"])
@pytest.mark.parametrize("N", [et.N_FOR_K300, _M2["first"]])
def test_sgd_without_momentum_leaves_a_buffer_alone(N, form, cuda_device):
    """momentum == 0 with d_mom given (test_fused_step passes NULL): the
    poisoned buffer comes back untouched, the parameters are the oracle's."""
    _run("sgd0", N, 5, form, "host", cuda_device, sgd0_buffer=True)


@pytest.mark.parametrize("v", VARIANTS)
def test_wrapper_clears_the_flag_for_an_offset_parameter(v, cuda_device):
    """kn.wsum_fedopt_* called with aligned=True and a parameter 4 bytes past
    its boundary: the wrapper clears FEDAGG_ALIGNED16, the result is the
    oracle's (16-byte stores to that address would not be)."""
    _run(v, et.N_FOR_K300, 5, "Dparam", "host", cuda_device, wrapper_flag=True)


# ---------------------------------------------------------------------------
# fedagg_wsum_fedopt_batch

def test_batch_equals_single_calls(cuda_device):
    """One table through fedagg_wsum_fedopt_batch on one device and stream:
    Small and Mid2 sizes mixed, an unaligned entry, a FEDAGG_FEDOPT_AVG entry;
    bit for bit what the single calls give (themselves checked against the
    oracle above)."""
    dev = cuda_device
    entries = [("adam", et.N_FOR_K300, 5, "A"), ("sgd9", _M2["first"], 2, "A"), ("avg", _M2["first"], 2, "A"),
               ("nadam", et.N_FOR_K300, 5, "C"), ("rmsprop", _M2["first"], 2, "B"), ("asgd", et.N_FOR_K300, 5, "A")]
    opt_code = {"sgd9": nat.FEDOPT_SGD, "adam": nat.FEDOPT_ADAM, "rmsprop": nat.FEDOPT_RMSPROP, **nat.OPT_CODES}
    tab = (nat.FedOptLaunch * len(entries))()
    keep, single = [], []
    stream = nat.stream_handle()
    for desc, (v, N, K, form) in zip(tab, entries):
        d = _data(N, K, dev)
        r_off, p_off, s0_off, s1_off, flag = FORMS[form]
        table, w = d.table(r_off), d.weights("dev")
        bufs = []
        for which in range(2):  # 0: the batch's buffers, 1: the single call's
            P = et.Guarded(N, torch.float32, p_off, dev, fill=d.p0)
            S = _states(v, N, (s0_off, s1_off), dev) if v != "avg" else []
            bufs.append((P, S))
        (P, S), (P1, S1) = bufs
        ts1 = [s.t for s in S1] + [None, None]
        desc.d_src, desc.weights, desc.K, desc.N = table.data_ptr(), w.data_ptr(), K, N
        desc.d_param = P.t.data_ptr()
        desc.d_state0 = S[0].t.data_ptr() if len(S) > 0 else 0
        desc.d_state1 = S[1].t.data_ptr() if len(S) > 1 else 0
        desc.device, desc.stream, desc.first_step = dev.index or 0, stream, 1
        desc.flags = nat.FEDAGG_ALIGNED16 if flag else 0
        desc.lr, desc.momentum, desc.eps, desc.alpha = (SGD_LR if v == "sgd9" else LR), 0.9, 1e-8, 0.99
        if v == "avg":
            desc.opt, desc.dtype = nat.FEDOPT_AVG, nat.DT_F32
            kn.wsum_ptrs(torch.float32, table, w, K, N, P1.t, flag)
        else:
            desc.opt = opt_code[v]
            carry = fo.optrepo_carry(v, LR) if v in orc.OPTREPO_STATE else None
            if v == "adam":
                sc = kn.adam_scalars(LR, 0.9, 0.999, 1e-8, 1)
            elif v in orc.OPTREPO_STATE:
                sc = kn.optrepo_scalars(v, LR, 1, fo.optrepo_carry(v, LR))
            else:
                sc = None
            if sc is not None:
                desc.scalars = ctypes.addressof(sc)
            _launch(v, table, w, K, N, P1.t, ts1[0], ts1[1], 1, flag, carry)
            keep.append(sc)
        keep += [table, w]
        single.append((v, P, S, P1, S1))
    nat.check(nat.lib().fedagg_wsum_fedopt_batch(tab, len(tab)), "batch")
    torch.cuda.synchronize()
    for v, P, S, P1, S1 in single:
        P.check(v), [s.check(v) for s in S]
        et.assert_bits(P.t, P1.t.clone(), f"batch {v} param")
        for i, (a, b) in enumerate(zip(S, S1)):
            et.assert_bits(a.t, b.t.clone(), f"batch {v} state {i}")
