"""LightSecAgg server-side field arithmetic on MI355X.

Mirrors, on the same numpy inputs and with identical results:

  aggregate_models_in_finite(weights_finite, prime_number)
      core/mpc/lightsecagg.py:134-148 — per key, w = x_0; w = (w + x_i) mod p
      over clients (numpy int64: wrapping adds, floor modulo).
  model_reconstruction(model_dict, active_clients, aggregate_mask, p, q_bits)
      the per-key loop of LightSecAggAggregator.aggregate_model_reconstruction
      (cross_silo/lightsecagg/lsa_fedml_aggregator.py:139-166): sum the masked
      finite models of the first-round survivors, cancel the decoded
      aggregate mask, mod p, de-quantize (my_q_inv / transform_finite_to_tensor,
      lightsecagg.py:157-182) and scale by 1/K — fused into ONE launch.

  aggregate_mask_reconstruction(aggregate_encoded_mask_dict, active_clients, ...)
      LightSecAggAggregator.aggregate_mask_reconstruction: the aggregate mask
      decoded from the survivors' encoded shares by Lagrange coded computing
      (LCC_decoding_with_points, lightsecagg.py: (U_dec.dot(f_eval)) % p).  It
      is a U x U by U x d/(U-T) int64 matrix product over the field, as large
      as the other two steps together, and numpy has no BLAS for int64 (NOTES.md
      5f: seconds on the host); lcc_decode runs it on the GPU, on the exact
      64-bit kernel or on the int8 matrix cores (csrc/lccdecode.hip), and the
      decoded mask can go to model_reconstruction without leaving the device.
      Only the U x U Lagrange coefficients (lagrange_coeffs) are host work.
"""
from __future__ import annotations

import copy
from collections import OrderedDict
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _native as nat
from . import kernels as kn
from .bucket import ClientBucket


# method="auto" of lcc_decode: the matrix-core kernel only where it beat the
# exact kernel at the tier's full size AND at a padded one by more than the
# larger min-max spread (tools/lcc_decode_probe.py, profiles/lcc_decode_probe.json,
# p = 2^15 - 19, T = U / 2, d = 25,610,152; key: the smallest tier >= U).
# Unmeasured sizes (U > 512) stay on the exact kernel.  Median ms (min-max) of 10,
# matrix cores / exact kernel, outputs bit-identical at every shape:
#   U = 32:  0.196 (0.194-0.199) / 0.238 (0.234-0.246)   U = 24:  0.233 (0.229-0.236) / 0.230 (0.226-0.237)
#   U = 128: 0.155 (0.152-0.156) / 0.701 (0.700-0.711)   U = 100: 0.158 (0.154-0.165) / 0.692 (0.687-0.704)
#   U = 512: 0.240 (0.235-0.243) / 2.829 (2.813-2.842)   U = 384: 0.210 (0.206-0.213) / 2.144 (2.138-2.152)
# The 32 tier wins at U = 32 but not at its padded U = 24 (k is padded to 64), so it stays False.
LCC_MFMA_AUTO = {32: False, 128: True, 512: True}
_METHODS = {"valu": nat.LCC_VALU, "mfma": nat.LCC_MFMA}


def _device(device) -> torch.device:
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise nat.FedAggNativeError("fedml_amd needs a GPU (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _int64_layout(d: "OrderedDict") -> list:
    lay = []
    for k, v in d.items():
        a = np.asarray(v)
        if a.dtype != np.int64:
            raise TypeError(f"key {k!r}: finite-field tensors are int64 (got {a.dtype})")
        lay.append((k, tuple(a.shape), torch.int64))
    return lay


def _fill(bucket: ClientBucket, dicts: Sequence["OrderedDict"]) -> None:
    for i, d in enumerate(dicts):
        # np.ascontiguousarray would turn a 0-d key into shape (1,)
        bucket.put(i, {k: torch.from_numpy(np.array(v, dtype=np.int64, order="C", copy=True)) for k, v in d.items()}, 1)
    bucket.sync_ingest()


def lagrange_coeffs(target_points, eval_points, p: int) -> np.ndarray:
    """The R x U decoding matrix of LCC_decoding_with_points as canonical field
    values: C[t][j] = prod_{l != j} (beta_t - alpha_l) (alpha_j - alpha_l)^-1 mod p
    (what gen_Lagrange_coeffs yields for p < 2^31), in exact Python ints."""
    p = int(p)
    if p < 2:
        raise ValueError("lagrange_coeffs: p must be a prime >= 2")
    alpha = [int(a) % p for a in eval_points]
    if len(set(alpha)) != len(alpha):
        raise ValueError("lagrange_coeffs: the evaluation points must be distinct mod p")
    out = np.zeros((len(target_points), len(alpha)), dtype=np.int64)
    inv_den = []
    for j, aj in enumerate(alpha):
        den = 1
        for l, al in enumerate(alpha):
            if l != j:
                den = den * (aj - al) % p
        inv_den.append(pow(den, -1, p))
    for t, beta in enumerate(target_points):
        for j in range(len(alpha)):
            num = 1
            for l, al in enumerate(alpha):
                if l != j:
                    num = num * (int(beta) - al) % p
            out[t, j] = num * inv_den[j] % p
    return out


def lcc_decode(f_eval_rows, coeffs, p: int, n_out=None, device=None, method: str = "auto", out=None) -> torch.Tensor:
    """(coeffs.dot(f_eval)) % p on the GPU with numpy's int64 semantics
    (fedagg_lcc_decode_i64): f_eval_rows are U equally long rows, host (numpy
    int64) or device int64 tensors; coeffs is R x U.  Returns the first n_out
    (default R * M) elements of the row-major product as a device tensor.
    method: "valu" (exact kernel), "mfma" (int8 matrix cores; anything outside
    the field is recomputed by the exact kernel, so the result is the same) or
    "auto" (LCC_MFMA_AUTO).  out: a contiguous device int64 tensor of at least
    n_out elements to decode into (its first n_out are returned)."""
    p = int(p)
    U = len(f_eval_rows)
    coef = np.ascontiguousarray(np.asarray(coeffs, dtype=np.int64))
    if coef.ndim != 2 or coef.shape[1] != U:
        raise ValueError(f"lcc_decode: coeffs must be R x {U} (got {coef.shape})")
    R = coef.shape[0]
    if method == "auto":
        tier = min((k for k in LCC_MFMA_AUTO if k >= U), default=None)
        method = "mfma" if tier is not None and LCC_MFMA_AUTO[tier] and p <= nat.LCC_MFMA_MAX_PRIME else "valu"
    if method not in _METHODS:
        raise ValueError(f"lcc_decode: unknown method {method!r}")
    dev = _device(device)
    with torch.cuda.device(dev):
        if all(isinstance(r, torch.Tensor) and r.is_cuda for r in f_eval_rows):
            rows = [r.reshape(-1).contiguous() for r in f_eval_rows]
            if any(r.dtype != torch.int64 or r.numel() != rows[0].numel() or r.device != dev for r in rows):
                raise TypeError("lcc_decode: device rows are equally long int64 tensors on the target device")
            M = rows[0].numel()
            d_ptrs = kn.upload_i64([r.data_ptr() for r in rows], dev)
        else:
            host = [np.asarray(r).reshape(-1) for r in f_eval_rows]
            M = host[0].size
            if any(r.size != M for r in host):
                raise ValueError("lcc_decode: rows of different lengths")
            rows = ClientBucket(_int64_layout(OrderedDict(f=host[0])), U, dev, promote_ints=False)
            _fill(rows, [OrderedDict(f=r) for r in host])
            d_ptrs = rows.groups[torch.int64].d_ptrs
        n_out = R * M if n_out is None else int(n_out)
        d_coef = torch.from_numpy(coef).to(dev)
        if out is None:
            out = torch.empty(max(n_out, 0), dtype=torch.int64, device=dev)
        elif out.dtype != torch.int64 or out.device != dev or not out.is_contiguous() or out.numel() < n_out:
            raise TypeError("lcc_decode: out must be a contiguous int64 tensor of >= n_out elements on the device")
        nbytes = nat.lib().fedagg_lcc_work_bytes(U, R, M) if method == "mfma" else 0
        work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        nat.check(nat.lib().fedagg_lcc_decode_i64(d_ptrs.data_ptr(), U, M, d_coef.data_ptr(), R, p, out.data_ptr(), n_out,
                                                  _METHODS[method], work.data_ptr(), work.numel(),
                                                  nat.stream_handle()), "lcc_decode_i64")
        torch.cuda.current_stream().synchronize()  # rows, d_coef and work are released on return
    return out.reshape(-1)[:max(n_out, 0)]


def aggregate_mask_reconstruction(aggregate_encoded_mask_dict, active_clients: Sequence[int], client_num: int,
                                  targeted_number_active_clients: int, privacy_guarantee: int, total_dimension: int,
                                  prime_number: int, device=None, method: str = "auto") -> torch.Tensor:
    """LightSecAggAggregator.aggregate_mask_reconstruction on the GPU: the
    aggregate mask, shape (d, 1), as a device tensor.  Evaluation points
    active_clients[i] + 1, targets N + 1 ... N + U, rows in active_clients
    order; only the ceil(d / M) target rows that FedML's [0:d] keeps are
    computed (FedML decodes all U and drops the rest)."""
    N, U, p, d = int(client_num), int(targeted_number_active_clients), int(prime_number), int(total_dimension)
    if len(active_clients) != U:
        raise ValueError(f"aggregate_mask_reconstruction: {len(active_clients)} active clients, U = {U}")
    rows = [aggregate_encoded_mask_dict[c] for c in active_clients]
    M = int(rows[0].numel() if isinstance(rows[0], torch.Tensor) else np.asarray(rows[0]).size)
    R = max(1, min(U, -(-d // max(M, 1))))
    coef = lagrange_coeffs([N + 1 + t for t in range(R)], [int(c) + 1 for c in active_clients], p)
    return lcc_decode(rows, coef, p, n_out=min(d, R * M), device=device, method=method).reshape(-1, 1)


def aggregate_models_in_finite(weights_finite: List["OrderedDict"], prime_number: int, device=None
                               ) -> "OrderedDict":
    """lightsecagg.py:134-148 on the GPU; returns a new dict of int64 arrays."""
    p = int(prime_number)
    K = len(weights_finite)
    w_sum = copy.copy(weights_finite[0])  # the reference deep-copies client 0's dict
    layout = _int64_layout(weights_finite[0])
    dev = _device(device)
    with torch.cuda.device(dev):
        bucket = ClientBucket(layout, K, dev, promote_ints=False)
        _fill(bucket, weights_finite)
        g = bucket.groups[torch.int64]
        out = torch.empty(g.padded, dtype=torch.int64, device=dev)
        nat.check(nat.lib().fedagg_sum_mod_i64(g.d_ptrs.data_ptr(), K, g.length, p, out.data_ptr(),
                                               nat.FEDAGG_ALIGNED16, nat.stream_handle()), "sum_mod_i64")
        host = out[:g.length].cpu().numpy()
    for key, off, n, shape in zip(g.keys, g.offsets, g.numels, g.shapes):
        w_sum[key] = host[off:off + n].reshape(shape).copy()
    return w_sum


def model_reconstruction(model_dict: Dict[int, "OrderedDict"], active_clients: Sequence[int],
                         aggregate_mask, prime_number: int, precision_parameter: int,
                         device=None) -> "OrderedDict":
    """The model-sized part of aggregate_model_reconstruction (:139-166):
    returns model_dict[active_clients[0]] with every key rebound to its float32
    average, as the reference does."""
    p = int(prime_number)
    q = int(precision_parameter)
    K = len(active_clients)
    dicts = [model_dict[c] for c in active_clients]
    averaged_params = dicts[0]
    layout = _int64_layout(averaged_params)
    on_device = isinstance(aggregate_mask, torch.Tensor) and aggregate_mask.is_cuda
    mask = aggregate_mask.reshape(-1) if on_device else np.asarray(aggregate_mask).reshape(-1)
    w = 1 / K  # :163, a Python float, rounded to fp32 by torch's mul
    dev = _device(device)
    with torch.cuda.device(dev):
        bucket = ClientBucket(layout, K, dev, promote_ints=False)
        _fill(bucket, dicts)
        g = bucket.groups[torch.int64]
        # the decoded mask, cut per key exactly as :147-151 does, in the row layout
        # (a device mask, e.g. aggregate_mask_reconstruction's, with device slices)
        mrow = torch.zeros(g.padded, dtype=torch.int64, device=dev) if on_device else np.zeros(g.padded, dtype=np.int64)
        pos = 0
        for off, n in zip(g.offsets, g.numels):
            mrow[off:off + n] = mask[pos:pos + n]
            pos += n
        d_mask = mrow if on_device else torch.from_numpy(mrow).to(dev)
        out = torch.empty(g.padded, dtype=torch.float32, device=dev)
        nat.check(nat.lib().fedagg_lsa_reconstruct_f32(g.d_ptrs.data_ptr(), K, g.length, d_mask.data_ptr(), p, q,
                                                       float(np.float32(w)), out.data_ptr(), nat.FEDAGG_ALIGNED16,
                                                       nat.stream_handle()), "lsa_reconstruct_f32")
        host = out[:g.length].cpu()
    for key, off, n, shape in zip(g.keys, g.offsets, g.numels, g.shapes):
        # a 0-d key comes back from my_q_inv as a numpy scalar, which
        # transform_finite_to_tensor wraps as torch.Tensor([x]): shape (1,)
        averaged_params[key] = host[off:off + n].clone().reshape(shape if len(shape) else (1,))
    return averaged_params
