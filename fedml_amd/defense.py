"""Robust aggregation on MI355X: the two FedML defenses
that are pure reductions over the client axis.

"wise_median"   CoordinateWiseMedianDefense.defend_on_aggregation
                (core/security/defense/coordinate_wise_median_defense.py:18-44):
                stack the "weight" keys of every client (vectorize_weight,
                core/security/common/utils.py:8-21: all keys except BatchNorm
                running_mean / running_var / num_batches_tracked), take
                torch.median over clients per coordinate (lower median; NaN if
                the column has one), then walk client 0's keys ALL of them
                assigning consecutive slices of that vector (.view(size)).
                The walk is reproduced as is: for models with BN buffers the
                slices no longer line up with the weight keys and the last
                .view() raises RuntimeError — exactly what FedML does.
                The median itself is fedagg_median (one launch over the
                whole weight row; fp32 rows, or bf16 / f16 rows for 16-bit
                models, whose torch.cat stays 16-bit; a mixed-width model's
                16-bit keys are widened into fp32 rows, as torch.cat promotes).

"trimmed_mean"  CoordinateWiseTrimmedMeanDefense.defend_before_aggregation
                (coordinate_wise_trimmed_mean_defense.py:19-26 ->
                common/utils.py:213-228 trimmed_mean): clients sorted by their
                sample count (compute_a_score), int(beta * K) dropped at each
                end, then ordinary FedAvg (our kernel) on the survivors.

"wise_trimmed_mean"
                Not in FedML: the coordinate-wise trimmed mean of Yin et al.
                FedML's "trimmed_mean" trims per client (whole clients, by
                sample count); "wise_trimmed_mean" trims per coordinate: every
                element of every key drops its int(beta * K) smallest and
                largest client values and averages the rest
                (fedagg_trimmed_mean, specified in include/fedagg.h: one
                launch per row group up to 128 clients, one launch of
                fedagg_trimmed_mean_wide from 129 to 1024 clients, the same
                rule in torch ops above that; BatchNorm statistics included,
                integer keys as fl32(v)).  Up to int(beta * K) clients sending anything,
                NaN and inf included, cannot move a coordinate outside the
                range of the honest values.

"geomed"        Not in FedML under this name: the geometric median of the clients'
                whole updates (RFA, Pillutla et al.; breakdown point 1/2 over
                clients, not per coordinate) by the smoothed Weiszfeld
                iteration, specified at geometric_median_loop.  One iteration
                is one pass over the rows: the weighted sum z and every
                client's distance to it (fedagg_wsum_dist2_f32, up to 128
                clients; fedagg_wsum_f32 + fedagg_dist2_f32 above that and
                where "auto" measured the pair faster).  FedML's own
                "geometric_median" / "RFA" loop (a Python set of weights, a
                truncating zip) is NOT reproduced: those names stay refused.

"wise_bulyan"   Not FedML's "bulyan" (which stays refused: its source is not
                mirrored here): Bulyan (El Mhamdi, Guerraoui, Rouault, ICML
                2018) under our own name and our own specification.  Stage 1
                picks theta = K - 2f clients by repeated Krum on the K x K
                squared distances of the weight keys (pairdist2_rows, computed
                once: the Gram on the matrix cores up to 128 clients, its
                tile-pair form fedagg_pairgram2_wide_f32 from 129 to 1024 in
                the tiers of PAIRGRAM_WIDE_AUTO, the exact kernel when
                gram_condition says so or above 1024; the rounds re-score on
                the host, bulyan_select).  Stage
                2 averages, per coordinate of EVERY key, the beta = theta - 2f
                selected values nearest the coordinate's median
                (fedagg_nearmedian_mean_f32, specified in include/fedagg.h:
                one launch over the whole row up to 128 selected clients,
                fedagg_nearmedian_mean_wide_f32 from 129 to 1024 in the tiers
                of NEARMEDIAN_WIDE_AUTO, the same rule in torch ops above
                that).  K >= 4f + 3.

"fltrust"       Not in FedML: FLTrust (Cao, Fang, Liu, Gong, NDSS 2021) under
                our own specification (fltrust, fltrust_coeffs), the one rule
                here that assumes no honest majority and the one that judges
                direction, not distance.  The server trains a root model of
                its own from the global model on clean data; each client's
                update is weighted by the ReLU of its cosine with the root
                update and rescaled to the root update's norm.  Two passes
                over the rows: every client's inner product with the root
                update and its squared norm over the weight keys
                (fedagg_dotnorm2_f32: exact products, fp64 sums, one read),
                then global + sum c_i (x_i - global) over EVERY key for the
                trusted clients only (fedagg_wsum_diff_f32); 2(K + 1) doubles
                on the host in between.  Any number of clients.

"krum", "multikrum"
                KrumDefense.defend_before_aggregation (krum_defense.py:28-60):
                the K x K squared distances of the clients' weight vectors are
                one pairdist2_rows call (fedagg_pairdist2_f32, or by default
                the centred Gram on the matrix cores: fedagg_pairgram2_f32 up
                to 128 clients, fedagg_pairgram2_wide_f32 from 129 to 1024);
                the scores (sum of the K - f - 2 smallest; in numpy above 128
                clients, bit for bit the reference's loop), their fp32 argsort
                and the returned sub-list of the ORIGINAL (sample_num, dict)
                tuples follow the reference on the host (K numbers).

"slsgd"         SLSGDDefense (slsgd_defense.py:28-67): option 2 trims by
                sample count before aggregation (the trimmed-mean helper);
                on aggregation FedAvg, then (1 - alpha) g + alpha avg per key,
                a two-row weighted sum on the GPU (our FedAvg kernel: the
                same two roundings per element as torch).

"cclip"         CClipDefense (cclip_defense.py:21-80): bucketization =
                FedAvg over consecutive groups of bucket_size clients (our
                kernel, one launch per group), one bucket mean drawn by
                np.random.randint as the guess, each mean's distance to it
                (fedagg_dist2_f32), the scaled differences (mean - guess) *
                min(1, tau / dist) over every key (fedagg_scale_diff_f32);
                after aggregation guess + aggregate (a two-row sum).

"norm_diff_clipping"
                NormDiffClippingDefense.defend_before_aggregation
                (norm_diff_clipping_defense.py:20-54): every client's distance
                to the global model is one fedagg_dist2_f32 launch, the clipped
                weights (x - g) / max(1, norm / bound) + g one
                fedagg_clip_diff_f32 launch; non-weight keys stay the client's
                own tensors, as in the reference.

Distances: the reference forms fp32 differences and takes an fp32 torch.norm
(.item(), then ** 2 for Krum).  The kernels sum the exact squares of the same
fp32 differences in fp64; the host rounds the root to fp32 as the reference's
norm does.  torch's own fp32 reduction may land one ulp away from that, so a
Krum selection matches the reference's except between clients whose fp32
scores are within an ulp (exact ties, e.g. mirror-image clients, can go either
way in the reference too: its reduction order depends on the thread count),
and a clipped client's divisor can differ in its last bit.
"""
from __future__ import annotations

import logging
import math
from collections import OrderedDict
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _native as nat
from . import kernels as kn
from .bucket import ClientBucket

DEFENSE_WISE_MEDIAN = "wise_median"
DEFENSE_TRIMMED_MEAN = "trimmed_mean"
DEFENSE_KRUM = "krum"
DEFENSE_MULTIKRUM = "multikrum"
DEFENSE_NORM_DIFF_CLIPPING = "norm_diff_clipping"
DEFENSE_SLSGD = "slsgd"
DEFENSE_CCLIP = "cclip"
DEFENSE_ROBUST_LEARNING_RATE = "robust_learning_rate"
DEFENSE_WEAK_DP = "weak_dp"
DEFENSE_WISE_TRIMMED_MEAN = "wise_trimmed_mean"  # not a FedML defense type: Yin et al.'s per-coordinate rule
DEFENSE_GEOMED = "geomed"  # not a FedML defense type either: our geometric median (RFA), see geometric_median
DEFENSE_WISE_BULYAN = "wise_bulyan"  # not FedML's "bulyan": our specification of Bulyan, see bulyan
DEFENSE_FLTRUST = "fltrust"  # not a FedML defense type: FLTrust (Cao et al.), see fltrust
SUPPORTED = (DEFENSE_WISE_MEDIAN, DEFENSE_TRIMMED_MEAN, DEFENSE_KRUM, DEFENSE_MULTIKRUM, DEFENSE_NORM_DIFF_CLIPPING,
             DEFENSE_SLSGD, DEFENSE_CCLIP, DEFENSE_ROBUST_LEARNING_RATE, DEFENSE_WEAK_DP, DEFENSE_WISE_TRIMMED_MEAN,
             DEFENSE_GEOMED, DEFENSE_WISE_BULYAN, DEFENSE_FLTRUST)
# FedMLDefender constructs these but lists them under none of its
# before / on / after-aggregation hooks (fedml_defender.py:131-154), so the
# plugin path aggregates as if no defense were set; they act only through
# FedMLDefender.defend (the MPI FedAvg aggregator)
PLUGIN_IDENTITY = (DEFENSE_ROBUST_LEARNING_RATE, DEFENSE_WEAK_DP)


def is_weight_param(k: str) -> bool:
    """core/security/common/utils.py:16-21."""
    return "running_mean" not in k and "running_var" not in k and "num_batches_tracked" not in k


def _one_device(d0, wkeys, what: str) -> None:
    """The defenses gather every client's weight keys into one bucket on one
    GPU.  A round that a MultiDeviceBucket spread over several GPUs (because
    it did not fit one) would be pulled back onto one device and fail with an
    out-of-memory error deep inside; say what happened instead."""
    devs = {d0[k].device for k in wkeys if isinstance(d0[k], torch.Tensor) and d0[k].is_cuda}
    if len(devs) > 1:
        raise NotImplementedError(
            f"{what}: the clients' weight keys are spread over {len(devs)} GPUs "
            f"({', '.join(sorted(str(d) for d in devs))}; a multi-device round, fedml_amd.multidev); the defense "
            f"gathers every client onto one GPU, so run it on a round that fits one device")


def _client_dicts(raw_client_grad_list, want=None) -> Tuple[list, list]:
    """The clients' dicts and client 0's keys (those `want` accepts; None: all),
    each looked up in every other client: KeyError for a missing key."""
    dicts = [raw_client_grad_list[i][1] for i in range(len(raw_client_grad_list))]
    keys = [k for k in dicts[0].keys() if want is None or want(k)]
    for d in dicts[1:]:
        for k in keys:
            d[k]
    return dicts, keys


def _rows_to_dict(rows, keys, on_device: bool, clone: bool) -> "OrderedDict":
    """Finished rows of a staging bucket as a new OrderedDict in `keys` order.
    rows: (group, row) pairs, consumed one by one (a generator may launch the
    next group's kernel only then).  Host inputs get host tensors back; clone:
    every key its own storage instead of a view of the row.  Call on the
    bucket's device: the stream is drained before the bucket goes out of scope."""
    res = {}
    for g, row in rows:
        if not on_device:
            row = row.cpu()
        for k, o, n, shp in zip(g.keys, g.offsets, g.numels, g.shapes):
            res[k] = row[o:o + n].view(shp).clone() if clone else row[o:o + n].view(shp)
    if on_device:
        torch.cuda.current_stream().synchronize()
    return OrderedDict((k, res[k]) for k in keys)


def median_f32(d_ptrs: torch.Tensor, K: int, N: int, out: torch.Tensor) -> None:
    """Coordinate-wise lower median of K fp32 device rows (fedagg_median_f32)."""
    kn._require_cuda(out, "median_f32")
    nat.check(nat.lib().fedagg_median_f32(d_ptrs.data_ptr(), K, N, out.data_ptr(), 0, nat.stream_handle()),
              "median_f32")


_MEDIAN_DT = {torch.float32: nat.DT_F32, torch.bfloat16: nat.DT_BF16, torch.float16: nat.DT_F16}


def median_rows(d_ptrs: torch.Tensor, K: int, N: int, out: torch.Tensor, aligned: bool = False) -> None:
    """Coordinate-wise lower median of K device rows of out's dtype (fp32, bf16
    or f16; fedagg_median).  aligned: every row pointer and out are 16-byte
    aligned (bucket rows are), which lets 16-bit rows use the packed kernel."""
    kn._require_cuda(out, "median")
    if out.dtype not in _MEDIAN_DT:
        raise TypeError(f"median: fp32, bf16 or f16 rows (got {out.dtype})")
    flags = nat.FEDAGG_ALIGNED16 if aligned and out.data_ptr() % 16 == 0 else 0
    nat.check(nat.lib().fedagg_median(_MEDIAN_DT[out.dtype], d_ptrs.data_ptr(), K, N, out.data_ptr(), flags,
                                      nat.stream_handle()), "median")


def median_row_dtype(dts) -> torch.dtype:
    """The dtype of the median's rows for weight keys of dtypes `dts`:
    vectorize_weight's torch.cat promotes to one dtype, fp32 when any key is
    fp32 or two float widths meet (bf16 + f16 -> fp32; the 16-bit keys widen
    exactly, integer weights ride as fl32(v)), or a 16-bit model's own bf16 /
    f16.  The median is one of its inputs, so selecting in the promoted dtype
    is exact.  Other mixes (all-integer, 16-bit floats with integers) raise."""
    dts = set(dts)
    floats = dts & {torch.float32, torch.bfloat16, torch.float16}
    ints = dts - floats
    if (torch.float32 in floats or len(floats) > 1) and ints <= {torch.int64, torch.int32, torch.bool}:
        return torch.float32
    if dts in ({torch.bfloat16}, {torch.float16}):
        return next(iter(dts))
    raise NotImplementedError("wise_median on the GPU takes fp32 or mixed-width float weights (integer keys "
                              f"allowed), or all-bf16 / all-f16 weights (got {sorted(map(str, dts))})")


def coordinate_wise_median(raw_client_grad_list: List[Tuple[float, "OrderedDict"]], device=None
                           ) -> "OrderedDict":
    """CoordinateWiseMedianDefense.defend_on_aggregation on the GPU."""
    K = len(raw_client_grad_list)
    dicts, wkeys = _client_dicts(raw_client_grad_list, is_weight_param)  # the keys of vectorize_weight
    t0 = dicts[0][wkeys[0]] if wkeys else None
    if t0 is None:
        raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")  # vectorize_weight on no keys
    _one_device(dicts[0], wkeys, "wise_median")
    dev = t0.device if t0.is_cuda else (torch.device(device) if device is not None else
                                        torch.device("cuda", torch.cuda.current_device()))
    dts = {dicts[0][k].dtype for k in wkeys}
    row_dt = median_row_dtype(dts)
    floats = dts & {torch.float32, torch.bfloat16, torch.float16}
    with torch.cuda.device(dev):
        # 16-bit keys of a promoted model are declared fp32: put() widens them
        layout = [(k, tuple(dicts[0][k].shape),
                   row_dt if dicts[0][k].dtype in floats else dicts[0][k].dtype) for k in wkeys]
        bucket = ClientBucket(layout, K, dev)
        for i in range(K):
            bucket.put(i, {k: dicts[i][k] for k in wkeys}, 1)
        bucket.sync_ingest()
        g = bucket.groups[row_dt]
        row_med = torch.empty(g.padded, dtype=row_dt, device=dev)
        median_rows(g.d_ptrs, K, g.length, row_med, aligned=True)  # bucket rows are 256-B aligned
        # the reference's vector: weight keys back to back, no alignment gaps
        vec = torch.cat([row_med[o:o + n] for o, n in zip(g.offsets, g.numels)]) if g.keys else row_med[:0]
        if not t0.is_cuda:
            vec = vec.cpu()
    # coordinate_wise_median_defense.py:36-44: walk ALL of client 0's keys
    index = 0
    (num0, averaged_params) = raw_client_grad_list[0]
    for k, params in list(averaged_params.items()):
        median_params = vec[index:index + params.numel()].view(params.size())
        index += params.numel()
        averaged_params[k] = median_params
    return averaged_params


def compute_a_score(local_sample_number):
    """common/utils.py:231-233 (the score is the sample count)."""
    return local_sample_number


def trimmed_mean(model_list: Sequence, trimmed_num: int) -> list:
    """common/utils.py:213-228: a stable sort by score, then both ends dropped."""
    temp = [(n, grad, compute_a_score(n)) for n, grad in model_list]
    temp.sort(key=lambda x: x[2])
    temp = temp[trimmed_num: len(model_list) - trimmed_num]
    return [(t[0], t[1]) for t in temp]


def trimmed_mean_before_aggregation(raw_client_grad_list: Sequence, beta: float) -> list:
    """CoordinateWiseTrimmedMeanDefense.defend_before_aggregation (:19-26)."""
    if beta > 1 / 2 or beta < 0:
        raise ValueError("the bound of beta is [0, 1/2)")
    return trimmed_mean(raw_client_grad_list, int(beta * len(raw_client_grad_list)))


# ---- coordinate-wise trimmed mean (csrc/trimmed.hip) ---------------------------

TRIMMED_MAX_CLIENTS = nat.TRIMMED_MAX_CLIENTS  # fedagg_trimmed_mean holds up to 128 clients


def trimmed_mean_rows(d_ptrs: torch.Tensor, K: int, N: int, trim: int, out: torch.Tensor,
                      aligned: bool = False) -> None:
    """Coordinate-wise trimmed mean of K device rows of out's dtype (fp32, bf16
    or f16; fedagg_trimmed_mean, specified in include/fedagg.h): per column
    the `trim` smallest and `trim` largest values dropped, the rest summed in
    fp32 in ascending order and divided by their number.  K <= 128.  aligned
    is accepted for symmetry with median_rows; the kernel has one form."""
    kn._require_cuda(out, "trimmed_mean")
    if out.dtype not in _MEDIAN_DT:
        raise TypeError(f"trimmed_mean: fp32, bf16 or f16 rows (got {out.dtype})")
    flags = nat.FEDAGG_ALIGNED16 if aligned and out.data_ptr() % 16 == 0 else 0
    nat.check(nat.lib().fedagg_trimmed_mean(_MEDIAN_DT[out.dtype], d_ptrs.data_ptr(), K, N, trim, out.data_ptr(),
                                            flags, nat.stream_handle()), "trimmed_mean")


# fedagg_trimmed_mean_wide holds up to 1024 clients (csrc/trimmed_wide.hip)
TRIMMED_WIDE_MAX_CLIENTS = nat.TRIMMED_WIDE_MAX_CLIENTS
# The K tiers of the wide kernel (K <= tier) that coordinate_wise_trimmed_mean
# hands to it above 128 clients: those where its median time beat
# trimmed_mean_rows_torch's by more than the larger min-max spread of the two
# (GEOMED_AUTO_FUSED's rule; tools/trimmed_wide_probe.py ->
# profiles/trimmed_wide_probe.json, NOTES.md §5b); a tier that did not win
# takes the torch path.  Measured at 4,194,304 columns, kernel and torch path
# launched alternately on the same rows, median of 10, torch / kernel (fp32,
# bf16; K = the full tier, then a padded K); spreads under 0.24 ms for the
# kernel and under 70 ms for the torch path:
#   tier  256: 63.1x, 63.4x (K = 256: 1.40 ms against 88 ms); 53.4x, 44.0x (K = 200)
#   tier  512: 50.8x, 52.5x (K = 512: 4.03 ms against 205 ms); 40.1x, 37.6x (K = 384)
#   tier 1024: 43.8x, 47.1x (K = 1024: 11.8 ms against 516 ms); 34.3x, 34.3x (K = 700)
TRIMMED_WIDE_AUTO = {256: True, 512: True, 1024: True}


def _tier_auto(table: dict, max_clients: int, K: int) -> bool:
    """A *_WIDE_AUTO table's entry for K clients; False above max_clients."""
    return K <= max_clients and table[min(t for t in table if K <= t)]


def trimmed_wide_auto(K: int) -> bool:
    """Whether coordinate_wise_trimmed_mean runs the wide kernel for K clients
    above TRIMMED_MAX_CLIENTS (TRIMMED_WIDE_AUTO)."""
    return _tier_auto(TRIMMED_WIDE_AUTO, TRIMMED_WIDE_MAX_CLIENTS, K)


def trimmed_mean_rows_wide(d_ptrs: torch.Tensor, K: int, N: int, trim: int, out: torch.Tensor) -> None:
    """Coordinate-wise trimmed mean of K <= 1024 device rows of out's dtype
    (fp32, bf16 or f16; fedagg_trimmed_mean_wide): trimmed_mean_rows's
    operation, bit for bit, with the column spread over 4 or 8 lanes.  One
    kernel form for every alignment."""
    kn._require_cuda(out, "trimmed_mean_wide")
    if out.dtype not in _MEDIAN_DT:
        raise TypeError(f"trimmed_mean_wide: fp32, bf16 or f16 rows (got {out.dtype})")
    nat.check(nat.lib().fedagg_trimmed_mean_wide(_MEDIAN_DT[out.dtype], d_ptrs.data_ptr(), K, N, trim,
                                                 out.data_ptr(), 0, nat.stream_handle()), "trimmed_mean_wide")


def _order_keys(x: torch.Tensor) -> torch.Tensor:
    """int32 keys of fp32 values whose integer order is the kernels' total
    order (-inf < negatives < -0 < +0 < positives < +inf < every NaN).  The
    map is its own inverse on non-NaN values; the NaN key maps back to a NaN."""
    b = x.view(torch.int32)
    k = b ^ ((b >> 31) & 0x7FFFFFFF)
    return torch.where(torch.isnan(x), torch.full_like(k, 0x7FFFFFFF), k)


def trimmed_mean_rows_torch(rows, trim: int, chunk_cols: "int | None" = None) -> torch.Tensor:
    """The specification of fedagg_trimmed_mean in torch ops, on any device
    and for any K: the slow path above 128 clients.  rows: a (K, N) tensor or
    a list of K rows of N elements (fp32, bf16 or f16).  Per column chunk the
    order keys are sorted, mapped back to values and added in ascending rank
    order, one fp32 add per kept rank, then divided by their count (a tensor
    divisor: torch turns a division by a Python scalar into a multiplication
    by its reciprocal on the GPU).  chunk_cols: columns per chunk (default:
    temporaries of about 1 GiB)."""
    K = len(rows)
    if K < 1:
        raise ValueError("trimmed mean of no rows")
    if trim < 0 or K - 2 * trim < 1:
        raise ValueError(f"trim = {trim} leaves no value of K = {K}")
    r0 = rows[0]
    if r0.dtype not in _MEDIAN_DT:
        raise TypeError(f"trimmed_mean: fp32, bf16 or f16 rows (got {r0.dtype})")
    N = r0.numel()
    if chunk_cols is None:
        chunk_cols = max(1, (1 << 30) // (32 * K))  # widened values, keys, sorted keys and sort indices
    out = torch.empty(N, dtype=r0.dtype, device=r0.device)
    count = torch.full((1,), float(K - 2 * trim), dtype=torch.float32, device=r0.device)
    for c0 in range(0, N, chunk_cols):
        c1 = min(N, c0 + chunk_cols)
        x = rows[:, c0:c1] if isinstance(rows, torch.Tensor) else torch.stack([r[c0:c1] for r in rows])
        keys = torch.sort(_order_keys(x.float().contiguous()), dim=0).values
        s = (keys ^ ((keys >> 31) & 0x7FFFFFFF)).view(torch.float32)
        acc = s[trim].clone()  # the chain starts from the value, not from 0.0
        for r in range(trim + 1, K - trim):
            acc += s[r]
        out[c0:c1] = (acc / count).to(r0.dtype)  # one rounding to the row dtype, nearest-even
    return out


def trimmed_row_dtype(dts) -> "torch.dtype | None":
    """The dtype of the float keys' rows for keys of dtypes `dts`, by
    median_row_dtype's rule: fp32 when any key is fp32 or two float widths
    meet (the 16-bit keys widen exactly), else the model's own bf16 / f16;
    None for a model of integer keys only.  Integer / bool keys sit in an fp32
    row as fl32(v) whatever the floats are."""
    dts = set(dts)
    floats = dts & {torch.float32, torch.bfloat16, torch.float16}
    if not dts - floats <= {torch.int64, torch.int32, torch.bool}:
        raise NotImplementedError("wise_trimmed_mean on the GPU takes fp32, bf16 and f16 keys and int64 / int32 / "
                                  f"bool buffers (got {sorted(map(str, dts))})")
    if not floats:
        return None
    return torch.float32 if torch.float32 in floats or len(floats) > 1 else next(iter(floats))


def coordinate_wise_trimmed_mean(raw_client_grad_list: List[Tuple[float, "OrderedDict"]], beta: float, device=None
                                 ) -> "OrderedDict":
    """The coordinate-wise trimmed mean of Yin et al. over the clients' dicts:
    every coordinate of EVERY key (BatchNorm statistics and counters too)
    drops its int(beta * K) smallest and largest client values and averages
    the rest: fedagg_trimmed_mean up to 128 clients, fedagg_trimmed_mean_wide
    from 129 to 1024 (in the tiers of TRIMMED_WIDE_AUTO), for the float keys'
    row and the fp32 row of the integer keys alike, and
    trimmed_mean_rows_torch above that; the three agree bit for bit.  Sample counts are ignored, as by the median.  Returns a new
    OrderedDict in client 0's key order, on the inputs' device; integer keys
    come back fp32, as FedMLAggOperator.agg returns them.  No client dict is
    modified."""
    if beta < 0 or beta >= 1 / 2:
        raise ValueError("the bound of beta is [0, 1/2)")
    K = len(raw_client_grad_list)
    trim = int(beta * K)
    if K - 2 * trim < 1:
        raise ValueError(f"beta = {beta} trims every one of {K} clients")
    dicts, keys = _client_dicts(raw_client_grad_list)
    if not keys:
        return OrderedDict()
    _one_device(dicts[0], keys, "wise_trimmed_mean")
    t0 = dicts[0][keys[0]]
    dev = t0.device if t0.is_cuda else (torch.device(device) if device is not None else
                                        torch.device("cuda", torch.cuda.current_device()))
    floats = {torch.float32, torch.bfloat16, torch.float16}
    row_dt = trimmed_row_dtype(dicts[0][k].dtype for k in keys)
    with torch.cuda.device(dev):
        # 16-bit keys of a promoted model are declared fp32: put() widens them
        layout = [(k, tuple(dicts[0][k].shape), row_dt if dicts[0][k].dtype in floats else dicts[0][k].dtype)
                  for k in keys]
        bucket = ClientBucket(layout, K, dev)
        for i in range(K):
            bucket.put(i, {k: dicts[i][k] for k in keys}, 1)
        bucket.sync_ingest()

        def rows():
            for g in bucket.groups.values():  # the float keys' row; integer keys in an fp32 row
                if K <= TRIMMED_MAX_CLIENTS:
                    row = torch.empty(g.padded, dtype=g.dtype, device=dev)
                    trimmed_mean_rows(g.d_ptrs, K, g.length, trim, row, aligned=True)
                elif trimmed_wide_auto(K):
                    row = torch.empty(g.padded, dtype=g.dtype, device=dev)
                    trimmed_mean_rows_wide(g.d_ptrs, K, g.length, trim, row)
                else:
                    row = trimmed_mean_rows_torch(g.rows[:, :g.length], trim)
                yield g, row

        return _rows_to_dict(rows(), keys, t0.is_cuda, clone=False)


# ---- distance-based defenses (csrc/robust.hip) ---------------------------------

def weight_chunks(group, chunk: int, device, absolute: bool = True) -> Tuple[torch.Tensor, int]:
    """Device (start, length) table of a row group's weight-key columns, runs
    of adjacent keys merged, split into pieces of at most `chunk` columns.

    absolute (default): cut at multiples of `chunk` in the row (a run's first
    piece is shorter), so pieces after the first start on whole cache lines.
    The kernels hand consecutive pieces to blocks on different XCDs; runs cut
    from their 16-byte aligned start made every boundary line a fetch for
    both blocks: dist2 at 1.036x the algorithmic bytes (1.009x now), Krum's
    Gram 5.58 ms (5.39 now) at config 3.  False: cuts from each run's start
    (tools' A/B baseline)."""
    segs = []
    for key, off, n in zip(group.keys, group.offsets, group.numels):
        if n == 0 or not is_weight_param(key):
            continue
        if segs and segs[-1][0] + segs[-1][1] == off:
            segs[-1][1] += n
        else:
            segs.append([off, n])
    starts, lens = [], []
    for off, n in segs:
        if absolute:
            st = np.concatenate([np.array([off], dtype=np.int64),
                                 np.arange((off // chunk + 1) * chunk, off + n, chunk, dtype=np.int64)])
        else:
            st = np.arange(off, off + n, chunk, dtype=np.int64)
        starts.append(st)
        lens.append(np.append(st[1:], off + n) - st)
    if not starts:
        return torch.zeros(2, dtype=torch.int64, device=device), 0
    tab = np.stack([np.concatenate(starts), np.concatenate(lens)], axis=1).ravel()
    return kn.upload_i64(tab.tolist(), device), len(tab) // 2


def _work(kind: int, K: int, n_chunks: int, device) -> torch.Tensor:
    n = int(nat.lib().fedagg_robust_work_len(kind, K, n_chunks))
    if n < 0:
        raise nat.FedAggNativeError("fedagg_robust_work_len: bad sizes")
    return torch.empty(max(n, 1), dtype=torch.float64, device=device)


GRAM_MAX_CLIENTS = 128  # fedagg_pairgram2_f32 holds up to 128 clients
# "auto" keeps the Gram's distances only while (|c_i|^2 + |c_j|^2) / D_ij stays
# at or below this for every pair (c = the rows centred on the client mean):
# iid clients sit near 1; one update scaled far away inflates every honest
# client's |c|^2 and triggers the exact kernel (gram_condition)
GRAM_MAX_CONDITION = 8.0


def gram_condition(D: np.ndarray) -> float:
    """max over client pairs i != j of (|c_i|^2 + |c_j|^2) / D_ij, where c_i is
    client i's row minus the mean of the K rows: the factor by which the
    centred Gram's rounding error (~1e-7 (|c_i|^2 + |c_j|^2) per entry) exceeds
    a relative error of D_ij itself.  The centred norms come from D alone
    (double centring of a squared-distance matrix: |c_i|^2 = mean_j D_ij -
    sum D / (2 K^2)).  inf when two distinct clients are at distance 0, or when any distance
    or centred norm is not finite (an inf client, squares beyond fp32)."""
    K = D.shape[0]
    if K < 2:
        return 0.0
    D = np.asarray(D, dtype=np.float64)
    if not np.all(np.isfinite(D)):  # an inf / NaN client, or squares beyond fp32: only the exact kernel copes
        return float("inf")
    c2 = np.maximum(D.sum(axis=1) / K - D.sum() / (2.0 * K * K), 0.0)
    if not np.all(np.isfinite(c2)):
        return float("inf")
    num = c2[:, None] + c2[None, :]
    off = ~np.eye(K, dtype=bool)
    d, s = D[off], num[off]
    if np.any((d <= 0) & (s > 0)):
        return float("inf")
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(d > 0, s / np.where(d > 0, d, 1.0), 0.0)
    m = float(r.max())
    return m if np.isfinite(m) else float("inf")


# fedagg_pairgram2_wide_f32 holds up to 1024 clients (csrc/robust.hip)
PAIRGRAM_WIDE_MAX_CLIENTS = nat.PAIRGRAM_WIDE_MAX_CLIENTS
# The K tiers (K <= tier) in which pairdist2_rows' "auto" runs "gram_wide"
# above 128 clients: those where its median time, the centre pass included,
# beat the exact kernel's by more than the larger min-max spread of the two
# (TRIMMED_WIDE_AUTO's rule; tools/pairgram_wide_probe.py ->
# profiles/pairgram_wide_probe.json, NOTES.md §5c).  A tier that
# did not win stays False and "auto" keeps the exact kernel there.  Measured
# at 4,194,304 fp32 columns, both launched alternately on the same rows,
# median of 10 (min - max), exact / gram_wide; a tier is True when its full K
# and its padded K both pass  gap = exact - gram_wide > larger spread:
#   tier  256: K = 256  8.06 (8.01 - 8.26) / 4.06 (4.03 - 4.10) ms: gap 4.00 > 0.26;
#              K = 200  7.76 (7.72 - 7.84) / 3.95 (3.86 - 3.98): gap 3.81 > 0.13
#   tier  512: K = 512  29.74 (29.60 - 29.92) / 14.37 (14.30 - 14.45): gap 15.37 > 0.32;
#              K = 384  17.59 (17.40 - 17.71) / 8.44 (8.41 - 8.49): gap 9.15 > 0.30
#   tier 1024: K = 1024 111.53 (111.09 - 111.61) / 50.74 (50.41 - 51.37): gap 60.79 > 0.96;
#              K = 700  54.61 (54.10 - 54.96) / 25.52 (25.39 - 25.65): gap 29.09 > 0.86
# (2.0x - 2.2x; the centre pass, 0.5 - 2.6 ms, is inside gram_wide's time.)
PAIRGRAM_WIDE_AUTO = {256: True, 512: True, 1024: True}


def pairgram_wide_auto(K: int) -> bool:
    """Whether pairdist2_rows' "auto" runs the wide Gram for K clients above
    GRAM_MAX_CLIENTS (PAIRGRAM_WIDE_AUTO)."""
    return _tier_auto(PAIRGRAM_WIDE_AUTO, PAIRGRAM_WIDE_MAX_CLIENTS, K)


def client_mean_row(d_ptrs: torch.Tensor, K: int, length: int, device, aligned: bool = False) -> torch.Tensor:
    """The mean of K fp32 device rows over their first `length` columns: one
    pass of the FedAvg kernel with device weights 1/K (the wide Gram's centre).
    aligned: every row is 16-byte aligned (the kernel's vector path)."""
    out = torch.empty(max(length, 1), dtype=torch.float32, device=device)
    d_w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=device)
    kn.wsum_ptrs(torch.float32, d_ptrs, d_w, K, length, out, aligned)
    return out


def pairdist2_rows(d_ptrs: torch.Tensor, K: int, chunks: torch.Tensor, n_chunks: int, device,
                   method: str = "auto", *, length: "int | None" = None,
                   center: "torch.Tensor | None" = None, aligned: bool = False) -> torch.Tensor:
    """K x K fp64 squared distances of K fp32 device rows over the chunked
    columns.  method "exact": the reference's fp32 differences, squared and
    summed on the VALU (fedagg_pairdist2_f32); "gram": the centred Gram on the
    bf16 matrix cores with an exact three-way split (fedagg_pairgram2_f32,
    K <= 128); "gram_wide": the same Gram by 64-client tile pairs
    (fedagg_pairgram2_wide_f32, K <= 1024), centred on `center`, an fp32 device
    row indexed like the client rows, or, when center is None, on the mean of
    the rows' first `length` columns (client_mean_row; length must then cover
    every chunk; aligned: the rows are 16-byte aligned, as bucket rows are, so
    that pass takes its vector path); "auto": gram when K allows it (same Krum
    selections, ~3x faster at config 3), gram_wide above 128 clients in the
    tiers of PAIRGRAM_WIDE_AUTO when a length or a centre is given,
    and the result is well conditioned (``gram_condition`` <=
    GRAM_MAX_CONDITION), else the exact kernel: one far-away update (the case
    Krum exists for) moves the client mean, and the honest clients' distances
    would then carry the Gram's error scaled by that update's norm."""
    if method not in ("auto", "gram", "gram_wide", "exact"):
        raise ValueError(f"pair distance method {method!r}: 'auto', 'gram', 'gram_wide' or 'exact'")
    gram = method == "gram" or (method == "auto" and K <= GRAM_MAX_CLIENTS)
    if gram and K > GRAM_MAX_CLIENTS:
        raise ValueError(f"the Gram pair kernel holds at most {GRAM_MAX_CLIENTS} clients (K = {K})")
    wide = method == "gram_wide" or (method == "auto" and not gram and pairgram_wide_auto(K)
                                     and (length is not None or center is not None))
    if wide and K > PAIRGRAM_WIDE_MAX_CLIENTS:
        raise ValueError(f"the wide Gram pair kernel holds at most {PAIRGRAM_WIDE_MAX_CLIENTS} clients (K = {K})")
    if wide and center is None and length is None:
        raise ValueError("pair distance method 'gram_wide' needs the rows' length or a centre row")
    out = torch.empty((K, K), dtype=torch.float64, device=device)
    if wide:
        if center is None:
            center = client_mean_row(d_ptrs, K, length, device, aligned)
        elif center.dtype != torch.float32 or not center.is_cuda:
            raise TypeError("pair distance centre: an fp32 device row")
        work = _work(nat.WORK_PAIRGRAM_WIDE, K, n_chunks, device)
        nat.check(nat.lib().fedagg_pairgram2_wide_f32(d_ptrs.data_ptr(), K, center.data_ptr(), chunks.data_ptr(),
                                                      n_chunks, out.data_ptr(), work.data_ptr(), work.numel(),
                                                      nat.stream_handle()), "pairgram2_wide")
    else:
        work = _work(nat.WORK_PAIRGRAM if gram else nat.WORK_PAIRDIST2, K, n_chunks, device)
        fn = nat.lib().fedagg_pairgram2_f32 if gram else nat.lib().fedagg_pairdist2_f32
        nat.check(fn(d_ptrs.data_ptr(), K, chunks.data_ptr(), n_chunks, out.data_ptr(), work.data_ptr(), work.numel(),
                     nat.stream_handle()), "pairgram2" if gram else "pairdist2")
    if (gram or wide) and method == "auto" and gram_condition(out.cpu().numpy()) > GRAM_MAX_CONDITION:
        return pairdist2_rows(d_ptrs, K, chunks, n_chunks, device, "exact")
    return out


def dist2_rows(d_ptrs: torch.Tensor, K: int, ref: "torch.Tensor | None", chunks: torch.Tensor, n_chunks: int,
               device) -> torch.Tensor:
    """K fp64 squared distances of K fp32 device rows to `ref` (None: norms)
    over the chunked columns (fedagg_dist2_f32)."""
    out = torch.empty(K, dtype=torch.float64, device=device)
    work = _work(nat.WORK_DIST2, K, n_chunks, device)
    nat.check(nat.lib().fedagg_dist2_f32(d_ptrs.data_ptr(), K, ref.data_ptr() if ref is not None else None,
                                         chunks.data_ptr(), n_chunks, out.data_ptr(), work.data_ptr(),
                                         work.numel(), nat.stream_handle()), "dist2")
    return out


def fp32_norm(sq: float) -> float:
    """The reference's `torch.norm(fp32 vector).item()`: an fp32 root."""
    return float(np.float32(np.sqrt(sq)))


def _weight_bucket(dicts: Sequence, what: str, device=None):
    """ClientBucket of the clients' weight keys (vectorize_weight's keys, in
    client 0's order) and its fp32 row group."""
    wkeys = [k for k in dicts[0].keys() if is_weight_param(k)]
    if not wkeys:
        raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")  # vectorize_weight on no keys
    for d in dicts[1:]:
        for k in wkeys:
            d[k]  # KeyError for a missing key, as the reference's walk would fail
    dts = {dicts[0][k].dtype for k in wkeys}
    if dts != {torch.float32}:
        raise NotImplementedError(f"{what} on the GPU takes fp32 weight keys (got {sorted(map(str, dts))})")
    _one_device(dicts[0], wkeys, what)
    t0 = dicts[0][wkeys[0]]
    dev = t0.device if t0.is_cuda else (torch.device(device) if device is not None else
                                        torch.device("cuda", torch.cuda.current_device()))
    layout = [(k, tuple(dicts[0][k].shape), torch.float32) for k in wkeys]
    with torch.cuda.device(dev):
        bucket = ClientBucket(layout, len(dicts), dev)
        for i, d in enumerate(dicts):
            bucket.put(i, {k: d[k] for k in wkeys}, 1)
        bucket.sync_ingest()
    return bucket, bucket.groups[torch.float32], wkeys, dev


def krum_scores(D: np.ndarray, byzantine_client_num: int) -> list:
    """KrumDefense._compute_krum_score (krum_defense.py:47-60) over the K x K
    squared distances: each distance enters as the reference's
    `norm.item() ** 2`, the K - f - 2 smallest are summed in ascending order."""
    K = D.shape[0]
    if K > KRUM_SCORES_LOOP_MAX_CLIENTS:
        scores = krum_scores_numpy(D, byzantine_client_num)
        if scores is not None:
            return scores
    return krum_scores_loop(D, byzantine_client_num)


# krum_scores runs its Python double loop up to this many clients and numpy
# above: the loop makes K (K - 1) fp32_norm calls, about a million (seconds)
# at K = 1024, beside a distance kernel that takes milliseconds
KRUM_SCORES_LOOP_MAX_CLIENTS = 128


def krum_scores_loop(D: np.ndarray, byzantine_client_num: int) -> list:
    """krum_scores as the reference writes it: the path up to
    KRUM_SCORES_LOOP_MAX_CLIENTS clients and the reference of the numpy form."""
    K = D.shape[0]
    scores = []
    for i in range(K):
        dists = [fp32_norm(D[i, j]) ** 2 for j in range(K) if j != i]
        dists.sort()
        scores.append(sum(dists[0:K - byzantine_client_num - 2]))
    return scores


def krum_scores_numpy(D: np.ndarray, byzantine_client_num: int) -> "list | None":
    """krum_scores_loop's scores, bit for bit, in numpy: the fp32 root, its
    square in float64 (exact: 24 x 24 bits), each row without its diagonal
    entry sorted, and the first K - f - 2 added one after the other in
    ascending order (cumsum adds sequentially, as sum() over the list does).
    None when a root is NaN (a NaN or negative entry): list.sort() and np.sort
    place NaN differently, so the loop decides those."""
    K = D.shape[0]
    with np.errstate(invalid="ignore"):
        R = np.sqrt(np.asarray(D, dtype=np.float64)).astype(np.float32).astype(np.float64)
    if np.isnan(R).any():
        return None
    R = (R * R)[~np.eye(K, dtype=bool)].reshape(K, K - 1)
    R.sort(axis=1)
    head = R[:, 0:K - byzantine_client_num - 2]  # the list slice's semantics, negative counts included
    if head.shape[1] == 0:
        return [0] * K
    return np.cumsum(head, axis=1)[:, -1].tolist()


def krum_before_aggregation(raw_client_grad_list: Sequence, byzantine_client_num: int, krum_param_m: int = 1,
                            device=None, method: str = "auto") -> list:
    """KrumDefense.defend_before_aggregation (krum_defense.py:28-45): the
    krum_param_m lowest-scoring clients' original tuples, in score order.
    method: the pair-distance kernel (pairdist2_rows)."""
    num_client = len(raw_client_grad_list)
    if not 2 * byzantine_client_num + 2 <= num_client - krum_param_m:
        raise ValueError("byzantine_client_num conflicts with requirements in Krum: "
                         "2 * byzantine_client_num + 2 < client number - krum_param_m")
    bucket, g, _, dev = _weight_bucket([item[1] for item in raw_client_grad_list], "krum", device)
    with torch.cuda.device(dev):
        chunks, n_chunks = weight_chunks(g, nat.PAIR_CHUNK, dev)
        D = pairdist2_rows(g.d_ptrs, num_client, chunks, n_chunks, dev, method, length=g.length,
                           aligned=True).cpu().numpy()
    scores = krum_scores(D, byzantine_client_num)
    score_index = torch.argsort(torch.Tensor(scores)).tolist()[0:krum_param_m]
    return [raw_client_grad_list[i] for i in score_index]


def krum_param_m(args) -> int:
    """KrumDefense.__init__ (krum_defense.py:19-25)."""
    m = getattr(args, "krum_param_m", None)
    return m if isinstance(m, int) else 1


def norm_diff_clipping_before_aggregation(raw_client_grad_list: Sequence, global_model, norm_bound: float,
                                          device=None) -> list:
    """NormDiffClippingDefense.defend_before_aggregation
    (norm_diff_clipping_defense.py:20-54): every client's weights pulled to
    within norm_bound of the global model; new dicts, the client's own
    tensors for non-weight keys."""
    K = len(raw_client_grad_list)
    if K == 0:
        return []
    dicts = [item[1] for item in raw_client_grad_list]
    bucket, g, wkeys, dev = _weight_bucket(dicts, "norm_diff_clipping", device)
    with torch.cuda.device(dev):
        gb = ClientBucket([(k, tuple(dicts[0][k].shape), torch.float32) for k in wkeys], 1, dev)
        gb.put(0, {k: global_model[k] for k in wkeys}, 1)
        gb.sync_ingest()
        ref = gb.groups[torch.float32].rows[0]
        chunks, n_chunks = weight_chunks(g, nat.DIST_CHUNK, dev)
        sq = dist2_rows(g.d_ptrs, K, ref, chunks, n_chunks, dev).cpu().numpy()
        divs = [max(1, fp32_norm(s) / norm_bound) for s in sq]  # _get_clipped_norm_diff
        d_div = kn.upload_f32(divs, dev)
        out = torch.empty_like(g.rows)
        d_dst = kn.upload_i64([out[i].data_ptr() for i in range(K)], dev)
        nat.check(nat.lib().fedagg_clip_diff_f32(g.d_ptrs.data_ptr(), K, ref.data_ptr(), d_div.data_ptr(),
                                                 g.rows.shape[1], d_dst.data_ptr(), nat.stream_handle()),
                  "clip_diff")
        if not dicts[0][wkeys[0]].is_cuda:
            out = out.cpu()  # host clients get host tensors back, as the reference returns
        else:
            torch.cuda.current_stream().synchronize()  # the staging buckets go out of scope
    pos = {k: j for j, k in enumerate(g.keys)}
    new_list = []
    for i, (sample_num, local_w) in enumerate(raw_client_grad_list):
        clipped = OrderedDict()
        for k, v in local_w.items():  # _get_clipped_weights (:44-54)
            if is_weight_param(k):
                j = pos[k]
                clipped[k] = out[i, g.offsets[j]:g.offsets[j] + g.numels[j]].view(v.size())
            else:
                clipped[k] = v
        new_list.append((sample_num, clipped))
    return new_list


# ---- SLSGD / CClip (two-row and grouped weighted sums, scaled differences) ------

def _like_input(out: "OrderedDict[str, torch.Tensor]", on_device: bool) -> "OrderedDict[str, torch.Tensor]":
    if on_device:
        return out
    return OrderedDict((k, t.cpu()) for k, t in out.items())


def _float_bucket(template, capacity: int, what: str, device=None):
    """A ClientBucket for fp32 models (integer buffers allowed: they sit in
    the fp32 row as fl32(v), the dtype torch's int64 * float yields), laid out
    by `template`'s keys, on its device (or `device` for host tensors)."""
    keys = list(template.keys())
    layout = [(k, tuple(template[k].shape), template[k].dtype) for k in keys]
    dts = {dt for _, _, dt in layout}
    if not dts <= {torch.float32, torch.int64, torch.int32} or torch.float32 not in dts:
        raise NotImplementedError(f"{what} on the GPU takes fp32 models (integer buffers allowed), got "
                                  f"{sorted(map(str, dts))}")
    t0 = template[keys[0]]
    dev = t0.device if t0.is_cuda else (torch.device(device) if device is not None else
                                        torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(dev):
        bucket = ClientBucket(layout, capacity, dev)
    return bucket, dev


def _put_float(bucket, slot: int, d, keys) -> None:
    """put() of the layout's keys; an integer tensor under a float key is
    converted by put (fl32(v), torch's rounding of int64 -> float32)."""
    bucket.put(slot, OrderedDict((k, d[k]) for k in keys), 1)


def mix_two(first, second, w_first: float, w_second: float, device=None) -> "OrderedDict[str, torch.Tensor]":
    """fl(w_first * first[k]) + fl(w_second * second[k]) for every key of
    `second`, as torch computes `(1 - alpha) * g[k] + alpha * avg[k]` (two
    rows of our weighted-sum kernel; integer keys enter as fl32(v))."""
    keys = list(second.keys())
    on_dev = second[keys[0]].is_cuda
    bucket, dev = _float_bucket(second, 2, "slsgd / cclip", device)
    with torch.cuda.device(dev):
        _put_float(bucket, 0, first, keys)
        _put_float(bucket, 1, second, keys)
        bucket.sync_ingest()
        outs = bucket.new_outputs()
        bucket.reduce_into(outs, [w_first, w_second], 2)
        res = OrderedDict((k, t.clone()) for k, t in bucket.unflatten(outs).items())
    return _like_input(res, on_dev)


def slsgd_alpha_check(alpha: float) -> None:
    """SLSGDDefense.__init__ (slsgd_defense.py:29-33)."""
    if alpha > 1 or alpha < 0:
        raise ValueError("the bound of alpha is [0, 1]")


def slsgd_before_aggregation(raw_client_grad_list: Sequence, b: int, option_type: int) -> list:
    """SLSGDDefense.defend_before_aggregation (slsgd_defense.py:36-52)."""
    if b > math.ceil(len(raw_client_grad_list) / 2) - 1 or b < 0:
        raise ValueError("the bound of b is [0, {}])".format(math.ceil(len(raw_client_grad_list) / 2) - 1))
    if option_type != 1 and option_type != 2:
        raise Exception("Such option type does not exist!")
    if option_type == 2:
        raw_client_grad_list = trimmed_mean(raw_client_grad_list, b)
    return list(raw_client_grad_list)


def slsgd_on_aggregation(avg_params, global_model, alpha: float, device=None):
    """SLSGDDefense.defend_on_aggregation (slsgd_defense.py:54-67) after the
    base FedAvg: (1 - alpha) * global + alpha * avg for every key."""
    return mix_two(global_model, avg_params, 1 - alpha, alpha, device)


def cclip_tau(args) -> float:
    """CClipDefense.__init__ (cclip_defense.py:22-26)."""
    tau = getattr(args, "tau", None)
    return tau if type(tau) in [int, float] and tau > 0 else 10


def cclip_before_aggregation(raw_client_grad_list: Sequence, tau: float, bucket_size: int, device=None):
    """CClipDefense.defend_before_aggregation (cclip_defense.py:30-56).
    Returns (new list, initial guess dict) -- the guess is kept for
    defend_after_aggregation, as the reference's defender object does."""
    K = len(raw_client_grad_list)
    dicts = [item[1] for item in raw_client_grad_list]
    on_dev = next(iter(dicts[0].values())).is_cuda
    bucket, dev = _float_bucket(dicts[0], K, "cclip", device)
    keys = list(dicts[0].keys())
    with torch.cuda.device(dev):
        for i, d in enumerate(dicts):
            bucket.put(i, {k: d[k] for k in keys}, 1)
        bucket.sync_ingest()
    g = bucket.groups[torch.float32]
    B = math.ceil(K / bucket_size)
    with torch.cuda.device(dev):
        means = torch.empty((B, g.rows.shape[1]), dtype=torch.float32, device=dev)
        nums = []
        for b in range(B):  # Bucket.bucketization (common/bucket.py:6-28)
            lo = b * bucket_size
            cn = min(bucket_size, K - lo)
            sample_num = 0
            for i in range(cn):
                sample_num += raw_client_grad_list[lo + i][0]
            w = [raw_client_grad_list[lo + i][0] / sample_num for i in range(cn)]
            kn.wsum_ptrs(torch.float32, g.d_ptrs[lo:lo + cn], kn.weights_for(w, torch.float32, dev), cn, g.length,
                         means[b], True)
            nums.append(sample_num)
        guess_idx = np.random.randint(0, B)  # _compute_an_initial_guess (:61-62), the global numpy RNG
        guess = means[guess_idx]
        m_ptrs = kn.upload_i64([means[b].data_ptr() for b in range(B)], dev)
        chunks, n_chunks = weight_chunks(g, nat.DIST_CHUNK, dev)
        sq = dist2_rows(m_ptrs, B, guess, chunks, n_chunks, dev).cpu().numpy()
        scores = [min(1, tau / (fp32_norm(v) + 1e-8)) for v in sq]  # _compute_cclip_score (:64-71)
        d_sc = kn.upload_f32([float(x) for x in scores], dev)
        out = torch.empty_like(means)
        d_dst = kn.upload_i64([out[b].data_ptr() for b in range(B)], dev)
        nat.check(nat.lib().fedagg_scale_diff_f32(m_ptrs.data_ptr(), B, guess.data_ptr(), d_sc.data_ptr(),
                                                  g.rows.shape[1], d_dst.data_ptr(), nat.stream_handle()),
                  "scale_diff")
        views = [bucket_view(g, out[b]) for b in range(B)]
        guess_dict = bucket_view(g, guess)
    new_list = [(nums[b], _like_input(views[b], on_dev)) for b in range(B)]
    return new_list, _like_input(guess_dict, on_dev)


def bucket_view(group, row: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
    """Per-key views of one fp32 row of a group (keys in layout order)."""
    return OrderedDict((k, row[o:o + n].view(shp))
                       for k, o, n, shp in zip(group.keys, group.offsets, group.numels, group.shapes))


def cclip_after_aggregation(global_model, initial_guess, device=None):
    """CClipDefense.defend_after_aggregation (cclip_defense.py:57-60):
    guess[k] + global[k] for every key (a two-row sum, weights 1 and 1:
    fl(1 * x) = x, so one rounding, as torch's add)."""
    return mix_two(initial_guess, global_model, 1.0, 1.0, device)


# ---- Robust learning rate (sign agreement per coordinate) ----------------------

def robust_learning_rate(raw_client_grad_list: Sequence, robust_threshold, base_aggregation_func=None,
                         device=None) -> "OrderedDict[str, torch.Tensor]":
    """RobustLearningRateDefense.run (robust_learning_rate_defense.py:35-62) on
    the GPU: ONE pass over the clients' rows computes the FedAvg chain and the
    per-coordinate sum of their signs (fedagg_wsum_rlr_f32), and the key
    becomes lr * avg with lr = +1 where |Σ sign| >= threshold, else -1.
    As in the reference: threshold 0 hands the list to base_aggregation_func,
    the weights are n_i / Σn (ZeroDivisionError at Σn = 0), a missing key
    raises KeyError, and client 0's dict is returned with its keys rebound
    (integer keys come back fp32: torch's fp32 average times the integer lr)."""
    if robust_threshold == 0:
        return base_aggregation_func(raw_client_grad_list)
    total = 0
    for n, _ in raw_client_grad_list:
        total += n
    K = len(raw_client_grad_list)
    ws = [n / total for n, _ in raw_client_grad_list]
    num0, avg_params = raw_client_grad_list[0]
    keys = list(avg_params.keys())
    on_dev = avg_params[keys[0]].is_cuda
    bucket, dev = _float_bucket(avg_params, K, "robust_learning_rate", device)
    with torch.cuda.device(dev):
        for i, (_, d) in enumerate(raw_client_grad_list):
            _put_float(bucket, i, d, keys)
        bucket.sync_ingest()
        outs = bucket.new_outputs()
        g = bucket.groups[torch.float32]
        kn.wsum_rlr_ptrs(g.d_ptrs, kn.weights_for(ws, torch.float32, dev), K, g.length,
                         float(np.float32(robust_threshold)), outs[torch.float32], True)
        res = _like_input(OrderedDict((k, t.clone()) for k, t in bucket.unflatten(outs).items()), on_dev)
    for k in keys:
        avg_params[k] = res[k]
    return avg_params


class RobustLearningRateDefense:
    """Drop-in for FedML's RobustLearningRateDefense (the object
    FedMLDefender.init builds for defense_type "robust_learning_rate"):
    FedMLDefender.defend -> run() aggregates on the GPU."""

    def __init__(self, config):
        self.robust_threshold = config.robust_threshold
        self.server_learning_rate = 1

    def run(self, raw_client_grad_list, base_aggregation_func=None, extra_auxiliary_info=None):
        return robust_learning_rate(raw_client_grad_list, self.robust_threshold, base_aggregation_func)

    def defend_before_aggregation(self, raw_client_grad_list, extra_auxiliary_info=None):
        return None  # BaseDefenseMethod's default (defense_base.py:11-24)

    def defend_on_aggregation(self, raw_client_grad_list, base_aggregation_func=None, extra_auxiliary_info=None):
        return None

    def get_malicious_client_idxs(self):
        return []


# ---- geometric median (csrc/geomed.hip) ----------------------------------------

GEOMED_MAX_CLIENTS = nat.GEOMED_MAX_CLIENTS  # fedagg_wsum_dist2_f32 holds up to 128 clients
# a client whose squared norm over the weight columns exceeds this (or is not
# finite) is dropped by the screen: what is left has every |value| <= 2^126, so
# every |z| <= 2^126 and no fp32 difference x - z can overflow
GEOMED_MAX_NORM2 = 2.0 ** 252
# "auto": the K tiers of the fused kernel (K <= tier) where its median time
# beat the unfused pair's by more than the larger min-max spread of the two
# (tools/geomed_probe.py -> profiles/geomed_probe.json, NOTES.md §7b); a tier
# that did not win would take the unfused pair.  Measured at 25,610,152
# columns: 1.79x to 1.92x at every tier, spreads under 0.05 ms
GEOMED_AUTO_FUSED = {8: True, 16: True, 32: True, 64: True, 128: True}


def geomed_auto_fused(K: int) -> bool:
    """Whether "auto" runs the fused kernel for K clients (GEOMED_AUTO_FUSED)."""
    if K > GEOMED_MAX_CLIENTS:
        return False
    return GEOMED_AUTO_FUSED[min(t for t in GEOMED_AUTO_FUSED if K <= t)]


class NonFiniteDistance(ArithmeticError):
    """A Weiszfeld pass returned a non-finite squared distance."""

    def __init__(self, iteration: int, D):
        super().__init__(f"non-finite squared distance in Weiszfeld pass {iteration}")
        self.iteration = iteration
        self.D = D


class GeomedInfo:
    """What geometric_median did: `iterations` weight updates (iterations + 1
    passes), the `objective` f_0 .. f_T, the final float64 `weights` (0 for a
    dropped client), the indices of the clients `dropped` by the screen and
    the `method` the passes ran with."""

    def __init__(self, iterations: int, objective: list, weights=None, dropped=(), method: str = ""):
        self.iterations = iterations
        self.objective = objective
        self.weights = weights
        self.dropped = list(dropped)
        self.method = method

    def __repr__(self):
        return (f"GeomedInfo(iterations={self.iterations}, objective={self.objective}, dropped={self.dropped}, "
                f"method={self.method!r})")


def wsum_dist2_rows(d_ptrs: torch.Tensor, d_w, K: int, chunks: torch.Tensor, n_chunks: int, z: torch.Tensor,
                    device) -> torch.Tensor:
    """One fused Weiszfeld pass (fedagg_wsum_dist2_f32): the weighted sum of
    the K fp32 device rows into z's chunked columns and, returned, the K fp64
    squared distances of the rows to it over those columns.  d_w: K device
    floats or kernels.HostWeights.  K <= GEOMED_MAX_CLIENTS."""
    kn._require_cuda(z, "wsum_dist2")
    if z.dtype != torch.float32:
        raise TypeError("wsum_dist2: fp32 rows and output")
    out = torch.empty(K, dtype=torch.float64, device=device)
    work = _work(nat.WORK_WSUM_DIST2, K, n_chunks, device)
    flags = nat.FEDAGG_ALIGNED16 if z.data_ptr() % 16 == 0 else 0  # the kernel has one form for every alignment
    if isinstance(d_w, kn.HostWeights):
        flags |= nat.FEDAGG_HOST_WEIGHTS
    nat.check(nat.lib().fedagg_wsum_dist2_f32(d_ptrs.data_ptr(), d_w.data_ptr(), K, chunks.data_ptr(), n_chunks,
                                              z.data_ptr(), out.data_ptr(), work.data_ptr(), work.numel(), flags,
                                              nat.stream_handle()), "wsum_dist2")
    return out


def weiszfeld_step_unfused(d_ptrs: torch.Tensor, d_w, K: int, N: int, chunks: torch.Tensor, n_chunks: int,
                           z: torch.Tensor, device, aligned: bool = False) -> torch.Tensor:
    """The same pass from the two kernels that were there before: fedagg_wsum_f32
    over the first N columns of the rows into z, then fedagg_dist2_f32 with
    ref = z over the chunked columns (two reads of the rows).  The path above
    GEOMED_MAX_CLIENTS clients, and what the fused kernel is checked and timed
    against.  aligned: the rows are 16-byte aligned (bucket rows are)."""
    kn.wsum_ptrs(torch.float32, d_ptrs, d_w, K, N, z, aligned)
    return dist2_rows(d_ptrs, K, z, chunks, n_chunks, device)


def weiszfeld_step_torch(rows, w32, cols=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The specification of one Weiszfeld pass in torch ops, on any device.
    rows: a (K, N) fp32 tensor or a list of K rows; w32: K weights (rounded to
    fp32 here); cols: index tensor of the columns that count (None: all).
    Returns (z, D): z[e] = the chain fl(x_0 w_0), fl(acc + fl(x_i w_i)) client
    by client in fp32 for EVERY column, D[i] = the fp64 sum over cols of the
    exact squares of the fp32 differences x_i - z."""
    K = len(rows)
    if K < 1:
        raise ValueError("Weiszfeld step over no rows")
    dev = rows[0].device
    w = torch.tensor([float(v) for v in w32], dtype=torch.float64).to(torch.float32).to(dev)
    z = rows[0] * w[0]
    for i in range(1, K):
        z = z + rows[i] * w[i]  # two roundings: torch's eager mul, then add
    zc = z if cols is None else z[cols]
    D = torch.empty(K, dtype=torch.float64, device=dev)
    for i in range(K):
        d = ((rows[i] if cols is None else rows[i][cols]) - zc).double()
        D[i] = (d * d).sum()
    return z, D


def geomed_weights(D, a, nu: float) -> np.ndarray:
    """The Weiszfeld weights in float64: d_i = sqrt(D_i), b_i = a_i /
    max(nu, d_i), w_i = b_i / sum(b), the sum taken left to right."""
    d = np.sqrt(np.asarray(D, dtype=np.float64))
    b = [float(ai) / max(float(nu), float(di)) for ai, di in zip(a, d)]
    total = 0.0
    for x in b:
        total += x
    return np.array([x / total for x in b], dtype=np.float64)


def geometric_median_loop(step, a, nu: float = 1e-6, maxiter: int = 16, ftol: float = 1e-6):
    """Smoothed Weiszfeld iteration (Pillutla et al., RFA), independent of
    where a pass runs.  step(w32) -> (z, D): the weighted sum of the clients
    with the K Python floats w32 (already fp32 values) and the K squared
    distances to it (array-like, float64).  a: the clients' sample weights
    n_i / sum(n).

        w = a
        for t = 0, 1, ...:
            z_t, D = step(fl32(w))
            f_t = sum_i a_i sqrt(D_i)            (float64, left to right)
            stop if t == maxiter or (t >= 1 and |f_{t-1} - f_t| <= ftol f_t)
            w = geomed_weights(D, a, nu)

    so maxiter updates cost maxiter + 1 passes and maxiter = 0 is FedAvg.
    Returns (z_T, w_T, GeomedInfo): the last pass's sum, the float64 weights
    it was formed with, and iterations = T with the objectives f_0 .. f_T.
    Raises NonFiniteDistance when a pass returns a non-finite D."""
    if maxiter < 0:
        raise ValueError("maxiter must be >= 0")
    a = [float(x) for x in a]
    w = np.array(a, dtype=np.float64)
    objective = []
    t = 0
    while True:
        z, D = step([float(np.float32(x)) for x in w])
        D = np.asarray(D, dtype=np.float64)
        if not np.all(np.isfinite(D)):
            raise NonFiniteDistance(t, D)
        f = 0.0
        for ai, di in zip(a, np.sqrt(D)):
            f += ai * float(di)
        objective.append(f)
        if t == maxiter or (t >= 1 and abs(objective[-2] - f) <= ftol * f):
            return z, w, GeomedInfo(t, objective, w)
        w = geomed_weights(D, a, nu)
        t += 1


def geometric_median_screened(make_step, norms2, a, nu: float = 1e-6, maxiter: int = 16, ftol: float = 1e-6):
    """geometric_median_loop with the lazy screen for non-finite clients.
    make_step(alive) -> the step over the clients `alive` (indices into a);
    norms2() -> the K clients' squared norms over the columns that count.
    Honest rounds run the loop once and pay nothing.  If pass 0 returns a
    non-finite D, every client whose squared norm is non-finite or above
    GEOMED_MAX_NORM2 is dropped (a warning names them), a is renormalised over
    the rest and the loop restarts; ValueError if the dropped clients hold half
    or more of the sample weight (the breakdown point), RuntimeError if D is
    non-finite after that.  Returns (z, w, info, alive): w has K entries (0 for
    a dropped client), info.dropped lists the dropped indices."""
    K = len(a)
    a = [float(x) for x in a]
    alive = list(range(K))
    try:
        z, w, info = geometric_median_loop(make_step(alive), a, nu, maxiter, ftol)
        return z, w, info, alive
    except NonFiniteDistance as e:
        if e.iteration != 0:
            raise RuntimeError(f"geomed: {e} although pass 0 was finite") from e
    n2 = np.asarray(norms2(), dtype=np.float64)
    dropped = [i for i in range(K) if not np.isfinite(n2[i]) or n2[i] > GEOMED_MAX_NORM2]
    if not dropped:
        raise RuntimeError("geomed: non-finite distances, yet every client's norm is finite and below 2^126")
    alive = [i for i in range(K) if i not in set(dropped)]
    lost = 0.0
    for i in dropped:
        lost += a[i]
    kept = 0.0
    for i in alive:
        kept += a[i]
    if lost >= kept:
        raise ValueError(f"geomed: clients {dropped} sent non-finite or overflowing updates and hold "
                         f"{lost:.3f} of the sample weight: half or more, the geometric median's breakdown point")
    logging.warning("geomed: dropped clients %s (non-finite or overflowing updates, %.3f of the sample weight)",
                    dropped, lost)
    a2 = [a[i] / kept for i in alive]
    try:
        z, w2, info = geometric_median_loop(make_step(alive), a2, nu, maxiter, ftol)
    except NonFiniteDistance as e:
        raise RuntimeError(f"geomed: {e} after the non-finite clients {dropped} were dropped") from e
    w = np.zeros(K, dtype=np.float64)
    w[alive] = w2
    info.weights = w
    info.dropped = dropped
    return z, w, info, alive


def geometric_median(raw_client_grad_list: List[Tuple[float, "OrderedDict"]], nu: float = 1e-6, maxiter: int = 16,
                     ftol: float = 1e-6, device=None, method: str = "auto", return_info: bool = False):
    """The geometric median of the clients' updates (RFA, Pillutla et al.; the
    "geomed" defense, ours: FedML's own "geometric_median" / "RFA" loop is not
    reproduced): the point minimising sum_i a_i |x_i - z| over the weight keys,
    a_i = n_i / sum(n), by geometric_median_loop.  Each pass is one
    fedagg_wsum_dist2_f32 launch ("fused", up to 128 clients) or fedagg_wsum_f32
    + fedagg_dist2_f32 ("unfused"); "auto" takes the fused kernel where it was
    measured faster (GEOMED_AUTO_FUSED) and the pair elsewhere and above 128
    clients.  One K-double device-to-host copy per pass, as Krum's.

    fp32 models (integer buffers allowed, entering as fl32(v)).  Distances run
    over the weight keys; the result's weight keys are the last pass's z, and
    BatchNorm statistics and counters are the weighted sum with the same final
    weights (one more fedagg_wsum_f32 over the row after a fused run, whose
    weight columns are bit-identical to z).  Non-finite clients are screened
    lazily (geometric_median_screened); a NaN in a non-weight key is not
    looked at and passes through into that key, as in FedAvg.  Returns a new
    OrderedDict in client 0's key order on the inputs' device (integer keys
    come back fp32); no client dict is modified.  return_info: also the
    GeomedInfo."""
    if method not in ("auto", "fused", "unfused"):
        raise ValueError(f"geomed method {method!r}: 'auto', 'fused' or 'unfused'")
    K = len(raw_client_grad_list)
    if K < 1:
        raise ValueError("geomed: no clients")
    dicts, keys = _client_dicts(raw_client_grad_list)
    total = 0
    for n, _ in raw_client_grad_list:
        total += n
    a = [n / total for n, _ in raw_client_grad_list]  # ZeroDivisionError at sum(n) = 0, as FedAvg
    if not keys:
        return (OrderedDict(), GeomedInfo(0, [], np.array(a), (), method)) if return_info else OrderedDict()
    if method == "fused" and K > GEOMED_MAX_CLIENTS:
        raise ValueError(f"the fused Weiszfeld kernel holds at most {GEOMED_MAX_CLIENTS} clients (K = {K})")
    _one_device(dicts[0], keys, "geomed")
    on_dev = dicts[0][keys[0]].is_cuda
    bucket, dev = _float_bucket(dicts[0], K, "geomed", device)
    fused = method == "fused" or (method == "auto" and geomed_auto_fused(K))
    with torch.cuda.device(dev):
        for i, d in enumerate(dicts):
            _put_float(bucket, i, d, keys)
        bucket.sync_ingest()
        g = bucket.groups[torch.float32]
        chunks, n_chunks = weight_chunks(g, nat.DIST_CHUNK, dev)
        z = torch.zeros(g.padded, dtype=torch.float32, device=dev)
        tables = {}

        def table(alive):
            if len(alive) == K:
                return g.d_ptrs
            if tuple(alive) not in tables:
                tables[tuple(alive)] = kn.upload_i64([g.rows[i].data_ptr() for i in alive], dev)
            return tables[tuple(alive)]

        def make_step(alive):
            ptrs, Ka = table(alive), len(alive)

            def step(w32):
                d_w = kn.weights_for(w32, torch.float32, dev)
                if fused:
                    D = wsum_dist2_rows(ptrs, d_w, Ka, chunks, n_chunks, z, dev)
                else:
                    D = weiszfeld_step_unfused(ptrs, d_w, Ka, g.length, chunks, n_chunks, z, dev, aligned=True)
                return z, D.cpu().numpy()
            return step

        def norms2():
            return dist2_rows(g.d_ptrs, K, None, chunks, n_chunks, dev).cpu().numpy()

        _, w, info, alive = geometric_median_screened(make_step, norms2, a, nu, maxiter, ftol)
        info.method = "fused" if fused else "unfused"
        row = z
        others = any(n > 0 and not is_weight_param(k) for k, n in zip(g.keys, g.numels))
        if fused and others:
            # BatchNorm statistics and counters with the robust weights; the
            # weight columns come out bit-identical to z
            row = torch.empty_like(z)
            w32 = [float(np.float32(w[i])) for i in alive]
            kn.wsum_ptrs(torch.float32, table(alive), kn.weights_for(w32, torch.float32, dev), len(alive), g.length,
                         row, True)
        out = _rows_to_dict([(g, row)], keys, on_dev, clone=True)
    return (out, info) if return_info else out


# ---- FLTrust (csrc/robust.hip: dotnorm2, wsum_diff) -----------------------------

def dotnorm2_rows(d_ptrs: torch.Tensor, K: int, ref: torch.Tensor, direction: torch.Tensor, chunks: torch.Tensor,
                  n_chunks: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dot, n2): for K fp32 device rows, the fp64 inner products of x_i - ref
    with direction - ref and the fp64 squared norms of x_i - ref over the
    chunked columns, in one read of the rows (fedagg_dotnorm2_f32).  Two views
    of one 2K-double device tensor."""
    kn._require_cuda(ref, "dotnorm2")
    if ref.dtype != torch.float32 or direction.dtype != torch.float32:
        raise TypeError("dotnorm2: fp32 rows")
    out = torch.empty(2 * K, dtype=torch.float64, device=device)
    work = _work(nat.WORK_DOTNORM2, K, n_chunks, device)
    nat.check(nat.lib().fedagg_dotnorm2_f32(d_ptrs.data_ptr(), K, ref.data_ptr(), direction.data_ptr(),
                                            chunks.data_ptr(), n_chunks, out.data_ptr(), work.data_ptr(),
                                            work.numel(), nat.stream_handle()), "dotnorm2")
    return out[:K], out[K:]


def wsum_diff_rows(d_ptrs: "torch.Tensor | None", d_c: "torch.Tensor | None", K: int, ref: torch.Tensor, N: int,
                   out: torch.Tensor) -> None:
    """out[:N] = ref + the chain of c_i (x_i - ref) over K fp32 device rows
    (fedagg_wsum_diff_f32; K == 0: out = ref, no table needed).  d_c: K device
    floats.  out aliases no input."""
    kn._require_cuda(out, "wsum_diff")
    if ref.dtype != torch.float32 or out.dtype != torch.float32:
        raise TypeError("wsum_diff: fp32 rows and output")
    nat.check(nat.lib().fedagg_wsum_diff_f32(d_ptrs.data_ptr() if K > 0 else None, d_c.data_ptr() if K > 0 else None,
                                             K, ref.data_ptr(), N, out.data_ptr(), nat.stream_handle()), "wsum_diff")


def dotnorm2_rows_torch(rows, ref, direction, cols=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The specification of fedagg_dotnorm2_f32 in torch ops, on any device.
    rows: a (K, N) fp32 tensor or a list of K rows; cols: index tensor of the
    columns that count (None: all).  Returns (dot, n2), K float64 each: the
    fp64 sums of the exact products of the fp32 differences a_i = x_i - ref
    with b = direction - ref, and of a_i with itself (torch's own summation
    order: equal to the kernel's up to fp64 rounding, not bit for bit)."""
    K = len(rows)
    dev = ref.device
    rc = ref if cols is None else ref[cols]
    b = ((direction if cols is None else direction[cols]) - rc).double()
    dot = torch.empty(K, dtype=torch.float64, device=dev)
    n2 = torch.empty(K, dtype=torch.float64, device=dev)
    for i in range(K):
        a = ((rows[i] if cols is None else rows[i][cols]) - rc).double()
        dot[i] = (a * b).sum()
        n2[i] = (a * a).sum()
    return dot, n2


def wsum_diff_rows_torch(rows, c32, ref) -> torch.Tensor:
    """The specification of fedagg_wsum_diff_f32 in torch ops, on any device:
    acc = fl(c_0 fl(x_0 - ref)), acc = fl(acc + fl(c_i fl(x_i - ref))) client by
    client, ref + acc at the end; ref itself (a copy) for no rows.  c32: K
    coefficients (rounded to fp32 here).  Separate mul and add, each rounded
    once, as the kernel's."""
    K = len(rows)
    if K == 0:
        return ref.clone()
    c = torch.tensor([float(v) for v in c32], dtype=torch.float64).to(torch.float32).to(ref.device)
    acc = (rows[0] - ref) * c[0]
    for i in range(1, K):
        acc = acc + (rows[i] - ref) * c[i]
    return ref + acc


def fltrust_coeffs(dot, n2, nb2, lr: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """FLTrust's trust scores and rebuild coefficients in float64, from the K
    inner products dot_i = <a_i, b>, the K squared norms n2_i = |a_i|^2 and
    nb2 = |b|^2 (a_i = client i's update, b the server's root update):

        n_i = sqrt(n2_i), n_b = sqrt(nb2), cos_i = dot_i / (n_i n_b)
        TS_i = cos_i if cos_i is finite and > 0 else 0        (ReLU)
        S = sum TS_i, left to right
        c_i = lr TS_i n_b / (n_i S)                            (0 where TS_i = 0)

    so sum_i c_i a_i is the trust-weighted mean of the updates rescaled to the
    root update's norm, times lr.  A client with a NaN, an inf, an overflowing
    difference or a zero update has a non-finite or non-positive cosine and
    gets trust 0.  S == 0: every c_i = 0 (the caller keeps the global model).
    ValueError when n_b is 0 or not finite: a root update that does not move
    cannot judge anything.  Returns (trust, coeffs), K float64 each."""
    dot = np.asarray(dot, dtype=np.float64)
    n2 = np.asarray(n2, dtype=np.float64)
    with np.errstate(all="ignore"):
        nb = float(np.sqrt(np.float64(nb2)))
        if not math.isfinite(nb) or nb == 0.0:
            raise ValueError(f"fltrust: the root update's norm is {nb}: the server's root model must differ from the "
                             f"global model by a finite amount")
        n = np.sqrt(n2)
        cos = dot / (n * nb)
    trust = np.array([float(v) if math.isfinite(v) and v > 0 else 0.0 for v in cos], dtype=np.float64)
    S = 0.0
    for v in trust:
        S += float(v)
    coeffs = np.zeros(len(trust), dtype=np.float64)
    if S > 0:
        for i, ts in enumerate(trust):
            if ts > 0:
                coeffs[i] = float(lr) * ts * nb / (float(n[i]) * S)
    return trust, coeffs


class FLTrustInfo:
    """What fltrust did: the float64 cosines `cos` (NaN for a non-finite or
    zero update), the `trust` scores, the fp32 `coeffs` the rebuild used (as
    float64 values, 0 for an untrusted client), the indices `trusted` and the
    root update's norm `root_norm`."""

    def __init__(self, cos, trust, coeffs, trusted, root_norm: float):
        self.cos = cos
        self.trust = trust
        self.coeffs = coeffs
        self.trusted = list(trusted)
        self.root_norm = root_norm

    def __repr__(self):
        return f"FLTrustInfo(trusted={self.trusted}, root_norm={self.root_norm!r}, trust={self.trust})"


def fltrust(raw_client_grad_list: List[Tuple[float, "OrderedDict"]], global_model, root_model, lr: float = 1.0,
            device=None, return_info: bool = False):
    """FLTrust (Cao, Fang, Liu, Gong, NDSS 2021; the "fltrust" defense, ours:
    FedML has none).  global_model: the server's current model g; root_model:
    g after the server's own local training on its clean root data this round.
    Client i's update a_i = x_i - g is weighted by the ReLU of its cosine with
    the root update b = r - g and rescaled to |b|:

        out = g + sum_i c_i (x_i - g),   (trust, c) = fltrust_coeffs(<a_i, b>, |a_i|^2, |b|^2, lr)

    No honest majority is assumed; sample counts are ignored.  Cosines run
    over the weight keys (is_weight_param, client 0's order) in one
    fedagg_dotnorm2_f32 pass over the K client rows and the root row (row K:
    its two sums are |b|^2), then one copy of 2(K + 1) doubles to the host.
    The rebuild runs over EVERY key (BatchNorm statistics and counters too) in
    one fedagg_wsum_diff_f32 pass over the trusted clients only, in ascending
    order: an untrusted client's row is not in the pointer table, so its NaNs
    are never read.  No trusted client (S == 0): a warning, and the result is g.

    fp32 models (integer buffers allowed, entering as fl32(v) and coming back
    fp32).  KeyError for a key of client 0 missing from another client, from
    global_model or from root_model; ValueError when the root update is zero or
    not finite.  Returns a new OrderedDict in client 0's key order on the
    inputs' device; no input is modified.  return_info: also the FLTrustInfo."""
    K = len(raw_client_grad_list)
    if K < 1:
        raise ValueError("fltrust: no clients")
    dicts, keys = _client_dicts(raw_client_grad_list)
    for k in keys:
        global_model[k]
        root_model[k]
    if not keys:
        info = FLTrustInfo(np.zeros(K), np.zeros(K), np.zeros(K), (), 0.0)
        return (OrderedDict(), info) if return_info else OrderedDict()
    _one_device(dicts[0], keys, "fltrust")
    on_dev = dicts[0][keys[0]].is_cuda
    bucket, dev = _float_bucket(dicts[0], K, "fltrust", device)
    gb, _ = _float_bucket(dicts[0], 2, "fltrust", dev)  # the global and the root model, laid out like the clients
    with torch.cuda.device(dev):
        for i, d in enumerate(dicts):
            _put_float(bucket, i, d, keys)
        _put_float(gb, 0, global_model, keys)
        _put_float(gb, 1, root_model, keys)
        bucket.sync_ingest()
        gb.sync_ingest()
        g, gg = bucket.groups[torch.float32], gb.groups[torch.float32]
        ref, root = gg.rows[0], gg.rows[1]
        chunks, n_chunks = weight_chunks(g, nat.DIST_CHUNK, dev)
        ptrs = kn.upload_i64([g.rows[i].data_ptr() for i in range(K)] + [root.data_ptr()], dev)
        dot, n2 = dotnorm2_rows(ptrs, K + 1, ref, root, chunks, n_chunks, dev)
        both = torch.cat([dot, n2]).cpu().numpy()  # 2(K + 1) doubles
        dot, n2 = both[:K + 1], both[K + 1:]
        trust, coeffs = fltrust_coeffs(dot[:K], n2[:K], n2[K], lr)
        nb = float(np.sqrt(n2[K]))
        with np.errstate(all="ignore"):
            cos = dot[:K] / (np.sqrt(n2[:K]) * nb)
        trusted = [i for i in range(K) if trust[i] > 0]
        c32 = np.asarray(coeffs, dtype=np.float64).astype(np.float32)
        if not trusted:
            logging.warning("fltrust: no client's update has a positive cosine with the root update; "
                            "the global model is kept")
        row = torch.empty(g.padded, dtype=torch.float32, device=dev)
        Kt = len(trusted)
        t_ptrs = kn.upload_i64([g.rows[i].data_ptr() for i in trusted], dev) if Kt else None
        d_c = kn.upload_f32([float(c32[i]) for i in trusted], dev) if Kt else None
        wsum_diff_rows(t_ptrs, d_c, Kt, ref, g.length, row)
        out = _rows_to_dict([(g, row)], keys, on_dev, clone=True)
    info = FLTrustInfo(cos, trust, c32.astype(np.float64), trusted, nb)
    return (out, info) if return_info else out


# ---- Bulyan (csrc/nearmedian.hip) ----------------------------------------------

NEARMEDIAN_MAX_CLIENTS = nat.NEARMEDIAN_MAX_CLIENTS  # fedagg_nearmedian_mean_f32 holds up to 128 rows


def nearmedian_mean_rows(d_ptrs: torch.Tensor, K: int, N: int, keep: int, out: torch.Tensor) -> None:
    """Per column the mean of the `keep` of K fp32 device rows' values nearest
    the column's lower median (fedagg_nearmedian_mean_f32, specified in
    include/fedagg.h): a contiguous rank window around the median, a tie
    between a lower and a higher candidate going to the lower, summed in fp32
    in ascending order and divided by keep.  K <= 128, 1 <= keep <= K."""
    kn._require_cuda(out, "nearmedian_mean")
    if out.dtype != torch.float32:
        raise TypeError(f"nearmedian_mean: fp32 rows (got {out.dtype})")
    nat.check(nat.lib().fedagg_nearmedian_mean_f32(d_ptrs.data_ptr(), K, N, keep, out.data_ptr(), 0,
                                                   nat.stream_handle()), "nearmedian_mean")


# fedagg_nearmedian_mean_wide_f32 holds up to 1024 rows (csrc/nearmedian_wide.hip)
NEARMEDIAN_WIDE_MAX_CLIENTS = nat.NEARMEDIAN_WIDE_MAX_CLIENTS
# The tiers of the wide kernel (theta <= tier) that bulyan hands to it above
# 128 selected clients, by TRIMMED_WIDE_AUTO's rule: those where its median
# time beat nearmedian_mean_rows_torch's by more than the larger min-max spread
# of the two (tools/nearmedian_wide_probe.py ->
# profiles/nearmedian_wide_probe.json, NOTES.md §5b); a tier that did not win
# takes the torch path.  Measured at 4,194,304 fp32 columns, kernel and torch
# path launched alternately on the same rows, median of 10, torch / kernel at
# keep = K - 2 (K // 8) and at keep = K (K = the full tier, then a padded K);
# spreads under 0.31 ms for the kernel and under 310 ms for the torch path,
# which is 111 ms to 2.4 s slower:
#   tier  256: 78.3x, 83.1x (K = 256: 1.87 ms against 147 ms); 61.5x, 64.0x (K = 200)
#   tier  512: 86.4x, 107.0x (K = 512: 4.74 ms against 410 ms); 58.8x, 70.9x (K = 384)
#   tier 1024: 107.8x, 176.1x (K = 1024: 13.4 ms against 1.44 s); 68.7x, 78.3x (K = 700)
NEARMEDIAN_WIDE_AUTO = {256: True, 512: True, 1024: True}


def nearmedian_wide_auto(theta: int) -> bool:
    """Whether bulyan runs the wide kernel for theta selected clients above
    NEARMEDIAN_MAX_CLIENTS (NEARMEDIAN_WIDE_AUTO)."""
    return _tier_auto(NEARMEDIAN_WIDE_AUTO, NEARMEDIAN_WIDE_MAX_CLIENTS, theta)


def nearmedian_mean_rows_wide(d_ptrs: torch.Tensor, K: int, N: int, keep: int, out: torch.Tensor) -> None:
    """nearmedian_mean_rows's operation, bit for bit, for K <= 1024 fp32 device
    rows (fedagg_nearmedian_mean_wide_f32): the column spread over 4 or 8
    lanes.  One kernel form for every alignment."""
    kn._require_cuda(out, "nearmedian_mean_wide")
    if out.dtype != torch.float32:
        raise TypeError(f"nearmedian_mean_wide: fp32 rows (got {out.dtype})")
    nat.check(nat.lib().fedagg_nearmedian_mean_wide_f32(d_ptrs.data_ptr(), K, N, keep, out.data_ptr(), 0,
                                                        nat.stream_handle()), "nearmedian_mean_wide")


def nearmedian_mean_rows_torch(rows, keep: int, chunk_cols: "int | None" = None) -> torch.Tensor:
    """The specification of fedagg_nearmedian_mean_f32 in torch ops, on any
    device and for any K: the slow path above 128 selected rows where the wide
    kernel does not run.  rows: a
    (K, N) fp32 tensor or a list of K fp32 rows of N elements.  Per column
    chunk the order keys are sorted and mapped back to values; with NaN
    standing as +inf the window start is lo_min plus the number of j in
    [lo_min, lo_max) whose value is strictly farther from the median than the
    value keep ranks above it (the two-pointer rule of the header, counted:
    d(s[j]) falls and d(s[j + keep]) rises with j); the keep values are then
    gathered and added one fp32 add per rank, and divided by a tensor holding
    keep (see trimmed_mean_rows_torch).  chunk_cols: columns per chunk
    (default: temporaries of about 1 GiB)."""
    K = len(rows)
    if K < 1:
        raise ValueError("nearmedian mean of no rows")
    if keep < 1 or keep > K:
        raise ValueError(f"keep = {keep} of K = {K} rows")
    r0 = rows[0]
    if r0.dtype != torch.float32:
        raise TypeError(f"nearmedian_mean: fp32 rows (got {r0.dtype})")
    N = r0.numel()
    if chunk_cols is None:
        chunk_cols = max(1, (1 << 30) // (32 * K))
    out = torch.empty(N, dtype=torch.float32, device=r0.device)
    count = torch.full((1,), float(keep), dtype=torch.float32, device=r0.device)
    r = (K - 1) // 2
    lo_min, lo_max = max(0, r - keep + 1), min(r, K - keep)
    inf = float("inf")
    for c0 in range(0, N, chunk_cols):
        c1 = min(N, c0 + chunk_cols)
        x = rows[:, c0:c1] if isinstance(rows, torch.Tensor) else torch.stack([row[c0:c1] for row in rows])
        keys = torch.sort(_order_keys(x.contiguous()), dim=0).values
        s = (keys ^ ((keys >> 31) & 0x7FFFFFFF)).view(torch.float32)
        nan = torch.isnan(s)
        nans = nan.sum(dim=0)
        sel = torch.where(nan, torch.full_like(s, inf), s)  # for the selection a NaN counts as +inf
        m = sel[r]

        def d(v):
            return torch.where(v == m, torch.zeros_like(v), (v - m).abs())

        lo = torch.full((c1 - c0,), lo_min, dtype=torch.int64, device=s.device)
        if lo_max > lo_min:
            lo += (d(sel[lo_min:lo_max]) > d(sel[lo_min + keep:lo_max + keep])).sum(dim=0)
        acc = torch.gather(s, 0, lo[None, :])[0]  # the chain starts from the value, not from 0.0
        for t in range(1, keep):
            acc += torch.gather(s, 0, (lo + t)[None, :])[0]
        res = acc / count
        res[lo + keep > K - nans] = float("nan")  # the window holds a NaN
        out[c0:c1] = res
    return out


# bulyan_select sorts every row of the distances once above this many clients;
# up to it the n x n sub-matrix is re-sorted in every round, which is as fast
# there (NOTES.md, "Bulyan above 128 selected clients")
BULYAN_PRESORT_ABOVE = 256
# rounds between two compactions of the presorted rows
_BULYAN_COMPACT_EVERY = 32


def bulyan_select(D, f: int):
    """Stage 1 of Bulyan on the host: theta = K - 2f clients by repeated Krum
    over the K x K squared distances D (computed once; every round re-scores
    from it).  R starts as all K clients; theta times, with n = |R|: for each
    i in R the score is the float64 sum, in ascending order, of the
    max(1, n - f - 2) smallest D[i][j] over j in R without i (NaN distances sort
    last, above +inf; a NaN score ranks as +inf); the lowest score is picked,
    ties going to the lowest client index, and moves from R to the selection.
    A client that sends NaN makes its row and column of D NaN: sorted last, a
    client with at most f such neighbours never sums one of them.  f = 0:
    every client, in index order, without looking at D (scores of 0).
    Returns (selected, scores): the clients in pick order and each pick's
    score in its round."""
    if f < 0:
        raise ValueError("bulyan: byzantine_client_num must be >= 0")
    K = len(D)
    if f == 0:  # only D's length is looked at
        return list(range(K)), [0.0] * K
    D = np.asarray(D, dtype=np.float64)
    theta = K - 2 * f
    if theta < 1:
        raise ValueError(f"bulyan: K = {K} clients leave no selection at f = {f}")
    if K > BULYAN_PRESORT_ABOVE:
        return _bulyan_select_presorted(D, f, theta)
    R = list(range(K))
    selected, scores = [], []
    for _ in range(theta):
        n = len(R)
        sub = D[np.ix_(R, R)].copy()
        # the client itself goes last with the NaNs: never among the n - 1 others' first c
        sub[np.arange(n), np.arange(n)] = np.nan
        c = min(max(1, n - f - 2), n - 1)
        if c < 1:  # a single client left: nothing to sum
            sc = np.zeros(n)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                sc = np.cumsum(np.sort(sub, axis=1)[:, :c], axis=1)[:, c - 1]  # sequential, ascending
        sc = np.where(np.isnan(sc), np.inf, sc)
        p = int(np.argmin(sc))  # the first of equal scores: R is ascending
        selected.append(R[p])
        scores.append(float(sc[p]))
        del R[p]
    return selected, scores


def _bulyan_select_presorted(D: np.ndarray, f: int, theta: int):
    """bulyan_select's rounds without the sort per round, bit for bit.  Every
    row of D is sorted once, NaN last and without the client itself, and kept
    as a COLUMN of `vals` (vals[j][i]: client i's j-th nearest), with the
    neighbour it belongs to in `ids`.  A round masks the entries of the client
    it removed to +0.0 and forms every score as the sequential sum down the
    columns, one vector add per sorted position (np.cumsum along a row is one
    dependent add after the other; down the columns the clients go side by
    side).  Adding +0.0 leaves a non-negative, infinite or NaN partial sum as
    it is, so a column's sum up to its c-th live entry is the sum of its c
    smallest live distances in ascending order; equal distances give equal
    sums in whichever order they stand.  The c-th live entry of column i is at
    at[i] = c - 1 + (masked entries at or before it), found from the masked
    positions since the last compaction; the rows up to the lowest at are
    added whole, the few up to the highest under at >= j.  Every
    _BULYAN_COMPACT_EVERY rounds the masked entries and the removed clients'
    columns are dropped, so at most that many rows are ragged."""
    K = len(D)
    order = np.argsort(D, axis=1, kind="stable")  # NaN last, as np.sort places it
    ids = order[order != np.arange(K)[:, None]].reshape(K, K - 1)  # the client itself is no neighbour
    vals = np.ascontiguousarray(np.take_along_axis(D, ids, axis=1).T)
    ids = np.ascontiguousarray(ids.T)
    cols = np.arange(K)  # the client of every column
    alive = np.ones(K, dtype=bool)
    where, gone = _bulyan_positions(ids), []
    selected, scores = [], []
    for _ in range(theta):
        if len(gone) >= _BULYAN_COMPACT_EVERY:
            vals, ids, cols = _bulyan_compact(vals, ids, cols, alive)
            alive = np.ones(len(cols), dtype=bool)
            where, gone = _bulyan_positions(ids), []
        R = np.flatnonzero(alive)
        n = len(R)
        c = min(max(1, n - f - 2), n - 1)
        if c < 1:  # a single client left: nothing to sum
            sc = np.zeros(n)
        else:
            # the least x with x + 1 - (masked entries at or before x) = c, from below
            at = np.full(len(cols), c - 1)
            if gone:
                masked = np.stack(gone)
                while True:
                    nxt = c - 1 + (masked <= at).sum(axis=0)
                    if np.array_equal(nxt, at):
                        break
                    at = nxt
            lo, hi = int(at[R].min()), int(at[R].max())  # a live column holds n - 1 >= c live entries
            with np.errstate(invalid="ignore", over="ignore"):
                acc = vals[0].copy()  # the chain starts from the value: 0.0 + v is v for every v a distance can be
                for j in range(1, lo + 1):
                    np.add(acc, vals[j], out=acc)
                for j in range(lo + 1, hi + 1):
                    np.add(acc, np.where(at >= j, vals[j], 0.0), out=acc)
            sc = acc[R]
        sc = np.where(np.isnan(sc), np.inf, sc)
        p = int(np.argmin(sc))  # the first of equal scores: R is ascending, and so is cols
        g = int(R[p])
        selected.append(int(cols[g]))
        scores.append(float(sc[p]))
        alive[g] = False
        at_g = where[:, g]  # where the removed client stands in every column (its own: nowhere)
        has = at_g < len(vals)
        vals[at_g[has], np.flatnonzero(has)] = 0.0  # a NaN distance to it becomes +0.0 too
        gone.append(at_g)
    return selected, scores


def _bulyan_positions(ids: np.ndarray) -> np.ndarray:
    """where[i][g]: the row at which client g stands in column i of ids
    ((m, w): m sorted positions of w clients); m for the client itself."""
    m, w = ids.shape
    where = np.full((w, w), m, dtype=np.intp)
    np.put_along_axis(where, np.ascontiguousarray(ids.T), np.arange(m)[None, :], axis=1)
    return where


def _bulyan_compact(vals: np.ndarray, ids: np.ndarray, cols: np.ndarray, alive: np.ndarray):
    """vals, ids and cols without the removed clients: their columns, and their
    (masked) entry in every other column; ids renumbered to the new columns."""
    R = np.flatnonzero(alive)
    n = len(R)
    sub = np.ascontiguousarray(ids[:, R].T)
    live = alive[sub]
    renumber = np.cumsum(alive) - 1
    new_ids = renumber[sub[live].reshape(n, n - 1)]
    new_vals = np.ascontiguousarray(vals[:, R].T)[live].reshape(n, n - 1)
    return np.ascontiguousarray(new_vals.T), np.ascontiguousarray(new_ids.T), cols[R]


class BulyanInfo:
    """What bulyan did: the clients `selected` by stage 1 in pick order with
    their `scores`, theta = K - 2f of them, `beta` = theta - 2f values kept
    per coordinate, and the pair-distance `method` asked for."""

    def __init__(self, selected, scores, theta: int, beta: int, method: str):
        self.selected = list(selected)
        self.scores = list(scores)
        self.theta = theta
        self.beta = beta
        self.method = method

    def __repr__(self):
        return (f"BulyanInfo(selected={self.selected}, theta={self.theta}, beta={self.beta}, "
                f"method={self.method!r})")


def bulyan(raw_client_grad_list: List[Tuple[float, "OrderedDict"]], byzantine_client_num: int, device=None,
           method: str = "auto", return_info: bool = False):
    """Bulyan (El Mhamdi, Guerraoui, Rouault; the "wise_bulyan" defense, ours:
    FedML's own "bulyan" is not reproduced) with f = byzantine_client_num of K
    clients, K >= 4f + 3.  Stage 1: theta = K - 2f clients by repeated Krum
    (bulyan_select) on the squared distances of the weight keys, one
    pairdist2_rows launch with `method` as Krum's.  Stage 2: per coordinate of
    EVERY key (BatchNorm statistics and counters too, as wise_trimmed_mean)
    the mean of the beta = theta - 2f selected values nearest the coordinate's
    median: one fedagg_nearmedian_mean_f32 launch over the whole row through a
    pointer table of the selected rows, fedagg_nearmedian_mean_wide_f32 from
    129 to 1024 selected clients (in the tiers of NEARMEDIAN_WIDE_AUTO) and
    nearmedian_mean_rows_torch for the rest.

    fp32 models (integer buffers allowed, entering as fl32(v)).  Sample counts
    are ignored, as by the median.  Returns a new OrderedDict in client 0's
    key order on the inputs' device (integer keys come back fp32); no client
    dict is modified.  return_info: also the BulyanInfo."""
    f = byzantine_client_num
    K = len(raw_client_grad_list)
    if f < 0:
        raise ValueError("bulyan: byzantine_client_num must be >= 0")
    if K < 4 * f + 3:
        raise ValueError(f"bulyan: byzantine_client_num = {f} needs at least 4f + 3 = {4 * f + 3} clients (got {K})")
    if method not in ("auto", "gram", "gram_wide", "exact"):
        raise ValueError(f"pair distance method {method!r}: 'auto', 'gram', 'gram_wide' or 'exact'")
    theta, beta = K - 2 * f, K - 4 * f
    dicts, keys = _client_dicts(raw_client_grad_list)
    if not keys:
        info = BulyanInfo(*bulyan_select(np.zeros((K, K)), f), theta, beta, method)
        return (OrderedDict(), info) if return_info else OrderedDict()
    _one_device(dicts[0], keys, "wise_bulyan")
    on_dev = dicts[0][keys[0]].is_cuda
    bucket, dev = _float_bucket(dicts[0], K, "wise_bulyan", device)
    with torch.cuda.device(dev):
        for i, d in enumerate(dicts):
            _put_float(bucket, i, d, keys)
        bucket.sync_ingest()
        g = bucket.groups[torch.float32]
        if f == 0:
            selected, scores = bulyan_select(np.empty((K, 0)), 0)  # no distances needed
        else:
            chunks, n_chunks = weight_chunks(g, nat.PAIR_CHUNK, dev)
            D = pairdist2_rows(g.d_ptrs, K, chunks, n_chunks, dev, method, length=g.length,
                               aligned=True).cpu().numpy()
            selected, scores = bulyan_select(D, f)
        if theta <= NEARMEDIAN_MAX_CLIENTS or nearmedian_wide_auto(theta):
            ptrs = g.d_ptrs if selected == list(range(K)) else \
                kn.upload_i64([g.rows[i].data_ptr() for i in selected], dev)
            row = torch.zeros(g.padded, dtype=torch.float32, device=dev)
            if theta <= NEARMEDIAN_MAX_CLIENTS:
                nearmedian_mean_rows(ptrs, theta, g.length, beta, row)
            else:
                nearmedian_mean_rows_wide(ptrs, theta, g.length, beta, row)
        else:
            row = nearmedian_mean_rows_torch([g.rows[i][:g.length] for i in selected], beta)
        out = _rows_to_dict([(g, row)], keys, on_dev, clone=True)
    return (out, BulyanInfo(selected, scores, theta, beta, method)) if return_info else out
