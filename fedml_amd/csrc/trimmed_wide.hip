// trimmed_wide.hip — gfx950 kernel of the coordinate-wise trimmed mean for
// 129 to 1024 clients, exported through include/fedagg.h
// (fedagg_trimmed_mean_wide; the operation is specified at fedagg_trimmed_mean)
// and linked into libfedagg.so.  Its own translation unit: the lane-group
// sorts compile beside median.hip's and trimmed.hip's kernels, not after them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "lanesort.h"
#include "sortnet.h"

namespace {

// ---------------------------------------------------------------------------
// The fp32 median's form above 128 clients (median.hip, median_lanes_kernel):
// P adjacent lanes share one column, lane `sub` holding slots sub·R + j of
// its KMAX = P·R in registers, the slot pointers staged in LDS with a skew
// per lane group, a padded slot pointing at a constant with its column offset
// masked to 0.  The differences are trimmed_mean_kernel's (trimmed.hip):
//   - every rank is needed, so the whole sort runs (lanes_sort_all, lanesort.h):
//     afterwards slot sub·R + j holds rank sub·R + j;
//   - padding is +inf only, all of it above rank K - 1;
//   - no NaN enters the networks: each is counted and replaced by +inf as it
//     arrives, the counts added over the P lanes of the column.
// The specification's chain acc = s[trim], acc = fl32(acc + s[r]) in ascending
// r crosses the lanes, so it runs in P phases: in phase p every lane starts
// from the sum that lane p - 1 ended with (phase 0: -0.f) and adds its R
// registers in order, and lane p's result is handed on.  A register outside
// the kept ranks was replaced by -0.f beforehand (y + (-0) = y for every y),
// by the predicate uint32_t(sub·R + j - trim) < K - 2·trim.  A phase whose
// slots [p·R, (p+1)·R) hold no kept rank is skipped (K and trim are uniform).

// +inf in each element type: what a padded slot's load returns
template <class E>
__device__ typename E::S g_trimmed_wide_pad = trim_pos_inf<E>();

template <int P, int R, bool FULL, class E, int BS = 256>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void trimmed_mean_lanes_kernel(
    const typename E::S* const* __restrict__ src, int K, int64_t N, int trim, typename E::S* __restrict__ out) {
  using S = typename E::S;
  static_assert(P == 2 || P == 4 || P == 8 || P == 16, "2 to 16 lanes per column");
  static_assert(R == 64 || R == 128, "64 or 128 values per lane");
  static_assert(BS % 64 == 0 && 64 % P == 0, "whole waves of whole lane groups");
  constexpr int KMAX = P * R, PAD = kLanesSkew;
  // row pointer of every slot, skewed by PAD entries per lane group
  // (median_lanes_kernel); a padded slot reads the +inf constant at offset 0
  __shared__ const S* rows[KMAX + PAD * P];
  __shared__ uint64_t offmask[FULL ? 1 : KMAX + PAD * P];
  const int t = threadIdx.x, sub = t & (P - 1);
  if constexpr (FULL) K = KMAX;
  for (int i = t; i < KMAX; i += BS) {
    const int q = i + PAD * (i / R);
    if (FULL || i < K) {
      rows[q] = src[i];
      if constexpr (!FULL) offmask[q] = ~uint64_t(0);
    } else {
      rows[q] = &g_trimmed_wide_pad<E>;
      offmask[q] = 0;
    }
  }
  __syncthreads();
  // every lane stays active through the DPP exchanges; a column past the end
  // recomputes the last one and does not store
  const int64_t e = (int64_t(blockIdx.x) * BS + t) / P;
  const uint64_t boff = uint64_t(e < N ? e : N - 1) * sizeof(S);
  float v[R];
  int nans = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (j % 16 == 0 && j) __builtin_amdgcn_sched_barrier(0);
    S x = lanes_load(lanes_slot_ptr<R, FULL, S>(rows, offmask, sub, j, boff));
    if constexpr (sizeof(S) == 2) {
      // 16-bit rows test the raw value as it widens (trimmed_mean_kernel)
      const bool n = E::raw_nan(x);
      nans += n ? 1 : 0;
      x = n ? trim_pos_inf<E>() : x;
    }
    v[j] = E::widen(x);
  }
  if constexpr (sizeof(S) == 4) {
    // fp32 tests after every load is in flight
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const bool n = __builtin_isnan(v[j]);
      nans += n ? 1 : 0;
      v[j] = n ? __builtin_huge_valf() : v[j];
    }
  }
  nans = lanes_count_sum<P>(nans);
  lanes_sort_all<P>(v, sub);
  // the kept ranks as what the chain adds, everything else as -0.f
  const uint32_t kept = uint32_t(K - 2 * trim);
  const int first = sub * R - trim;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    float x = TrimVal<E>::value(v[j]);
    // opaque, so the value is made in every lane and then selected: left
    // visible, the f16 conversion went under a per-lane branch per register
    // (130 exec-mask branches at R = 128, and 28 B/lane of scratch)
    if constexpr (std::is_same_v<E, MedF16>) asm volatile("" : "+v"(x));
    v[j] = uint32_t(first + j) < kept ? x : -0.f;
  }
  float carry = -0.f;
  const int lane0 = int(__lane_id()) & ~(P - 1);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (p * R < K - trim && (p + 1) * R > trim) {  // uniform: the phase holds a kept rank
      float acc = carry;
#pragma unroll
      for (int j = 0; j < R; ++j) acc = acc + v[j];
      carry = __shfl(acc, lane0 + p, 64);  // lane p's sum; the other lanes' are dropped
    }
  }
  const float mean = carry / float(kept);  // IEEE division (the build's correctly rounded divide)
  if (sub == 0 && e < N) out[e] = TrimVal<E>::round(nans > trim ? __builtin_nanf("") : mean);
}

template <int P, int R, class E, int BS = 256>
int launch_trimmed_lanes(const typename E::S* const* src, int K, int64_t N, int trim, typename E::S* out,
                         hipStream_t st) {
  return launch_lanes("fedagg_trimmed_mean_wide", trimmed_mean_lanes_kernel<P, R, true, E, BS>,
                      trimmed_mean_lanes_kernel<P, R, false, E, BS>, K == P * R, P, BS, st, src, K, N, out, trim);
}

template <class E>
int trimmed_wide_dispatch(const typename E::S* const* d_src, int32_t K, int64_t N, int32_t trim,
                          typename E::S* d_out, hipStream_t st) {
  return with_lane_tier(K, [&](auto p, auto r) {
    return launch_trimmed_lanes<decltype(p)::value, decltype(r)::value, E>(d_src, K, N, trim, d_out, st);
  });
}

}  // namespace

extern "C" {

int fedagg_trimmed_mean_wide(int32_t dtype, const void* const* d_src, int32_t K, int64_t N, int32_t trim, void* d_out,
                             uint32_t flags, fedagg_stream_t stream) {
  (void)flags;  // one kernel form for every alignment
  if (K < 1 || N < 0) return set_error(FEDAGG_EINVAL, "fedagg_trimmed_mean_wide: K must be >= 1 and N >= 0");
  if (trim < 0 || 2 * int64_t(trim) >= int64_t(K))
    return set_error(FEDAGG_EINVAL,
                     "fedagg_trimmed_mean_wide: trim must be >= 0 and leave K - 2 * trim >= 1 values");
  if (!d_src || !d_out) return set_error(FEDAGG_EINVAL, "fedagg_trimmed_mean_wide: null pointer");
  if (dtype != FEDAGG_DT_F32 && dtype != FEDAGG_DT_BF16 && dtype != FEDAGG_DT_F16)
    return set_error(FEDAGG_EINVAL, "fedagg_trimmed_mean_wide: dtype must be FEDAGG_DT_F32, _BF16 or _F16");
  if (K > FEDAGG_TRIMMED_WIDE_MAX_CLIENTS)
    return set_error(FEDAGG_ENOKERNEL, "fedagg_trimmed_mean_wide: the kernel holds at most " +
                                           std::to_string(FEDAGG_TRIMMED_WIDE_MAX_CLIENTS) + " clients (K = " +
                                           std::to_string(K) + ")");
  if (N == 0) return FEDAGG_OK;  // launch_lanes bounds the grid ("N too large")
  auto st = reinterpret_cast<hipStream_t>(stream);
  switch (dtype) {
    case FEDAGG_DT_F32:
      return trimmed_wide_dispatch<MedF32>(reinterpret_cast<const float* const*>(d_src), K, N, trim,
                                           static_cast<float*>(d_out), st);
    case FEDAGG_DT_BF16:
      return trimmed_wide_dispatch<MedBF16>(reinterpret_cast<const uint16_t* const*>(d_src), K, N, trim,
                                            static_cast<uint16_t*>(d_out), st);
    default:
      return trimmed_wide_dispatch<MedF16>(reinterpret_cast<const uint16_t* const*>(d_src), K, N, trim,
                                           static_cast<uint16_t*>(d_out), st);
  }
}

}  // extern "C"
