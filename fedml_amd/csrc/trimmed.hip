// trimmed.hip — gfx950 kernel of the coordinate-wise trimmed mean (Yin et
// al.: every coordinate drops its `trim` smallest and `trim` largest client
// values and averages the rest), exported through include/fedagg.h
// (fedagg_trimmed_mean, where the operation is specified) and linked into
// libfedagg.so.  Its own translation unit: the unpruned networks compile
// beside median.hip's pruned ones, not after them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "sortnet.h"

namespace {

// ---------------------------------------------------------------------------
// The median kernel's form (median.hip: one lane per column, the column's K
// values in KMAX registers, loads in the SGPR-base + 32-bit-offset form, the
// slot pointers of a padded tier staged in LDS), with three differences:
//   - every rank is needed, so the pairwise network runs unpruned (1,471
//     comparators at 128 slots against ~1,040 kept by the median);
//   - padding is +inf only, all of it above rank K - 1, so ranks below K are
//     those of the column itself;
//   - fminf / fmaxf drop a NaN and duplicate its partner, so no NaN enters
//     the network: each is counted and replaced by +inf as it arrives.  The
//     replacements sit with the real +inf at the top; with count <= trim the
//     kept ranks trim .. K-trim-1 hold exactly the specification's multiset
//     (NaN ranks above +inf there too), with count > trim the result is NaN.
// The sum is the specification's sequential fp32 chain over the sorted
// registers, fully unrolled; which slots count is decided by the
// wave-uniform predicate trim <= r < K - trim, so no register array is
// indexed by a runtime value.

// TrimVal (what the chain adds for a sorted selection value, and the final
// rounding) and trim_pos_inf: sortnet.h, shared with trimmed_wide.hip

// +inf in each element type: what a padded slot's load returns
template <class E>
__device__ typename E::S g_trimmed_pad = trim_pos_inf<E>();

// Columns [col0, col0 + N) of the rows; out points at column col0's slot.
// Launches cover at most 2^30 columns (kColsChunk) so that a lane's byte
// offset from the (wave-uniform) row base + col0 fits in 32 bits.
template <int KMAX, bool FULL, int BS, class E, bool OFF = false>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void trimmed_mean_kernel(const typename E::S* const* __restrict__ src, int K,
                                                          int64_t N, int trim, typename E::S* __restrict__ out,
                                                          int64_t col0 = 0) {
  using S = typename E::S;
  const int64_t e = int64_t(blockIdx.x) * BS + threadIdx.x;
  if constexpr (FULL) K = KMAX;  // K == KMAX: no padding, no per-client conditions
  // K < KMAX: the KMAX slot pointers (pads point at a +inf constant) staged
  // in LDS once per block, as in median_kernel
  __shared__ const S* tab[FULL ? 1 : KMAX];
  if constexpr (!FULL) {
    for (int i = threadIdx.x; i < KMAX; i += BS) tab[i] = i < K ? src[i] : &g_trimmed_pad<E>;
    __syncthreads();
  }
  if (e >= N) return;
  // the host guarantees N * sizeof(S) < 2^32 per launch
  const uint32_t boff = uint32_t(e) * uint32_t(sizeof(S));
  float v[KMAX];
  int nans = 0;
#pragma unroll
  for (int c = 0; c < KMAX; ++c) {
    // the load form and the barrier: load_slot (sortnet.h)
    if (c % 16 == 0 && c) __builtin_amdgcn_sched_barrier(0);
    S x = load_slot<FULL, OFF>(src, tab, c, K, boff, col0);
    if constexpr (sizeof(S) == 2) {
      // 16-bit rows test the raw value as it widens (holding every raw value
      // until all loads have landed would double the live registers)
      const bool n = E::raw_nan(x);
      nans += n ? 1 : 0;
      x = n ? trim_pos_inf<E>() : x;
    }
    v[c] = E::widen(x);
  }
  if constexpr (sizeof(S) == 4) {
    // fp32 tests after every load is in flight: one unordered compare, a
    // count and a select per value
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < KMAX; ++c) {
      const bool n = __builtin_isnan(v[c]);
      nans += n ? 1 : 0;
      v[c] = n ? __builtin_huge_valf() : v[c];
    }
  }
  pairwise_sort<KMAX>(v);  // every output slot is live: nothing is pruned
  // acc = s[trim], then acc = fl32(acc + s[r]) for r = trim+1 .. K-trim-1,
  // as one uniform chain from -0: a slot outside the kept ranks adds -0,
  // and y + (-0) = y for every y (-0 and NaN included), so the first kept
  // value enters as itself and nothing else moves the sum.  One
  // wave-uniform predicate per slot, trim <= r < K - trim as a single
  // unsigned compare.  The predicates are made after the sort, 16 slots at a
  // time: computed up front, their 128 lane masks spilled out of the SGPRs.
  const uint32_t kept = uint32_t(K - 2 * trim);
  float acc = -0.f;
#pragma unroll
  for (int r = 0; r < KMAX; ++r) {
    if (r % 16 == 0) __builtin_amdgcn_sched_barrier(0);
    const float x = TrimVal<E>::value(v[r]);
    acc = acc + (uint32_t(r - trim) < kept ? x : -0.f);
  }
  const float mean = acc / float(kept);  // IEEE division (the build's correctly rounded divide)
  out[e] = TrimVal<E>::round(nans > trim ? __builtin_nanf("") : mean);
}

template <int KMAX, class E>
int launch_trimmed(const typename E::S* const* src, int K, int64_t N, int trim, typename E::S* out, hipStream_t st) {
  constexpr int BS = 64;  // the median kernel's block (median.hip launch_median)
  return launch_col_chunks("fedagg_trimmed_mean", trimmed_mean_kernel<KMAX, true, BS, E>,
                           trimmed_mean_kernel<KMAX, false, BS, E>, trimmed_mean_kernel<KMAX, false, BS, E, true>,
                           K == KMAX, BS, 1, st, src, K, N, out, trim);
}

template <class E>
int trimmed_dispatch(const typename E::S* const* d_src, int32_t K, int64_t N, int32_t trim, typename E::S* d_out,
                     hipStream_t st) {
  return with_tier(
      K, [&](auto kmax, auto) { return launch_trimmed<decltype(kmax)::value, E>(d_src, K, N, trim, d_out, st); });
}

}  // namespace

extern "C" {

int fedagg_trimmed_mean(int32_t dtype, const void* const* d_src, int32_t K, int64_t N, int32_t trim, void* d_out,
                        uint32_t flags, fedagg_stream_t stream) {
  (void)flags;  // one kernel form for every alignment
  if (K < 1 || N < 0) return set_error(FEDAGG_EINVAL, "fedagg_trimmed_mean: K must be >= 1 and N >= 0");
  if (trim < 0 || 2 * int64_t(trim) >= int64_t(K))
    return set_error(FEDAGG_EINVAL, "fedagg_trimmed_mean: trim must be >= 0 and leave K - 2 * trim >= 1 values");
  if (!d_src || !d_out) return set_error(FEDAGG_EINVAL, "fedagg_trimmed_mean: null pointer");
  if (dtype != FEDAGG_DT_F32 && dtype != FEDAGG_DT_BF16 && dtype != FEDAGG_DT_F16)
    return set_error(FEDAGG_EINVAL, "fedagg_trimmed_mean: dtype must be FEDAGG_DT_F32, _BF16 or _F16");
  if (K > FEDAGG_TRIMMED_MAX_CLIENTS)
    return set_error(FEDAGG_ENOKERNEL, "fedagg_trimmed_mean: the kernel holds at most " +
                                           std::to_string(FEDAGG_TRIMMED_MAX_CLIENTS) + " clients (K = " +
                                           std::to_string(K) + ")");
  if (N == 0) return FEDAGG_OK;
  auto st = reinterpret_cast<hipStream_t>(stream);
  switch (dtype) {
    case FEDAGG_DT_F32:
      return trimmed_dispatch<MedF32>(reinterpret_cast<const float* const*>(d_src), K, N, trim,
                                      static_cast<float*>(d_out), st);
    case FEDAGG_DT_BF16:
      return trimmed_dispatch<MedBF16>(reinterpret_cast<const uint16_t* const*>(d_src), K, N, trim,
                                       static_cast<uint16_t*>(d_out), st);
    default:
      return trimmed_dispatch<MedF16>(reinterpret_cast<const uint16_t* const*>(d_src), K, N, trim,
                                      static_cast<uint16_t*>(d_out), st);
  }
}

}  // extern "C"
