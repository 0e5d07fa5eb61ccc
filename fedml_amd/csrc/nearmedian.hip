// nearmedian.hip — gfx950 kernel of stage 2 of the "wise_bulyan" defense: per
// coordinate the mean of the `keep` client values nearest the coordinate's
// median, exported through include/fedagg.h (fedagg_nearmedian_mean_f32,
// where the operation is specified) and linked into libfedagg.so.  Its own
// translation unit: trimmed.hip is untouched, and the two sets of unpruned
// networks compile side by side.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "sortnet.h"

namespace {

// +inf: what a padded slot's load returns
__device__ float g_nearmedian_pad = __builtin_huge_valf();

// ---------------------------------------------------------------------------
// trimmed_mean_kernel's form for fp32 rows (trimmed.hip: one lane per column,
// the column in KMAX registers, SGPR-base + 32-bit-offset loads, the slot
// pointers of a padded tier staged in LDS, every NaN counted and replaced by
// +inf on arrival, +inf padding above rank K - 1, the unpruned pairwise
// network), then the window instead of the centred ranks.  With s[] the
// sorted registers, r = (K - 1) / 2, m = s[r] and d(v) = 0 if v == m else
// |v - m| (the replaced NaNs are the specification's "+inf above the real
// +inf"), the kept ranks are [lo, lo + keep) with
//     lo_min = max(0, r - keep + 1),  lo_max = min(r, K - keep),
//     lo = lo_min + #{ j in [lo_min, lo_max) : d(s[j]) > d(s[j + keep]) }:
// the window starting at j gives way to the one starting at j + 1 exactly
// when its lowest value is strictly farther from m than the value it would
// gain, d(s[j]) falls and d(s[j + keep]) rises with j, so the count is where
// the two-pointer rule of the header stops (a tie keeps the left value).
// No register array is indexed by a runtime value:
//   - m is a chain of selects under the wave-uniform r == j (padded tiers
//     only, over the ranks the tier's K can give; a full tier's r is static);
//   - the partners s[j + keep] come from a barrel shifter: a copy of the
//     sorted registers moved down by each set bit of the wave-uniform keep,
//     one stage of selects per bit, highest bit first.  A slot whose source
//     would lie above KMAX - 1 keeps its value: it is only ever read for a j
//     outside [lo_min, lo_max), which the wave-uniform range predicate
//     discards;
//   - the sum is trimmed.hip's uniform chain from -0 with the per-lane
//     predicate uint32(j - lo) < keep.
// Padding slots lie above rank K - 1: j + keep <= K - 1 for every counted j,
// the window ends at or below K, and r, lo_max and the NaN rule use the real K.

// The barrel shifter and the count, spelled as templates over the slot
// numbers (as the sorting network is): loops whose bounds depend on an outer
// loop's variable were unrolled too late for the copies to leave scratch.

// a[J] = a[J + SH] where keep has bit SH; a slot with no source keeps its value
template <int KMAX, int J, int SH>
__device__ __forceinline__ void shift_slot(float (&a)[KMAX], bool bit) {
  if constexpr (J + SH < KMAX) a[J] = bit ? a[J + SH] : a[J];
}
template <int KMAX, int SH, int... J>
__device__ __forceinline__ void shift_stage(float (&a)[KMAX], int keep, std::integer_sequence<int, J...>) {
  const bool bit = (keep & SH) != 0;
  (shift_slot<KMAX, J, SH>(a, bit), ...);  // ascending: a[J + SH] is still the stage's input
}
// stages SH, SH / 2, .. 1 for the partners of j in [0, NB): before the stage
// of SH the lower bits can still move a value down by SH - 1 slots
template <int KMAX, int NB, int SH>
__device__ __forceinline__ void shift_stages(float (&a)[KMAX], int keep) {
  if constexpr (SH < KMAX)  // keep == KMAX has no counted j
    shift_stage<KMAX, SH>(a, keep, std::make_integer_sequence<int, NB + SH - 1>{});
  if constexpr (SH > 1) shift_stages<KMAX, NB, SH / 2>(a, keep);
}

// d(x) is near_dist (sortnet.h, shared with nearmedian_wide.hip)

template <int KMAX, int J>
__device__ __forceinline__ void count_slot(const float (&v)[KMAX], const float (&a)[KMAX], float m, int lo_min,
                                           uint32_t span, int& lo) {
  // the range predicates are made 8 at a time: hoisted to the front, their
  // lane masks spill out of the SGPRs
  if constexpr (J % 8 == 0) __builtin_amdgcn_sched_barrier(0);
  const bool counted = uint32_t(J - lo_min) < span;  // wave-uniform
  lo += counted && near_dist(v[J], m) > near_dist(a[J], m) ? 1 : 0;
}
// lo += #{ j in [lo_min, lo_min + span) : d(s[j]) > d(s[j + keep]) }, j below NB
template <int KMAX, int... J>
__device__ __forceinline__ void count_window_start(const float (&v)[KMAX], float m, int keep, int lo_min,
                                                   uint32_t span, int& lo, std::integer_sequence<int, J...>) {
  float a[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) a[c] = v[c];
  shift_stages<KMAX, int(sizeof...(J)), 128>(a, keep);  // a[j] = s[j + keep] for j in [0, NB)
  (count_slot<KMAX, J>(v, a, m, lo_min, span, lo), ...);
  __builtin_amdgcn_sched_barrier(0);
}

template <int KMAX, int KMIN, bool FULL, int BS, bool OFF = false>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void nearmedian_mean_kernel(
    const float* const* __restrict__ src, int K, int64_t N, int keep, float* __restrict__ out, int64_t col0 = 0) {
  const int64_t e = int64_t(blockIdx.x) * BS + threadIdx.x;
  if constexpr (FULL) K = KMAX;  // K == KMAX: no padding, no per-client conditions
  __shared__ const float* tab[FULL ? 1 : KMAX];
  if constexpr (!FULL) {
    for (int i = threadIdx.x; i < KMAX; i += BS) tab[i] = i < K ? src[i] : &g_nearmedian_pad;
    __syncthreads();
  }
  if (e >= N) return;
  // the host guarantees N * sizeof(float) < 2^32 per launch
  const uint32_t boff = uint32_t(e) * uint32_t(sizeof(float));
  float v[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) {
    // the load form and the barrier: load_slot (sortnet.h)
    if (c % 16 == 0 && c) __builtin_amdgcn_sched_barrier(0);
    v[c] = load_slot<FULL, OFF>(src, tab, c, K, boff, col0);
  }
  // after every load is in flight: one unordered compare, a count and a
  // select per value
  __builtin_amdgcn_sched_barrier(0);
  int nans = 0;
#pragma unroll
  for (int c = 0; c < KMAX; ++c) {
    const bool n = __builtin_isnan(v[c]);
    nans += n ? 1 : 0;
    v[c] = n ? __builtin_huge_valf() : v[c];
  }
  // the count is complete here: left to sink to its use after the window, it
  // kept the 128 compares' lane masks alive across the sort (176 SGPR spills)
  asm volatile("" : "+v"(nans));
  __builtin_amdgcn_sched_barrier(0);
  pairwise_sort<KMAX>(v);  // every output slot is live: nothing is pruned
  __builtin_amdgcn_sched_barrier(0);

  // m = s[r]: r is static in a full tier, else one of the ranks K in
  // [KMIN, KMAX] can give
  constexpr int RMAX = (KMAX - 1) / 2, RMIN = FULL ? RMAX : (KMIN - 1) / 2;
  const int r = (K - 1) / 2;
  float m = v[RMAX];
#pragma unroll
  for (int j = RMIN; j < RMAX; ++j) m = r == j ? v[j] : m;
  const int lo_min = r - keep + 1 > 0 ? r - keep + 1 : 0;
  const int lo_max = r < K - keep ? r : K - keep;
  const uint32_t span = uint32_t(lo_max - lo_min);  // lo_max >= lo_min: both hold r's window
  int lo = lo_min;
  // counted j lie below lo_max <= r <= RMAX
  count_window_start<KMAX>(v, m, keep, lo_min, span, lo, std::make_integer_sequence<int, RMAX>{});

  // acc = s[lo], then acc = fl32(acc + s[j]) for j = lo+1 .. lo+keep-1, as
  // one uniform chain from -0 (see trimmed_mean_kernel): a slot outside the
  // window adds -0, which moves no sum
  const uint32_t ukeep = uint32_t(keep);
  float acc = -0.f;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    // 16 slots at a time: the compares' lane masks live in SGPR pairs
    if (j % 16 == 0) __builtin_amdgcn_sched_barrier(0);
    acc = acc + (uint32_t(j - lo) < ukeep ? v[j] : -0.f);
  }
  const float mean = acc / float(keep);  // IEEE division (the build's correctly rounded divide)
  // the window reaches a (replaced) NaN: ranks K - nans and above
  out[e] = lo + keep > K - nans ? __builtin_nanf("") : mean;
}

template <int KMAX, int KMIN>
int launch_nearmedian(const float* const* src, int K, int64_t N, int keep, float* out, hipStream_t st) {
  constexpr int BS = 64;  // the median kernel's block (median.hip launch_median)
  return launch_col_chunks("fedagg_nearmedian_mean_f32", nearmedian_mean_kernel<KMAX, KMIN, true, BS>,
                           nearmedian_mean_kernel<KMAX, KMIN, false, BS>,
                           nearmedian_mean_kernel<KMAX, KMIN, false, BS, true>, K == KMAX, BS, 1, st, src, K, N, out,
                           keep);
}

}  // namespace

extern "C" {

int fedagg_nearmedian_mean_f32(const float* const* d_src, int32_t K, int64_t N, int32_t keep, float* d_out,
                               uint32_t flags, fedagg_stream_t stream) {
  (void)flags;  // one kernel form for every alignment
  if (K < 1 || N < 0) return set_error(FEDAGG_EINVAL, "fedagg_nearmedian_mean_f32: K must be >= 1 and N >= 0");
  if (keep < 1 || keep > K)
    return set_error(FEDAGG_EINVAL, "fedagg_nearmedian_mean_f32: keep must be >= 1 and <= K");
  if (!d_src || !d_out) return set_error(FEDAGG_EINVAL, "fedagg_nearmedian_mean_f32: null pointer");
  if (K > FEDAGG_NEARMEDIAN_MAX_CLIENTS)
    return set_error(FEDAGG_ENOKERNEL, "fedagg_nearmedian_mean_f32: the kernel holds at most " +
                                           std::to_string(FEDAGG_NEARMEDIAN_MAX_CLIENTS) + " rows (K = " +
                                           std::to_string(K) + ")");
  if (N == 0) return FEDAGG_OK;
  auto st = reinterpret_cast<hipStream_t>(stream);
  // KMIN, the smallest K a tier is launched for, bounds the ranks the median can take
  return with_tier(K, [&](auto kmax, auto kmin) {
    return launch_nearmedian<decltype(kmax)::value, decltype(kmin)::value>(d_src, K, N, keep, d_out, st);
  });
}

}  // extern "C"
