// nearmedian.h — the kernels of stage 2 of the "wise_bulyan" defense: per
// coordinate the mean of the `keep` client values nearest the coordinate's
// median (specified at fedagg_nearmedian_mean_f32, include/fedagg.h), as
// templates over the rows' element type E.  nearmedian.hip and
// nearmedian_wide.hip instantiate them for fp32 rows (E = MedF32),
// nearmedian16.hip and nearmedian_wide16.hip for bf16 and f16 rows (MedBF16,
// NearF16); everything is internal to the including translation unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "lanesort.h"
#include "sortnet.h"

namespace {

// The distance d(x) of a sorted value from the median m.  x - m is NaN only
// for equal infinities, which fmaxf turns into the 0 of x == m; every other
// x == m gives 0 by itself
__device__ __forceinline__ float near_dist(float x, float m) { return fmaxf(__builtin_fabsf(x - m), 0.f); }

// f16 rows here.  MedF16's selection value (sortnet.h) is an order key, which
// serves kernels that only compare; every counted rank of this one needs
// |v - m|, and the output is a mean, not one of the inputs.  So the value is
// widened to what it is, one v_cvt_f32_f16 as it arrives (exact, subnormals
// included), and never narrowed back: after the load an f16 column is an fp32
// column.  bf16 rows need nothing of their own: MedBF16::widen is the value.
struct NearF16 {
  using S = uint16_t;
  static __device__ __forceinline__ bool raw_nan(S x) { return MedF16::raw_nan(x); }
  static __device__ __forceinline__ float widen(S x) { return static_cast<float>(__builtin_bit_cast(_Float16, x)); }
  static constexpr uint32_t kPosInf = MedF16::kPosInf;
};
template <>
struct TrimVal<NearF16> {
  static __device__ __forceinline__ float value(float v) { return v; }
  static __device__ __forceinline__ uint16_t round(float f) { return TrimVal<MedF16>::round(f); }
};

// +inf in each element type: what a padded slot's load returns
template <class E>
__device__ typename E::S g_nearmedian_pad = trim_pos_inf<E>();

// ---------------------------------------------------------------------------
// trimmed_mean_kernel's form (trimmed.hip: one lane per column, the column in
// KMAX registers, SGPR-base + 32-bit-offset loads, the slot pointers of a
// padded tier staged in LDS, every NaN counted and replaced by +inf on
// arrival, +inf padding above rank K - 1, the unpruned pairwise network), then
// the window instead of the centred ranks.  16-bit rows are widened exactly as
// they arrive (their raw bits tested for NaN first) and are fp32 values from
// there on; the fp32 mean is rounded once to the rows' type at the store.
// With s[] the sorted registers, r = (K - 1) / 2, m = s[r] and d(v) = 0 if
// v == m else |v - m| (the replaced NaNs are the specification's "+inf above
// the real +inf"), the kept ranks are [lo, lo + keep) with
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

template <int KMAX, int KMIN, bool FULL, int BS, class E, bool OFF = false>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void nearmedian_mean_kernel(
    const typename E::S* const* __restrict__ src, int K, int64_t N, int keep, typename E::S* __restrict__ out,
    int64_t col0 = 0) {
  using S = typename E::S;
  const int64_t e = int64_t(blockIdx.x) * BS + threadIdx.x;
  if constexpr (FULL) K = KMAX;  // K == KMAX: no padding, no per-client conditions
  __shared__ const S* tab[FULL ? 1 : KMAX];
  if constexpr (!FULL) {
    for (int i = threadIdx.x; i < KMAX; i += BS) tab[i] = i < K ? src[i] : &g_nearmedian_pad<E>;
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
      // 16-bit rows test the raw value as it widens (trimmed_mean_kernel:
      // holding every raw value until all loads have landed would double the
      // live registers)
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
  out[e] = TrimVal<E>::round(lo + keep > K - nans ? __builtin_nanf("") : mean);
}

// ---------------------------------------------------------------------------
// trimmed_mean_lanes_kernel's form (trimmed_wide.hip: P adjacent lanes share
// a column, lane `sub` holding slots sub·R + j in registers, the slot pointers
// staged in LDS with a skew, a padded slot reading +inf, every NaN counted and
// replaced by +inf on arrival, then the whole sort (lanes_sort_all), so that
// slot sub·R + j holds rank sub·R + j), then nearmedian_mean_kernel's window
// instead of the centred ranks; 16-bit rows widen as they arrive, as there.
// With s[] the sorted slots, r = (K - 1) / 2, m = s[r], d = near_dist:
//     lo_min = max(0, r - keep + 1),  lo_max = min(r, K - keep),
//     lo = lo_min + #{ p in [lo_min, lo_max) : d(s[p]) > d(s[p + keep]) }.
//   - m: r is wave-uniform, so m is register r % R of lane r / R: a chain of
//     selects under the uniform r % R == j, then one broadcast inside the lane
//     group.  A full tier's r = KMAX / 2 - 1 is static: register R - 1 of lane
//     P / 2 - 1.
//   - the partners s[p + keep] of a column that lives in P lanes.  In
//     registers they would be a rotated copy of all R sorted values beside the
//     values themselves (2 R = 256 VGPRs at R = 128, the whole budget of two
//     waves per SIMD), so they go through LDS instead, where a shift by keep
//     is a write address: the lane holding rank g writes it to position
//     g - keep of the column's ring, the lane holding rank p reads position p.
//       * Every counted p has its partner in [r + 1, K), and K <= r + 1 + W
//         with W = KMAX / 2.  Exactly the W ranks g in [r + 1, r + 1 + W) are
//         written, to ring slot (g - keep) mod W: no two of them share a slot,
//         and a reader finds position p at slot p mod W, which for lane `sub`
//         is chunk sub % (P/2) of the ring at offset j: a lane-constant base
//         plus the register number, an immediate.  A slot that nothing wrote
//         (or that holds the position W below or above) is only ever read for
//         a p outside [lo_min, lo_max), which the range predicate discards.
//       * With q = keep / R and t = keep % R (wave-uniform), lane w's register
//         j lands in chunk (w - q) % (P/2) at offset j - t, or for j < t in
//         the chunk before it at offset j - t + R: two lane-constant bases
//         selected per register under the uniform j >= t.  Whether a register
//         is written is one of two lane masks in the same way: with
//         wq = (r + 1) / R and tr = (r + 1) % R, lane w writes j >= tr when
//         0 <= w - wq < P/2 and j < tr when 0 <= w - wq - 1 < P/2.  In a full
//         tier r + 1 = W: the upper half of the lanes write everything.
//       * Banks (32 for ds_read_b32 / ds_write_b32, conflicts per 32-lane
//         half): a half wave reads 32 / P columns x P/2 distinct chunks = 16
//         addresses at one j.  A chunk is R + 8 words and a column's ring is
//         padded to 1 mod 32 words, so they fall on 16 different banks.  The
//         ring holds fp32 words whatever the rows' type.
//       * The ring (W + padding words per column, 64 columns of 4 lanes or 32
//         of 8 per block: 41 to 74 KB) shares its LDS with the slot-pointer
//         table, which is dead once the loads have returned; a block barrier
//         stands between the two uses.  A ring is written and read by the P
//         lanes of one column only, which sit in one wave: its writes and reads
//         are ordered by a wave-level fence.
//       * R words in front of the first ring keep the lane-constant write
//         base (which has - t folded in) from going below the array.
//   - the per-lane counts are added over the P lanes (lanes_count_sum), so
//     every lane of the group has the same lo.
//   - the sum is trimmed_mean_lanes_kernel's P-phase chain from -0.f with the
//     per-column predicate uint32_t(sub·R + j - lo) < keep; a phase is skipped
//     when its slots lie wholly outside [lo_min, lo_max + keep), which is
//     uniform.
// No register array is indexed by a runtime value.  Padding slots lie above
// rank K - 1: p + keep <= K - 1 for every counted p, the window ends at or
// below K, and r, lo_max and the NaN rule use the real K.

template <int P, int R, bool FULL, class E, int BS = 256>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void nearmedian_mean_lanes_kernel(
    const typename E::S* const* __restrict__ src, int K, int64_t N, int keep, typename E::S* __restrict__ out) {
  using S = typename E::S;
  static_assert(P == 4 || P == 8, "4 or 8 lanes per column");
  static_assert(R == 64 || R == 128, "64 or 128 values per lane");
  static_assert(BS % 64 == 0 && 64 % P == 0, "whole waves of whole lane groups");
  constexpr int KMAX = P * R, PAD = kLanesSkew, NSLOT = KMAX + PAD * P;
  // the ring of partner positions: H chunks of R (+ 8) words per column
  constexpr int H = P / 2, W = H * R, CHUNK = R + 8;
  constexpr int COLW = H * CHUNK + (33 - (H * CHUNK) % 32) % 32;  // 1 mod 32 words per column
  constexpr int NCOL = BS / P, FRONT = R;
  static_assert(COLW % 32 == 1 && COLW >= H * CHUNK, "a column's ring, padded to 1 mod 32 words");
  constexpr size_t kTabBytes = size_t(NSLOT) * 8 * (FULL ? 1 : 2);
  constexpr size_t kRingBytes = size_t(FRONT + NCOL * COLW) * sizeof(float);
  __shared__ __attribute__((aligned(16))) char smem[kTabBytes > kRingBytes ? kTabBytes : kRingBytes];
  // row pointer of every slot, skewed by PAD entries per lane group
  // (median_lanes_kernel); a padded slot reads the +inf constant at offset 0
  const S** rows = reinterpret_cast<const S**>(smem);
  uint64_t* offmask = reinterpret_cast<uint64_t*>(smem + size_t(NSLOT) * 8);  // padded tiers only
  float* ring = reinterpret_cast<float*>(smem);
  const int t = threadIdx.x, sub = t & (P - 1);
  if constexpr (FULL) K = KMAX;
  for (int i = t; i < KMAX; i += BS) {
    const int q = i + PAD * (i / R);
    if (FULL || i < K) {
      rows[q] = src[i];
      if constexpr (!FULL) offmask[q] = ~uint64_t(0);
    } else {
      rows[q] = &g_nearmedian_pad<E>;
      offmask[q] = 0;
    }
  }
  __syncthreads();
  // every lane stays active through the DPP exchanges and the block barrier;
  // a column past the end recomputes the last one and does not store
  const int64_t e = (int64_t(blockIdx.x) * BS + t) / P;
  const uint64_t boff = uint64_t(e < N ? e : N - 1) * sizeof(S);
  float v[R];
  int nans = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (j % 16 == 0 && j) __builtin_amdgcn_sched_barrier(0);
    S x = lanes_load(lanes_slot_ptr<R, FULL, S>(rows, offmask, sub, j, boff));
    if constexpr (sizeof(S) == 2) {
      // 16-bit rows test the raw value as it widens (nearmedian_mean_kernel)
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
  __syncthreads();  // the pointer table is dead in every wave: its LDS becomes the ring

  // m = s[r]
  const int lane0 = int(__lane_id()) & ~(P - 1);
  const int r = FULL ? W - 1 : (K - 1) / 2;
  float m;
  if constexpr (FULL) {
    m = __shfl(v[R - 1], lane0 + H - 1, 64);
  } else {
    const int rj = r & (R - 1);
    m = v[0];
#pragma unroll
    for (int j = 1; j < R; ++j) m = rj == j ? v[j] : m;
    m = __shfl(m, lane0 + r / R, 64);
  }
  const int lo_min = r - keep + 1 > 0 ? r - keep + 1 : 0;
  const int lo_max = r < K - keep ? r : K - keep;
  const uint32_t span = uint32_t(lo_max - lo_min);  // lo_max >= lo_min: both hold r's window

  // ranks [r + 1, r + 1 + W) to ring slot (rank - keep) mod W
  const int cbase = FRONT + (t / P) * COLW;
  const int kq = keep / R, kt = keep & (R - 1);
  // as byte offsets: the select's result is the address register
  const int a1 = 4 * (cbase + ((sub - kq) & (H - 1)) * CHUNK - kt);  // j >= kt
  const int a0 = 4 * (cbase + ((sub - kq - 1) & (H - 1)) * CHUNK - kt + R);  // j < kt
  if constexpr (FULL) {
    if (sub >= H) {
#pragma unroll
      for (int j = 0; j < R; ++j) *reinterpret_cast<float*>(smem + ((j >= kt ? a1 : a0) + 4 * j)) = v[j];
    }
  } else {
    const int wq = (r + 1) / R, tr = (r + 1) & (R - 1);
    const bool hi = uint32_t(sub - wq) < uint32_t(H), lo_ok = uint32_t(sub - wq - 1) < uint32_t(H);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (j >= tr ? hi : lo_ok) *reinterpret_cast<float*>(smem + ((j >= kt ? a1 : a0) + 4 * j)) = v[j];
    }
  }
  // the readers are other lanes of the same wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // lo = lo_min + #{ p in [lo_min, lo_max) : d(s[p]) > d(s[p + keep]) }
  const float* rd = ring + cbase + (sub & (H - 1)) * CHUNK;
  const int rel = sub * R - lo_min;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    // 16 partners in flight at a time, and the count complete up to here:
    // left to the scheduler, every read and every 0 / 1 waits in a register
    // of its own for one sum at the end
    if (j % 16 == 0) {
      asm volatile("" : "+v"(cnt));
      __builtin_amdgcn_sched_barrier(0);
    }
    float a = rd[j];
    // opaque, so the read is made in every lane: left visible, it went under
    // a per-lane branch on `counted` per register
    asm volatile("" : "+v"(a));
    const bool counted = uint32_t(rel + j) < span;
    cnt += (counted & (near_dist(v[j], m) > near_dist(a, m))) ? 1 : 0;
  }
  __builtin_amdgcn_sched_barrier(0);
  const int lo = lo_min + lanes_count_sum<P>(cnt);

  // acc = s[lo], then acc = fl32(acc + s[j]) for j = lo+1 .. lo+keep-1: the
  // chain of trimmed_mean_lanes_kernel with the column's own window
  const uint32_t ukeep = uint32_t(keep);
  const int first = sub * R - lo;
#pragma unroll
  for (int j = 0; j < R; ++j) v[j] = uint32_t(first + j) < ukeep ? v[j] : -0.f;
  float carry = -0.f;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (p * R < lo_max + keep && (p + 1) * R > lo_min) {  // uniform: the phase can hold a kept rank
      float acc = carry;
#pragma unroll
      for (int j = 0; j < R; ++j) acc = acc + v[j];
      carry = __shfl(acc, lane0 + p, 64);  // lane p's sum; the other lanes' are dropped
    }
  }
  const float mean = carry / float(keep);  // IEEE division (the build's correctly rounded divide)
  // the window reaches a (replaced) NaN: ranks K - nans and above
  if (sub == 0 && e < N) out[e] = TrimVal<E>::round(lo + keep > K - nans ? __builtin_nanf("") : mean);
}

// ---------------------------------------------------------------------------
// Host side: `what` is the export's name in every message.

// the checks every export makes before any HIP call
inline int nearmedian_args(const std::string& what, const void* d_src, int32_t K, int64_t N, int32_t keep,
                           const void* d_out, int max_clients) {
  if (K < 1 || N < 0) return set_error(FEDAGG_EINVAL, what + ": K must be >= 1 and N >= 0");
  if (keep < 1 || keep > K) return set_error(FEDAGG_EINVAL, what + ": keep must be >= 1 and <= K");
  if (!d_src || !d_out) return set_error(FEDAGG_EINVAL, what + ": null pointer");
  if (K > max_clients)
    return set_error(FEDAGG_ENOKERNEL, what + ": the kernel holds at most " + std::to_string(max_clients) +
                                           " rows (K = " + std::to_string(K) + ")");
  return FEDAGG_OK;
}

// K <= 128: KMIN, the smallest K a tier is launched for, bounds the ranks the median can take
template <class E>
int nearmedian_dispatch(const char* what, const typename E::S* const* src, int K, int64_t N, int keep,
                        typename E::S* out, hipStream_t st) {
  constexpr int BS = 64;  // the median kernel's block (median.hip launch_median)
  return with_tier(K, [&](auto kmax, auto kmin) {
    constexpr int KMAX = decltype(kmax)::value, KMIN = decltype(kmin)::value;
    return launch_col_chunks(what, nearmedian_mean_kernel<KMAX, KMIN, true, BS, E>,
                             nearmedian_mean_kernel<KMAX, KMIN, false, BS, E>,
                             nearmedian_mean_kernel<KMAX, KMIN, false, BS, E, true>, K == KMAX, BS, 1, st, src, K, N,
                             out, keep);
  });
}

// K <= 1024
template <class E, int BS = 256>
int nearmedian_wide_dispatch(const char* what, const typename E::S* const* src, int K, int64_t N, int keep,
                             typename E::S* out, hipStream_t st) {
  return with_lane_tier(K, [&](auto p, auto r) {
    constexpr int P = decltype(p)::value, R = decltype(r)::value;
    return launch_lanes(what, nearmedian_mean_lanes_kernel<P, R, true, E, BS>,
                        nearmedian_mean_lanes_kernel<P, R, false, E, BS>, K == P * R, P, BS, st, src, K, N, out, keep);
  });
}

}  // namespace
