// nearmedian_wide.hip — gfx950 kernel of stage 2 of the "wise_bulyan" defense
// for 129 to 1024 selected clients, exported through include/fedagg.h
// (fedagg_nearmedian_mean_wide_f32; the operation is specified at
// fedagg_nearmedian_mean_f32) and linked into libfedagg.so.  Its own
// translation unit: the lane-group sorts compile beside trimmed_wide.hip's.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "lanesort.h"
#include "sortnet.h"

namespace {

// +inf: what a padded slot's load returns
__device__ float g_nearmedian_wide_pad = __builtin_huge_valf();

// ---------------------------------------------------------------------------
// trimmed_mean_lanes_kernel's form for fp32 rows (trimmed_wide.hip: P adjacent
// lanes share a column, lane `sub` holding slots sub·R + j in registers, the
// slot pointers staged in LDS with a skew, a padded slot reading +inf, every
// NaN counted and replaced by +inf on arrival, then the whole sort
// (lanes_sort_all), so that slot sub·R + j holds rank sub·R + j), then
// nearmedian_mean_kernel's window (nearmedian.hip) instead of the centred
// ranks.  With s[] the sorted slots, r = (K - 1) / 2, m = s[r], d = near_dist:
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
//         padded to 1 mod 32 words, so they fall on 16 different banks.
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

template <int P, int R, bool FULL, int BS = 256>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(2))) void nearmedian_mean_lanes_kernel(
    const float* const* __restrict__ src, int K, int64_t N, int keep, float* __restrict__ out) {
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
  const float** rows = reinterpret_cast<const float**>(smem);
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
      rows[q] = &g_nearmedian_wide_pad;
      offmask[q] = 0;
    }
  }
  __syncthreads();
  // every lane stays active through the DPP exchanges and the block barrier;
  // a column past the end recomputes the last one and does not store
  const int64_t e = (int64_t(blockIdx.x) * BS + t) / P;
  const uint64_t boff = uint64_t(e < N ? e : N - 1) * sizeof(float);
  float v[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (j % 16 == 0 && j) __builtin_amdgcn_sched_barrier(0);
    v[j] = lanes_load(lanes_slot_ptr<R, FULL, float>(rows, offmask, sub, j, boff));
  }
  // after every load is in flight
  __builtin_amdgcn_sched_barrier(0);
  int nans = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const bool n = __builtin_isnan(v[j]);
    nans += n ? 1 : 0;
    v[j] = n ? __builtin_huge_valf() : v[j];
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
  if (sub == 0 && e < N) out[e] = lo + keep > K - nans ? __builtin_nanf("") : mean;
}

template <int P, int R, int BS = 256>
int launch_nearmedian_lanes(const float* const* src, int K, int64_t N, int keep, float* out, hipStream_t st) {
  return launch_lanes("fedagg_nearmedian_mean_wide_f32", nearmedian_mean_lanes_kernel<P, R, true, BS>,
                      nearmedian_mean_lanes_kernel<P, R, false, BS>, K == P * R, P, BS, st, src, K, N, out, keep);
}

}  // namespace

extern "C" {

int fedagg_nearmedian_mean_wide_f32(const float* const* d_src, int32_t K, int64_t N, int32_t keep, float* d_out,
                                    uint32_t flags, fedagg_stream_t stream) {
  (void)flags;  // one kernel form for every alignment
  if (K < 1 || N < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_nearmedian_mean_wide_f32: K must be >= 1 and N >= 0");
  if (keep < 1 || keep > K)
    return set_error(FEDAGG_EINVAL, "fedagg_nearmedian_mean_wide_f32: keep must be >= 1 and <= K");
  if (!d_src || !d_out) return set_error(FEDAGG_EINVAL, "fedagg_nearmedian_mean_wide_f32: null pointer");
  if (K > FEDAGG_NEARMEDIAN_WIDE_MAX_CLIENTS)
    return set_error(FEDAGG_ENOKERNEL, "fedagg_nearmedian_mean_wide_f32: the kernel holds at most " +
                                           std::to_string(FEDAGG_NEARMEDIAN_WIDE_MAX_CLIENTS) + " rows (K = " +
                                           std::to_string(K) + ")");
  if (N == 0) return FEDAGG_OK;  // launch_lanes bounds the grid ("N too large")
  auto st = reinterpret_cast<hipStream_t>(stream);
  return with_lane_tier(K, [&](auto p, auto r) {
    return launch_nearmedian_lanes<decltype(p)::value, decltype(r)::value>(d_src, K, N, keep, d_out, st);
  });
}

}  // extern "C"
