// geomed16.hip — the fused Weiszfeld step of the geometric-median defense for
// bf16 / f16 rows, exported through include/fedagg.h (fedagg_wsum_dist2_16,
// where the operation is specified) and linked into libfedagg.so beside
// geomed.hip, whose reduction, finish kernel and chunk-group rule it shares
// (weiszfeld.h).
//
// The rows stay 16-bit on the card and are widened exactly as they load; the
// iterate z and everything after the load are fp32 / fp64 as in geomed.hip.
// The layout is made for 16-bit rows, not the fp32 one with a narrower load:
//
//   Two columns per lane.  A lane's load is ONE DWORD holding two adjacent
//   columns, so a wave's row segment is still a coalesced 256-byte read and
//   covers 128 columns (a 2-byte load per lane would halve the bytes per
//   request); a block's four waves take the 128-column groups w, w + 4, ...
//   of a chunk.  The K packed dwords sit in KMAX registers (tiers 8 .. 128,
//   FULL for K == KMAX): twice the values in geomed.hip's register budget.
//
//   Widening in registers.  bf16: x << 16 and x & 0xffff0000; f16: the two
//   halves' converts.  A slot past K re-reads row 0, its packed dword is
//   masked to 0 once (both halves +0) and its weight is -0, which leaves both
//   chains as they were (geomed.hip's trick).
//
//   Two chains per lane, fedagg_wsum_f32's: fl32(x * w), then fl32(acc + .),
//   never an FMA, the weights broadcast from LDS, the pointer table re-read
//   per column group through the scalar cache.  z leaves as one 8-byte store
//   per lane where d_z + start is 8-byte aligned, as two dword stores
//   otherwise.
//
//   Distances.  The lane forms both fp32 differences, adds their two exact
//   fp64 squares ONCE and enters geomed.hip's transposing reduction with the
//   sum, so one fold serves two columns.  KMAX / 64 fp64 accumulators per
//   lane persist across the loop; per-block partials, then wd_finish_kernel.
//
//   Alignment.  A chunk takes the dword form when its start is even and every
//   row pointer is 4-byte aligned; the block finds the latter once, while the
//   weights are copied into LDS.  Whole 128-column groups then load dwords.
//   The chunk's last, partial group, and every group of a chunk that cannot
//   take dwords (the element form: one column per lane, 64-column groups),
//   load 2-byte elements into the same packed register, so nothing past a
//   chunk's last column is ever read; a half-lane past the end holds +0, is
//   masked out of the distances and stores nothing.  After the load the two
//   forms are the same instructions: z is the same bits in either.
//
// This unit is compiled without packed fp32 VALU instructions (build.py,
// UNIT_FLAGS, which gives the reason): the chains are v_mul_f32 / v_add_f32.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "weiszfeld.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the two columns of a packed dword -> fp32, exactly
template <bool BF>
__device__ __forceinline__ float widen_lo(uint32_t v) {
  if constexpr (BF) return __uint_as_float(v << 16);
  return float(__builtin_bit_cast(_Float16, uint16_t(v)));
}
template <bool BF>
__device__ __forceinline__ float widen_hi(uint32_t v) {
  if constexpr (BF) return __uint_as_float(v & 0xffff0000u);
  return float(__builtin_bit_cast(_Float16, uint16_t(v >> 16)));
}

// geomed.hip's part<> for a packed pair of columns: at M == B the sum of the
// two exact fp64 squares of the fp32 differences (+0 from a half past the
// chunk's end), else the fold of slots J and J + M of the level above.
template <bool BF, int KMAX, int BASE, int B, int M, int J>
__device__ __forceinline__ double part2(const uint32_t (&x)[KMAX], float z0, float z1, uint32_t live0, uint32_t live1,
                                        int lane) {
  if constexpr (M == B) {
    const float d0 = __uint_as_float(__float_as_uint(widen_lo<BF>(x[BASE + J]) - z0) & live0);
    const float d1 = __uint_as_float(__float_as_uint(widen_hi<BF>(x[BASE + J]) - z1) & live1);
    const double e0 = double(d0), e1 = double(d1);
    return e0 * e0 + e1 * e1;  // exact squares, one fp64 rounding
  } else {
    const double a = part2<BF, KMAX, BASE, B, 2 * M, J>(x, z0, z1, live0, live1, lane);
    const double b = part2<BF, KMAX, BASE, B, 2 * M, J + M>(x, z0, z1, live0, live1, lane);
    const double r = fold<M>(a, b, lane);
    // A leaf passes through two floats and two doubles on its way from one
    // dword to one double: eight leaves are folded before the next eight are
    // widened, or the scheduler widens them all first (400 registers and more
    // at the 128-client tier).
    if constexpr (M * 8 == B) __builtin_amdgcn_sched_barrier(0);
    return r;
  }
}

// BF: bf16 rows (else f16); FULL: K == KMAX, no slot past K
template <bool BF, int KMAX, bool FULL>
__global__ __launch_bounds__(kBS, FULL ? 3 : 2) void wsum_dist2_16_kernel(const uint16_t* const* __restrict__ src,
                                                            const float* __restrict__ wdev, const InlW winl, int K,
                                                            const int64_t* __restrict__ chunks, int64_t n_chunks,
                                                            int G, float* __restrict__ z,
                                                            double* __restrict__ partial) {
  constexpr int B = KMAX < 64 ? KMAX : 64;  // clients per transposed batch
  constexpr int NB = KMAX / B;
  __shared__ double red[kWaves][KMAX];
  __shared__ float sw[KMAX];
  __shared__ uint32_t sm[FULL ? 1 : KMAX];  // a slot past K: packed dword & 0, weight -0
  if constexpr (FULL) K = KMAX;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int odd = 0;  // a row pointer that is not 4-byte aligned: no dword loads in this call
  for (int i = threadIdx.x; i < KMAX; i += kBS) {
    sw[i] = i < K ? (wdev ? wdev[i] : winl.v[i]) : -0.f;
    if constexpr (!FULL) sm[i] = i < K ? 0xffffffffu : 0u;
    if (i < K) odd |= int(reinterpret_cast<uintptr_t>(src[i]) & 3);
  }
  const bool rows_al = __syncthreads_or(odd) == 0;
  double acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = 0.0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += G) {
    const int64_t start = chunks[2 * c];
    const int len = int(chunks[2 * c + 1]);  // 1 .. FEDAGG_DIST_CHUNK
    const bool dw = rows_al && (start & 1) == 0;  // block-uniform: the chunk's form
    const bool z8 = (reinterpret_cast<uintptr_t>(z + start) & 7) == 0;
    const int gcols = dw ? 128 : 64, cpl = dw ? 2 : 1;  // columns per group and per lane
    for (int col0 = wave * gcols; col0 < len; col0 += kWaves * gcols) {
      const int e0 = col0 + cpl * lane;  // the lane's first column
      const bool live0 = e0 < len, live1 = dw && e0 + 1 < len;
      const bool whole = dw && col0 + 128 <= len;  // wave-uniform: every half-lane live
      // a half-lane past the chunk's end re-reads a column of the chunk
      // (inside the table), contributes 0 and stores nothing
      const uint32_t off0 = live0 ? uint32_t(e0) : 0u, off1 = live1 ? uint32_t(e0 + 1) : off0;
      const auto tab = fresh_table(src);
      int kk = K;  // the clamped slot indices are loop-invariant too
      if constexpr (!FULL) asm volatile("" : "+s"(kk));
      uint32_t x[KMAX];
      if (whole) {
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
          // at most 16 row pointers live in SGPRs at a time (see trimmed.hip)
          if (!FULL && i % 16 == 0 && i) __builtin_amdgcn_sched_barrier(0);
          const uint16_t* p = tab[FULL || i < kk ? i : 0] + start;  // 4-byte aligned: rows_al, even start
          x[i] = __builtin_nontemporal_load(gptr(reinterpret_cast<const uint32_t*>(p)) + (off0 >> 1));
        }
      } else {
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
          // two loads a client: packed eight clients at a time, so the halves
          // in flight stay far below the whole groups' register count
          if (i % 8 == 0 && i) __builtin_amdgcn_sched_barrier(0);
          const uint16_t* p = tab[FULL || i < kk ? i : 0] + start;
          const uint32_t lo = __builtin_nontemporal_load(gptr(p) + off0);
          const uint32_t hi = __builtin_nontemporal_load(gptr(p) + off1);
          x[i] = lo | (hi << 16);
        }
      }
      uint32_t wo = 0;
      asm volatile("" : "+v"(wo));
      const float* wp = sw + wo;
      if constexpr (!FULL) {
        const uint32_t* mp = sm + wo;
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
          if (i % 16 == 0 && i) __builtin_amdgcn_sched_barrier(0);  // 16 masks in flight, not KMAX
          x[i] &= mp[i];  // once per dword: both halves
          asm volatile("" : "+v"(x[i]));  // (not folded into the halves' own masks and shifts)
        }
      }
      // fedagg_wsum_f32's chain on either column: two roundings per client, never an FMA
      float a0 = widen_lo<BF>(x[0]) * wp[0], a1 = widen_hi<BF>(x[0]) * wp[0];
#pragma unroll
      for (int i = 1; i < KMAX; ++i) {
        if (i % 8 == 0) __builtin_amdgcn_sched_barrier(0);  // as in part2: no 2 KMAX products ahead of the adds
        const float w = wp[i];
        a0 = a0 + widen_lo<BF>(x[i]) * w;
        a1 = a1 + widen_hi<BF>(x[i]) * w;
      }
      // The distances widen the packed dwords again.  Without this the
      // compiler keeps the chain's 2 KMAX widened values for them instead of
      // the KMAX dwords (one wave per SIMD at the 128-client tier).
#pragma unroll
      for (int i = 0; i < KMAX; ++i) asm volatile("" : "+v"(x[i]));
      float* zp = z + start + e0;
      if (z8 && live1) {
        *reinterpret_cast<f32x2*>(zp) = f32x2{a0, a1};  // e0 is even here
      } else {
        if (live0) zp[0] = a0;
        if (live1) zp[1] = a1;
      }
      uint32_t lm0 = live0 ? 0xffffffffu : 0u, lm1 = live1 ? 0xffffffffu : 0u;
      asm volatile("" : "+v"(lm0), "+v"(lm1));  // kept masks: one v_and per difference
      if constexpr (NB >= 1) acc[0] += part2<BF, KMAX, 0, B, 1, 0>(x, a0, a1, lm0, lm1, lane);
      if constexpr (NB >= 2) acc[1] += part2<BF, KMAX, 64, B, 1, 0>(x, a0, a1, lm0, lm1, lane);
    }
  }
  if constexpr (B < 64) {  // the lanes' B-aligned groups, in a fixed order
#pragma unroll
    for (int m = B; m < 64; m <<= 1) acc[0] += __shfl_xor(acc[0], m, 64);
  }
  if (lane < B) {
#pragma unroll
    for (int b = 0; b < NB; ++b) red[wave][b * 64 + lane] = acc[b];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += kBS)
    partial[int64_t(blockIdx.x) * K + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

struct Args {
  const uint16_t* const* src;
  const float* wdev;
  InlW winl;
  int K;
  const int64_t* chunks;
  int64_t n_chunks;
  int G;
  float* z;
  double* work;
  hipStream_t st;
};

template <bool BF, int KMAX>
void launch_tier(const Args& a) {
  if (a.K == KMAX)
    hipLaunchKernelGGL((wsum_dist2_16_kernel<BF, KMAX, true>), dim3(unsigned(a.G)), dim3(kBS), 0, a.st, a.src, a.wdev,
                       a.winl, a.K, a.chunks, a.n_chunks, a.G, a.z, a.work);
  else
    hipLaunchKernelGGL((wsum_dist2_16_kernel<BF, KMAX, false>), dim3(unsigned(a.G)), dim3(kBS), 0, a.st, a.src,
                       a.wdev, a.winl, a.K, a.chunks, a.n_chunks, a.G, a.z, a.work);
}

template <bool BF>
void launch_k(const Args& a) {
  if (a.K <= 8) return launch_tier<BF, 8>(a);
  if (a.K <= 16) return launch_tier<BF, 16>(a);
  if (a.K <= 32) return launch_tier<BF, 32>(a);
  if (a.K <= 64) return launch_tier<BF, 64>(a);
  return launch_tier<BF, 128>(a);
}

}  // namespace

extern "C" int fedagg_wsum_dist2_16(int32_t dtype, const void* const* d_src, const float* d_w, int32_t K,
                                    const int64_t* d_chunks, int64_t n_chunks, float* d_z, double* d_dist2,
                                    double* d_work, int64_t work_len, uint32_t flags, fedagg_stream_t stream) {
  if (dtype != FEDAGG_DT_BF16 && dtype != FEDAGG_DT_F16)
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
  if (K < 1 || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_16: K must be >= 1 and n_chunks >= 0");
  if (!d_src || !d_w || !d_z || !d_dist2 || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_16: null pointer");
  if (K > FEDAGG_GEOMED_MAX_CLIENTS)
    return set_error(FEDAGG_ENOKERNEL, "fedagg_wsum_dist2_16: the kernel holds at most " +
                                           std::to_string(FEDAGG_GEOMED_MAX_CLIENTS) + " clients (K = " +
                                           std::to_string(K) + "): widen the rows and run the fp32 passes");
  if (n_chunks > 0 && work_len < K)
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_16: workspace smaller than K doubles");
  auto st = reinterpret_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_dist2, 0, sizeof(double) * K, st) != hipSuccess) return check_launch("fedagg_wsum_dist2_16");
    return FEDAGG_OK;
  }
  Args a;
  a.src = reinterpret_cast<const uint16_t* const*>(d_src);
  const bool host_w = (flags & FEDAGG_HOST_WEIGHTS) != 0;
  a.wdev = host_w ? nullptr : d_w;
  for (int i = 0; i < FEDAGG_GEOMED_MAX_CLIENTS; ++i) a.winl.v[i] = host_w && i < K ? d_w[i] : 0.f;
  a.K = K;
  a.chunks = d_chunks;
  a.n_chunks = n_chunks;
  a.G = groups_for(K, n_chunks, work_len);
  a.z = d_z;
  a.work = d_work;
  a.st = st;
  if (dtype == FEDAGG_DT_BF16)
    launch_k<true>(a);
  else
    launch_k<false>(a);
  hipLaunchKernelGGL(wd_finish_kernel, dim3(unsigned(K)), dim3(256), 0, st, d_work, a.G, K, d_dist2);
  return check_launch("fedagg_wsum_dist2_16");
}
