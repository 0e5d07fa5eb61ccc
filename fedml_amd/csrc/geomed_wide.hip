// geomed_wide.hip — the fused Weiszfeld step of the geometric-median defense
// for 129 to 1024 clients, on fp32 rows and on bf16 / f16 rows that stay
// 16-bit on the card, exported through include/fedagg.h
// (fedagg_wsum_dist2_wide_f32 / fedagg_wsum_dist2_wide_16; the operation is
// specified at fedagg_wsum_dist2_f32 / _16) and linked into libfedagg.so.  It
// shares fold<>, wd_finish_kernel and the chunk-group rule with geomed.hip and
// geomed16.hip (weiszfeld.h); the kernel is its own.
//
// A column's K values no longer fit one lane, so a column is held by a LANE
// GROUP, the shape trimmed_wide.hip and nearmedian_wide.hip use for this range:
//
//   Layout.  P = 2, 4 or 8 lanes share a column (K <= 256, 512, 1024); lane
//   `sub` holds slots sub·128 .. sub·128 + 127 in 128 registers.  An fp32 row
//   gives one column per lane group, a 16-bit row one packed dword (two
//   adjacent columns) with geomed16.hip's widening, alignment rule and element
//   form for odd starts, unaligned rows and a chunk's last partial group.  A
//   wave covers 64 / P groups, a block's four waves adjacent ones, so at P = 8
//   the block still consumes whole 128-byte lines of every row.
//
//   Lane order: ADJACENT, sub = lane & (P - 1).  The lanes that hold the same
//   slots for other columns are then lane ^ P, ^ 2P, .. ^ 32, and the
//   transposing reduction over them runs its two widest levels, which carry
//   three quarters (P = 2) to all but one eighth (P = 8) of the exchanges, as
//   v_permlane32_swap / v_permlane16_swap; strided groups would push every
//   level down to masks 1 .. 32 / P, where a 64-bit exchange is a select pair
//   and two ds_bpermutes.  The price is the loads: a wave instruction touches P
//   rows, so the row pointer is per lane (the LDS slot table below) and not a
//   scalar base.
//
//   Parameters.  The 1024 row pointers cannot live in SGPRs and P of them are
//   needed per instruction, so they are staged in LDS once per block together
//   with the weights and the padding masks, lane sub's 128 entries skewed by 4
//   entries from lane sub - 1's (a group's P reads of one instruction then fall
//   on different banks, and the 16-byte reads stay aligned).  The table's
//   offset passes through an empty asm per column group and per phase:
//   otherwise the loop-invariant LDS reads are hoisted into registers.
//
//   Padding.  A slot past K re-reads row 0, is masked to +0 once and carries
//   weight -0 (geomed.hip's trick); FULL kernels (K == KMAX) skip the masks.
//
//   Chain.  fedagg_wsum_f32's chain crosses the lanes, so it runs in P phases
//   (trimmed_mean_lanes_kernel's scheme): in phase p every lane starts from
//   the value lane p - 1 ended with and adds its 128 products in order; lane
//   p's result is handed on and lane P - 1's is z, which every lane of the
//   group then has.  Phase 0 starts with the product itself (0 + -0 would turn
//   a column of -0 into +0).  A phase whose slots are all past K is skipped
//   (K is uniform; its products are all -0).
//
//   Distances.  Every lane forms the differences of its 128 slots against z
//   and enters fold<M> at M = 32, 16, .., P: log2(64 / P) levels, after which
//   lane (g, sub) holds, for each a < 2P, client sub·128 + a·(64 / P) + g summed
//   over the wave's columns: 2P = KMAX / 64 fp64 accumulators that persist
//   across the block's chunk loop.  Per-block partials, then wd_finish_kernel.
//
// This unit is compiled without packed fp32 VALU instructions (build.py,
// UNIT_FLAGS, which gives the reason): the chains are v_mul_f32 / v_add_f32.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "weiszfeld.h"

extern "C" __attribute__((visibility("hidden"))) int64_t fedagg_wsum_dist2_wide_work_len_internal(int32_t K,
                                                                                                  int64_t n_chunks);

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

enum RowKind { kF32 = 0, kBF16 = 1, kF16 = 2 };
constexpr int kR = 128;   // slots per lane
constexpr int kSkew = 4;  // LDS entries between one lane's 128 and the next lane's

// the first (T == kF32: only) and second column of a lane's register -> fp32, exactly
template <int T>
__device__ __forceinline__ float widen_lo(uint32_t v) {
  if constexpr (T == kF32) return __uint_as_float(v);
  if constexpr (T == kBF16) return __uint_as_float(v << 16);
  return float(__builtin_bit_cast(_Float16, uint16_t(v)));
}
template <int T>
__device__ __forceinline__ float widen_hi(uint32_t v) {
  if constexpr (T == kBF16) return __uint_as_float(v & 0xffff0000u);
  return float(__builtin_bit_cast(_Float16, uint16_t(v >> 16)));
}

// geomed.hip's part<> / geomed16.hip's part2<> over the lanes of equal sub: at
// M == 64 the exact fp64 square(s) of slot J's fp32 difference(s) (+0 from a
// column past the chunk's end), else the fold of slots J and J + M / P of the
// level above.  partw<.., P, J> leaves slot J + lane / P in the lane.
template <int T, int P, int M, int J>
__device__ __forceinline__ double partw(const uint32_t (&x)[kR], float z0, float z1, uint32_t live0, uint32_t live1,
                                        int lane) {
  if constexpr (M == 64) {
    const float d0 = __uint_as_float(__float_as_uint(widen_lo<T>(x[J]) - z0) & live0);
    const double e0 = double(d0);
    if constexpr (T == kF32) {
      return e0 * e0;  // exact in fp64
    } else {
      const float d1 = __uint_as_float(__float_as_uint(widen_hi<T>(x[J]) - z1) & live1);
      const double e1 = double(d1);
      return e0 * e0 + e1 * e1;  // exact squares, one fp64 rounding
    }
  } else {
    const double a = partw<T, P, 2 * M, J>(x, z0, z1, live0, live1, lane);
    const double b = partw<T, P, 2 * M, J + M / P>(x, z0, z1, live0, live1, lane);
    const double r = fold<M>(a, b, lane);
    // eight leaves are folded before the next eight are widened (geomed16.hip)
    if constexpr (M == 8) __builtin_amdgcn_sched_barrier(0);
    return r;
  }
}

template <int T, int P, int A>
__device__ __forceinline__ void add_parts(double (&acc)[2 * P], const uint32_t (&x)[kR], float z0, float z1,
                                          uint32_t live0, uint32_t live1, int lane) {
  if constexpr (A < 2 * P) {
    acc[A] += partw<T, P, P, A * (64 / P)>(x, z0, z1, live0, live1, lane);
    add_parts<T, P, A + 1>(acc, x, z0, z1, live0, live1, lane);
  }
}

// T: the rows' element (RowKind); P lanes per column group; FULL: K == P·128
template <int T, int P, bool FULL>
__global__ __launch_bounds__(kBS, 2) void wsum_dist2_wide_kernel(const void* const* __restrict__ src,
                                                                 const float* __restrict__ wdev, int K,
                                                                 const int64_t* __restrict__ chunks,
                                                                 int64_t n_chunks, int G, float* __restrict__ z,
                                                                 double* __restrict__ partial) {
  static_assert(P == 2 || P == 4 || P == 8, "2, 4 or 8 lanes per column group");
  constexpr int KMAX = P * kR, GN = 64 / P, NA = 2 * P, NQ = P * (kR + kSkew);
  constexpr int ES = T == kF32 ? 4 : 2;  // bytes per element
  __shared__ double red[kWaves][KMAX];
  __shared__ const char* rows[NQ];  // slot q = sub·(128 + skew) + j: its row, ...
  __shared__ float sw[NQ];          // ... its weight (-0 past K) ...
  __shared__ uint32_t sm[FULL ? 1 : NQ];  // ... and its mask (0 past K)
  if constexpr (FULL) K = KMAX;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane & (P - 1), grp = lane / P, lane0 = lane & ~(P - 1);
  int odd = 0;  // 16-bit rows: a row pointer that is not 4-byte aligned, no dword loads in this call
  for (int i = threadIdx.x; i < KMAX; i += kBS) {
    const int q = i + kSkew * (i / kR);
    const void* p = src[i < K ? i : 0];
    rows[q] = static_cast<const char*>(p);
    sw[q] = i < K ? wdev[i] : -0.f;
    if constexpr (!FULL) sm[q] = i < K ? 0xffffffffu : 0u;
    if constexpr (T != kF32) odd |= int(reinterpret_cast<uintptr_t>(p) & 3);
  }
  const bool rows_al = __syncthreads_or(odd) == 0;
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += G) {
    const int64_t start = chunks[2 * c];
    const int len = int(chunks[2 * c + 1]);  // 1 .. FEDAGG_DIST_CHUNK
    // block-uniform: the chunk's form (dwords of two columns, or elements)
    const bool dw = T != kF32 && rows_al && (start & 1) == 0;
    const bool z8 = (reinterpret_cast<uintptr_t>(z + start) & 7) == 0;
    const int cpl = dw ? 2 : 1, gcols = cpl * GN;  // columns per lane group and per wave
    for (int col0 = wave * gcols; col0 < len; col0 += kWaves * gcols) {
      const int e0 = col0 + cpl * grp;  // the group's first column
      const bool live0 = e0 < len, live1 = dw && e0 + 1 < len;
      const bool whole = dw && col0 + gcols <= len;  // wave-uniform: every half live
      // a column past the chunk's end re-reads a column of the chunk (inside
      // the table), contributes 0 and stores nothing
      const uint32_t off0 = live0 ? uint32_t(e0) : 0u, off1 = live1 ? uint32_t(e0 + 1) : off0;
      const uint64_t b0 = uint64_t(start + off0) * ES, b1 = uint64_t(start + off1) * ES;
      uint32_t qo = uint32_t(sub) * (kR + kSkew);
      asm volatile("" : "+v"(qo));
      const char* const* rp = rows + qo;
      uint32_t x[kR];
      if (T == kF32 || whole) {
#pragma unroll
        for (int j = 0; j < kR; ++j) {
          if (j % 16 == 0 && j) __builtin_amdgcn_sched_barrier(0);  // 16 slot pointers in registers, not 128
          // 16-bit: 4-byte aligned (rows_al, even start, even e0)
          x[j] = *gptr(reinterpret_cast<const uint32_t*>(rp[j] + b0));
        }
      } else {
#pragma unroll
        for (int j = 0; j < kR; ++j) {
          if (j % 8 == 0 && j) __builtin_amdgcn_sched_barrier(0);  // two loads a slot (geomed16.hip)
          const uint32_t lo = *gptr(reinterpret_cast<const uint16_t*>(rp[j] + b0));
          const uint32_t hi = *gptr(reinterpret_cast<const uint16_t*>(rp[j] + b1));
          x[j] = lo | (hi << 16);
        }
      }
      if constexpr (!FULL) {
        uint32_t mo = qo;
        asm volatile("" : "+v"(mo));
        const uint32_t* mp = sm + mo;
#pragma unroll
        for (int j = 0; j < kR; ++j) {
          if (j % 16 == 0 && j) __builtin_amdgcn_sched_barrier(0);  // 16 masks in flight
          x[j] &= mp[j];  // once per register: both halves
          asm volatile("" : "+v"(x[j]));
        }
      }
      // fedagg_wsum_f32's chain, two roundings per client and never an FMA, in
      // P phases: c0 / c1 are what lane p - 1 ended with
      float c0 = 0.f, c1 = 0.f;
#pragma unroll
      for (int p = 0; p < P; ++p) {
        if (p == 0 || p * kR < K) {  // uniform: a later phase's slots are all past K
          uint32_t wo = qo;
          asm volatile("" : "+v"(wo));  // the weights are re-read per phase, not kept
          const float* wp = sw + wo;
          float a0, a1 = 0.f;
          if (p == 0) {
            a0 = widen_lo<T>(x[0]) * wp[0];
            if constexpr (T != kF32) a1 = widen_hi<T>(x[0]) * wp[0];
          } else {
            a0 = c0 + widen_lo<T>(x[0]) * wp[0];
            if constexpr (T != kF32) a1 = c1 + widen_hi<T>(x[0]) * wp[0];
          }
#pragma unroll
          for (int j = 1; j < kR; ++j) {
            if (j % 8 == 0) __builtin_amdgcn_sched_barrier(0);  // no 128 products ahead of the adds
            const float w = wp[j];
            a0 = a0 + widen_lo<T>(x[j]) * w;
            if constexpr (T != kF32) a1 = a1 + widen_hi<T>(x[j]) * w;
          }
          c0 = __shfl(a0, lane0 + p, 64);  // lane p's sum; the other lanes' are dropped
          if constexpr (T != kF32) c1 = __shfl(a1, lane0 + p, 64);
          // the next phase and the distances widen the registers again
          // instead of keeping this phase's widened values (geomed16.hip)
#pragma unroll
          for (int j = 0; j < kR; ++j) asm volatile("" : "+v"(x[j]));
        }
      }
      // phases are skipped from the top only, so c0 / c1 are lane P' - 1's:
      // z, in every lane of the group; lane 0 of the group stores it
      if (sub == 0) {
        float* zp = z + start + e0;
        if (T != kF32 && z8 && live1) {
          *reinterpret_cast<f32x2*>(zp) = f32x2{c0, c1};  // e0 is even here
        } else {
          if (live0) zp[0] = c0;
          if (live1) zp[1] = c1;
        }
      }
      uint32_t lm0 = live0 ? 0xffffffffu : 0u, lm1 = live1 ? 0xffffffffu : 0u;
      asm volatile("" : "+v"(lm0), "+v"(lm1));  // kept masks: one v_and per difference
      add_parts<T, P, 0>(acc, x, c0, c1, lm0, lm1, lane);
    }
  }
  // lane (grp, sub) holds clients sub·128 + a·GN + grp, a < NA: every client once per wave
#pragma unroll
  for (int a = 0; a < NA; ++a) red[wave][sub * kR + a * GN + grp] = acc[a];
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += kBS)
    partial[int64_t(blockIdx.x) * K + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

struct Args {
  const void* const* src;
  const float* w;
  int K;
  const int64_t* chunks;
  int64_t n_chunks;
  int G;
  float* z;
  double* work;
  hipStream_t st;
};

template <int T, int P>
void launch_tier(const Args& a) {
  if (a.K == P * kR)
    hipLaunchKernelGGL((wsum_dist2_wide_kernel<T, P, true>), dim3(unsigned(a.G)), dim3(kBS), 0, a.st, a.src, a.w, a.K,
                       a.chunks, a.n_chunks, a.G, a.z, a.work);
  else
    hipLaunchKernelGGL((wsum_dist2_wide_kernel<T, P, false>), dim3(unsigned(a.G)), dim3(kBS), 0, a.st, a.src, a.w,
                       a.K, a.chunks, a.n_chunks, a.G, a.z, a.work);
}

template <int T>
void launch_k(const Args& a) {
  if (a.K <= 2 * kR) return launch_tier<T, 2>(a);
  if (a.K <= 4 * kR) return launch_tier<T, 4>(a);
  return launch_tier<T, 8>(a);
}

// the checks and the launch of both entry points; kind: the rows' RowKind
int wsum_dist2_wide(const std::string& what, int kind, const void* const* d_src, const float* d_w, int32_t K,
                    const int64_t* d_chunks, int64_t n_chunks, float* d_z, double* d_dist2, double* d_work,
                    int64_t work_len, uint32_t flags, fedagg_stream_t stream) {
  if (K < 1 || n_chunks < 0) return set_error(FEDAGG_EINVAL, what + ": K must be >= 1 and n_chunks >= 0");
  if (!d_src || !d_w || !d_z || !d_dist2 || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, what + ": null pointer");
  if (flags & FEDAGG_HOST_WEIGHTS)
    return set_error(FEDAGG_EINVAL, what + ": FEDAGG_HOST_WEIGHTS is not taken here (the weights are K device floats)");
  if (K > FEDAGG_GEOMED_WIDE_MAX_CLIENTS)
    return set_error(FEDAGG_ENOKERNEL, what + ": the kernel holds at most " +
                                           std::to_string(FEDAGG_GEOMED_WIDE_MAX_CLIENTS) + " clients (K = " +
                                           std::to_string(K) + "): run the weighted sum, then the distances");
  if (n_chunks > 0 && work_len < K) return set_error(FEDAGG_EINVAL, what + ": workspace smaller than K doubles");
  auto st = reinterpret_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_dist2, 0, sizeof(double) * K, st) != hipSuccess) return check_launch(what.c_str());
    return FEDAGG_OK;
  }
  Args a{d_src, d_w, K, d_chunks, n_chunks, groups_for(K, n_chunks, work_len), d_z, d_work, st};
  if (kind == kF32)
    launch_k<kF32>(a);
  else if (kind == kBF16)
    launch_k<kBF16>(a);
  else
    launch_k<kF16>(a);
  hipLaunchKernelGGL(wd_finish_kernel, dim3(unsigned(K)), dim3(256), 0, st, d_work, a.G, K, d_dist2);
  return check_launch(what.c_str());
}

}  // namespace

extern "C" {

int64_t fedagg_wsum_dist2_wide_work_len_internal(int32_t K, int64_t n_chunks) {
  if (K < 1 || K > FEDAGG_GEOMED_WIDE_MAX_CLIENTS || n_chunks < 0) return -1;
  return int64_t(K) * groups_for(K, n_chunks, -1);
}

int fedagg_wsum_dist2_wide_f32(const float* const* d_src, const float* d_w, int32_t K, const int64_t* d_chunks,
                               int64_t n_chunks, float* d_z, double* d_dist2, double* d_work, int64_t work_len,
                               uint32_t flags, fedagg_stream_t stream) {
  return wsum_dist2_wide("fedagg_wsum_dist2_wide_f32", kF32, reinterpret_cast<const void* const*>(d_src), d_w, K,
                         d_chunks, n_chunks, d_z, d_dist2, d_work, work_len, flags, stream);
}

int fedagg_wsum_dist2_wide_16(int32_t dtype, const void* const* d_src, const float* d_w, int32_t K,
                              const int64_t* d_chunks, int64_t n_chunks, float* d_z, double* d_dist2, double* d_work,
                              int64_t work_len, uint32_t flags, fedagg_stream_t stream) {
  if (dtype != FEDAGG_DT_BF16 && dtype != FEDAGG_DT_F16)
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_wide_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
  return wsum_dist2_wide("fedagg_wsum_dist2_wide_16", dtype == FEDAGG_DT_BF16 ? kBF16 : kF16, d_src, d_w, K, d_chunks,
                         n_chunks, d_z, d_dist2, d_work, work_len, flags, stream);
}

}  // extern "C"
