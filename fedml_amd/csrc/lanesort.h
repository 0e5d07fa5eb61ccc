// lanesort.h — what the lane-group kernels above 128 clients share: P adjacent
// lanes hold one column, each R of its P·R values in registers (slot
// s = sub·R + j), their addresses in the block's LDS slot table
// (lanes_slot_ptr).  Every lane sorts its R values with the pairwise network
// (sortnet.h); the sorted runs are then merged across lanes by reverse pairing
// plus half-cleaner stages (single DPP movs and v_med3 against ±inf), one level
// per doubling of the lane group.  median.hip describes the scheme where it
// prunes the last level (median_lanes_kernel); trimmed_wide.hip and
// nearmedian_wide.hip run every level (lanes_sort_all).  On the host: the
// launch (launch_lanes) and the tiers of 129 to 1024 clients (with_lane_tier).
// Everything is internal to the including translation unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sortnet.h"

// Loads of the lane-group kernels: a wave instruction reads 64 B of each of P
// rows' 128-B lines and the block's next wave reads the other half, so plain
// loads (0) keep the line in L2 for it; non-temporal ones (1) fetched 1.04-1.5x
// the algorithmic bytes vs 1.00-1.03x, at the same time
// (profiles/r03/lanes_nt/)
constexpr int kLanesNT = 0;

namespace {

// loads of the lane-group kernels (kLanesNT)
template <class T>
__device__ __forceinline__ T lanes_load(const T __attribute__((address_space(1)))* p) {
  if constexpr (kLanesNT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}

// Address of slot j of lane `sub`, as a T, at byte offset boff of the rows (a
// padded slot: of its constant).  The table is skewed by kLanesSkew entries per
// lane group (median_lanes_kernel, which stages it, says why).
constexpr int kLanesSkew = 2;
template <int R, bool FULL, class T, class S>
__device__ __forceinline__ const T __attribute__((address_space(1)))* lanes_slot_ptr(
    const S* const* rows, const uint64_t* offmask, int sub, int j, uint64_t boff) {
  const int q = sub * (R + kLanesSkew) + j;
  const uint64_t off = FULL ? boff : (boff & offmask[q]);
  return as_global(reinterpret_cast<const T*>(reinterpret_cast<const char*>(rows[q]) + off));
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ short2_t dpp_mov(short2_t x) {
  return __builtin_bit_cast(short2_t, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
template <int M>
constexpr int dpp_xor_ctrl() {
  static_assert(M == 1 || M == 2 || M == 3 || M == 7 || M == 15, "lane xor pattern without a single DPP mov");
  // quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0]; row_half_mirror; row_mirror
  return M == 1 ? 0xB1 : M == 2 ? 0x4E : M == 3 ? 0x1B : M == 7 ? 0x141 : 0x140;
}

// The value of lane ^ M: one DPP mov where a pattern exists (xor 1, 2, 3,
// 7, 15), two for xor 4 (xor 7 then xor 3), else ds_bpermute (xor 31: the
// last level of the 32-lane groups above 2,048 clients).
template <int M>
constexpr bool dpp_xor_ok() { return M == 1 || M == 2 || M == 3 || M == 7 || M == 15; }
template <int M>
__device__ __forceinline__ float xor_mov(float x) {
  if constexpr (dpp_xor_ok<M>()) return dpp_mov<dpp_xor_ctrl<M>()>(x);
  else if constexpr (M == 4) return dpp_mov<dpp_xor_ctrl<3>()>(dpp_mov<dpp_xor_ctrl<7>()>(x));  // (i ^ 7) ^ 3
  else return __int_as_float(__shfl_xor(__float_as_int(x), M, 64));
}

// sum of x over the P adjacent lanes of a column (every lane gets it)
template <int P>
__device__ __forceinline__ int lanes_count_sum(int x) {
  static_assert(P <= 16, "a lane group inside one DPP row");
  if constexpr (P >= 2) x += __builtin_amdgcn_mov_dpp(x, dpp_xor_ctrl<1>(), 0xF, 0xF, true);
  if constexpr (P >= 4) x += __builtin_amdgcn_mov_dpp(x, dpp_xor_ctrl<2>(), 0xF, 0xF, true);
  if constexpr (P >= 8) x += __builtin_amdgcn_mov_dpp(x, dpp_xor_ctrl<7>(), 0xF, 0xF, true);  // the other quad's sum
  if constexpr (P >= 16) x += __builtin_amdgcn_mov_dpp(x, dpp_xor_ctrl<15>(), 0xF, 0xF, true);  // the other half's
  return x;
}

// min (lower lanes, sel = -inf) or max (upper lanes, sel = +inf) of own
// register i and the partner lane's register R-1-i, for every i
template <int M, int R>
__device__ __forceinline__ void lanes_reverse_pair(float (&v)[R], float sel) {
  // opaque to the compiler: knowing sel is ±inf it splits every v_med3 into
  // min, max and a select (three ops and twice the live registers)
  asm volatile("" : "+v"(sel));
#pragma unroll
  for (int i = 0; i < R / 2; ++i) {
    const float a = xor_mov<M>(v[R - 1 - i]);
    const float b = xor_mov<M>(v[i]);
    v[i] = __builtin_amdgcn_fmed3f(v[i], a, sel);
    v[R - 1 - i] = __builtin_amdgcn_fmed3f(v[R - 1 - i], b, sel);
  }
}

// half-cleaner stage between lanes sub and sub ^ M, same register
template <int M, int R>
__device__ __forceinline__ void lanes_cross_stage(float (&v)[R], int sub) {
  float sel = (sub & M) ? __builtin_huge_valf() : -__builtin_huge_valf();
  asm volatile("" : "+v"(sel));
#pragma unroll
  for (int i = 0; i < R; ++i) v[i] = __builtin_amdgcn_fmed3f(v[i], xor_mov<M>(v[i]), sel);
}

// in-lane half-cleaner cascade: a bitonic register array -> ascending
template <int R>
__device__ __forceinline__ void lane_bitonic_merge(float (&v)[R]) {
#pragma unroll
  for (int d = R / 2; d > 0; d /= 2) {
#pragma unroll
    for (int i = 0; i < R; ++i)
      if ((i & d) == 0) cmpx(v[i], v[i + d]);
  }
}

// merge levels G = 2, 4, 8 (< P): afterwards every group of G lanes holds its
// G·R values sorted ascending over slots (sub % G)·R + j
template <int G, int P, int R>
__device__ __forceinline__ void lanes_merge_levels(float (&v)[R], int sub) {
  if constexpr (G < P) {
    static_assert(G <= 16, "lane groups of at most 32");
    lanes_reverse_pair<G - 1>(v, (sub & (G / 2)) ? __builtin_huge_valf() : -__builtin_huge_valf());
    if constexpr (G == 16) lanes_cross_stage<4>(v, sub);  // slot distance 4R
    if constexpr (G >= 8) lanes_cross_stage<2>(v, sub);  // slot distance 2R
    if constexpr (G >= 4) lanes_cross_stage<1>(v, sub);  // slot distance R
    lane_bitonic_merge(v);
    lanes_merge_levels<G * 2, P, R>(v, sub);
  }
}

// the in-lane network, then every merge level (G = P included): slot s holds rank s
template <int P, int R>
__device__ __forceinline__ void lanes_sort_all(float (&v)[R], int sub) {
  pairwise_sort<R>(v);
  lanes_merge_levels<2, 2 * P, R>(v, sub);
}

// Host side.  One launch over N columns, P lanes per column in blocks of BS:
// kernel(src, K, N, mid..., out), `full` when K is the tier's P·R, else `padded`.
// A grid past 2^31 - 1 blocks is "<what>: N too large".  As in launch_col_chunks
// the kernel's own arguments follow `out` here: a pack is deduced only at the end.
template <class Kern, class S, class... Mid>
int launch_lanes(const char* what, Kern full, Kern padded, bool is_full, int P, int BS, hipStream_t st,
                 const S* const* src, int K, int64_t N, S* out, Mid... mid) {
  if (N > int64_t(0x7fffffff) * BS / P) return set_error(FEDAGG_EINVAL, std::string(what) + ": N too large");
  const unsigned grid = unsigned((N * P + BS - 1) / BS);
  const Kern kernel = is_full ? full : padded;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(BS), 0, st, src, K, N, mid..., out);
  return check_launch(what);
}

// The tiers of 129 to 1024 clients (the callers bound K): f(P, R) as
// std::integral_constant<int, ..> values.  Each tier's call stands before the
// next tier's (with_tier, sortnet.h: the order the kernels are emitted in).
template <class F>
int with_lane_tier(int K, F f) {
  if (K <= 256) return f(std::integral_constant<int, 4>{}, std::integral_constant<int, 64>{});
  if (K <= 512) return f(std::integral_constant<int, 4>{}, std::integral_constant<int, 128>{});
  return f(std::integral_constant<int, 8>{}, std::integral_constant<int, 128>{});
}

}  // namespace
