// lanesort.h — the lane-group sort that the kernels above 128 clients share:
// P adjacent lanes hold one column, each R of its P·R values in registers
// (slot s = sub·R + j).  Every lane sorts its R values with the pairwise
// network (sortnet.h); the sorted runs are then merged across lanes by reverse
// pairing plus half-cleaner stages (single DPP movs and v_med3 against ±inf),
// one level per doubling of the lane group.  median.hip describes the scheme
// where it prunes the last level (median_lanes_kernel); trimmed_wide.hip and
// nearmedian_wide.hip run every level.  Everything is internal to the
// including translation unit.
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

}  // namespace
