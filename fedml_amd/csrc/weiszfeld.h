// weiszfeld.h — what the fused Weiszfeld-step units share (geomed.hip: fp32
// rows; geomed16.hip: bf16 / f16 rows): the block shape, the weights carried
// in the kernel arguments, one step of the transposing reduction, the
// pointer-table trick, the finish kernel and the chunk-group rule.  Everything
// here is internal to the including unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedagg.h"

namespace {

constexpr int kBS = 256;
constexpr int kWaves = kBS / 64;
// at most this many blocks (chunk groups), four per CU, each streaming its
// chunks g, g + G, ... start to end (three are resident per CU at the
// 128-client tier's register count); the one value tried
constexpr int kMaxGroups = 1024;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// weights carried in the kernel arguments (FEDAGG_HOST_WEIGHTS)
struct InlW {
  float v[FEDAGG_GEOMED_MAX_CLIENTS];
};

// a and b are this lane's values of two clients whose indices differ in bit
// M: afterwards the lane holds, for the one of the two whose bit M equals the
// lane's bit M, the sum of its own value and lane ^ M's.
template <int M>
__device__ __forceinline__ double fold(double a, double b, int lane) {
  if constexpr (M == 32 || M == 16) {
    // v_permlane32_swap: lanes 32-63 of the first operand <-> lanes 0-31 of
    // the second; v_permlane16_swap: odd 16-lane rows of the first <-> even
    // rows of the second.  Either way the first then holds {a, b} of the
    // lanes with bit M clear and the second {a, b} of those with it set.
    uint32_t alo = uint32_t(__double2loint(a)), ahi = uint32_t(__double2hiint(a));
    uint32_t blo = uint32_t(__double2loint(b)), bhi = uint32_t(__double2hiint(b));
    u32x2 lo, hi;
    if constexpr (M == 32) {
      lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
      hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    } else {
      lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
      hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    }
    return __hiloint2double(int(hi[0]), int(lo[0])) + __hiloint2double(int(hi[1]), int(lo[1]));
  } else {
    const bool up = (lane & M) != 0;
    const double keep = up ? b : a, send = up ? a : b;
    return keep + __shfl_xor(send, M, 64);
  }
}

template <class T>
__device__ __forceinline__ const T __attribute__((address_space(1)))* gptr(const T* p) {
  return (const T __attribute__((address_space(1)))*)(p);
}

// Loop-invariant scalar values are hoisted out of the column loop by the
// compiler, and 128 row pointers plus 128 weights do not fit the SGPRs (the
// first version spilled ~1,000 of them to VGPR lanes).  So the pointer table's
// address passes through an empty asm once per column group: its entries are
// re-read there (s_load from the scalar cache, 16 pointers per instruction at
// K == KMAX) and live only until their row's load is issued.  The weights sit
// in LDS (copied once per block from the device array or from the kernel
// arguments) and are read as broadcast LDS reads, their offset hidden in the
// same way.
template <class T>
__device__ __forceinline__ const T* const __attribute__((address_space(4)))* fresh_table(const T* const* src) {
  uint64_t a = reinterpret_cast<uint64_t>(src);
  asm volatile("" : "+s"(a));
  return reinterpret_cast<const T* const __attribute__((address_space(4)))*>(a);
}

// out[i] = sum over the G blocks of partial[g][i]: one block per client,
// thread t adds g = t, t + 256, ... in order, then a fixed LDS tree
__global__ __launch_bounds__(256) void wd_finish_kernel(const double* __restrict__ partial, int G, int K,
                                                        double* __restrict__ out) {
  __shared__ double red[256];
  const int i = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int g = t; g < G; g += 256) s += partial[int64_t(g) * K + i];
  red[t] = s;
  __syncthreads();
#pragma unroll
  for (int m = 128; m > 0; m >>= 1) {
    if (t < m) red[t] += red[t + m];
    __syncthreads();
  }
  if (t == 0) out[i] = red[0];
}

[[maybe_unused]] int groups_for(int32_t K, int64_t n_chunks, int64_t work_len) {
  int64_t G = n_chunks < kMaxGroups ? n_chunks : kMaxGroups;
  if (work_len >= 0 && G > work_len / K) G = work_len / K;
  return int(G);
}

}  // namespace
