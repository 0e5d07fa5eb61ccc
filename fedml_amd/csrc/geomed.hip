// geomed.hip — the fused Weiszfeld step of the geometric-median defense
// ("geomed"), exported through include/fedagg.h (fedagg_wsum_dist2_f32, where
// the operation is specified) and linked into libfedagg.so.  Its own
// translation unit, so robust.hip's device code stays as it was.
//
// One Weiszfeld iteration is "weighted sum z of the K rows, then every
// client's squared distance to z".  fedagg_wsum_f32 followed by
// fedagg_dist2_f32(ref = z) reads the K rows from HBM twice; a column's z is
// complete once its K values have been seen, so here both come from one read.
//
// Layout (trimmed.hip's: one lane per column, the column's K values in KMAX
// registers, K tiers 8 .. 128).  A block owns the chunks g, g + G, ... of the
// chunk table; per chunk its four waves take the 64-column groups w, w + 4, ...
// A lane loads its column's K values (every load one coalesced 256-byte row
// segment with a wave-uniform base), forms the fedagg_wsum_f32 chain, stores
// z, and then holds K squared differences in fp64 whose sums over the wave's
// 64 columns are wanted.  A butterfly per client would cost 6 exchanges per
// client; the transposing reduction costs about one: at mask m = 32, 16, .. 1
// lane l keeps the clients whose bit m equals l's bit m and hands the others
// to lane l ^ m, so the count of live values halves per step and after six
// steps lane l holds the wave's total of client l (of each batch of 64).
// The two widest steps, which carry three quarters of the exchanges, are
// v_permlane32_swap / v_permlane16_swap (one VALU op per dword, no select);
// the narrow ones are a select pair and a ds_bpermute.  Only KMAX / 64 fp64
// accumulators per lane persist across the wave's loop.
//
// A block adds its four waves' totals in a fixed order and writes K partials
// to the workspace; wd_finish_kernel sums the blocks' partials in a fixed
// order.  No atomics: two calls on the same inputs give the same bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fedagg.h"
#include "host_util.h"

extern "C" __attribute__((visibility("hidden"))) int64_t fedagg_wsum_dist2_work_len_internal(int32_t K,
                                                                                             int64_t n_chunks);

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

// The wave's partial of slot J at mask M over the batch of B clients starting
// at BASE: the raw fp64 square at M == B, else the fold of slots J and J + M
// of the level above.  part<.., 1, 0> leaves client BASE + (lane & (B - 1))
// in the lane, summed over the lanes of its B-aligned group.
template <int KMAX, int BASE, int B, int M, int J>
__device__ __forceinline__ double part(const float (&x)[KMAX], float z, uint32_t live, int lane) {
  if constexpr (M == B) {
    // the reference's fp32 difference; +0 in a lane past the chunk's end (a
    // bit mask: a select was sunk behind the conversion, onto both dwords)
    const float d = __uint_as_float(__float_as_uint(x[BASE + J] - z) & live);
    const double dd = double(d);
    return dd * dd;  // exact in fp64
  } else {
    const double a = part<KMAX, BASE, B, 2 * M, J>(x, z, live, lane);
    const double b = part<KMAX, BASE, B, 2 * M, J + M>(x, z, live, lane);
    return fold<M>(a, b, lane);
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
typedef const float* rowptr_t;
__device__ __forceinline__ const rowptr_t __attribute__((address_space(4)))* fresh_table(const float* const* src) {
  uint64_t a = reinterpret_cast<uint64_t>(src);
  asm volatile("" : "+s"(a));
  return reinterpret_cast<const rowptr_t __attribute__((address_space(4)))*>(a);
}

// FULL: K == KMAX, no slot past K and so no per-client conditions
template <int KMAX, bool FULL>
__global__ __launch_bounds__(kBS) void wsum_dist2_kernel(const float* const* __restrict__ src,
                                                         const float* __restrict__ wdev, const InlW winl, int K,
                                                         const int64_t* __restrict__ chunks, int64_t n_chunks, int G,
                                                         float* __restrict__ z, double* __restrict__ partial) {
  constexpr int B = KMAX < 64 ? KMAX : 64;  // clients per transposed batch
  constexpr int NB = KMAX / B;
  __shared__ double red[kWaves][KMAX];
  __shared__ float sw[KMAX];
  if constexpr (FULL) K = KMAX;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // A slot past K reads row 0 again (whatever it holds), is masked to +0 and
  // weighted by -0: fl(+0 * -0) = -0 and y + (-0) = y for every y, -0 and NaN
  // included, so it leaves the chain as it was without a condition per slot
  // (128 hoisted wave-uniform predicates spilled out of the SGPRs).
  __shared__ uint32_t sm[FULL ? 1 : KMAX];
  for (int i = threadIdx.x; i < KMAX; i += kBS) {
    sw[i] = i < K ? (wdev ? wdev[i] : winl.v[i]) : -0.f;
    if constexpr (!FULL) sm[i] = i < K ? 0xffffffffu : 0u;
  }
  __syncthreads();
  double acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = 0.0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += G) {
    const int64_t start = chunks[2 * c];
    const int len = int(chunks[2 * c + 1]);  // 1 .. FEDAGG_DIST_CHUNK
    for (int col0 = wave * 64; col0 < len; col0 += kBS) {
      const int col = col0 + lane;
      const bool live = col < len;
      // a lane past the chunk's end reads the chunk's first column (inside
      // the table), contributes 0 and stores nothing
      const uint32_t off = live ? uint32_t(col) : 0u;
      const auto tab = fresh_table(src);
      int kk = K;  // the clamped slot indices are loop-invariant too
      if constexpr (!FULL) asm volatile("" : "+s"(kk));
      float x[KMAX];
#pragma unroll
      for (int i = 0; i < KMAX; ++i) {
        // at most 16 row pointers live in SGPRs at a time (see trimmed.hip)
        if (!FULL && i % 16 == 0 && i) __builtin_amdgcn_sched_barrier(0);
        const float* p = tab[FULL || i < kk ? i : 0] + start;
        x[i] = __builtin_nontemporal_load(gptr(p) + off);
      }
      uint32_t wo = 0;
      asm volatile("" : "+v"(wo));
      const float* wp = sw + wo;
      if constexpr (!FULL) {
        const uint32_t* mp = sm + wo;
#pragma unroll
        for (int i = 0; i < KMAX; ++i) x[i] = __uint_as_float(__float_as_uint(x[i]) & mp[i]);
      }
      // fedagg_wsum_f32's chain: two roundings per client, never an FMA
      float a = x[0] * wp[0];
#pragma unroll
      for (int i = 1; i < KMAX; ++i) a = a + x[i] * wp[i];
      if (live) z[start + col] = a;
      uint32_t lm = live ? 0xffffffffu : 0u;
      asm volatile("" : "+v"(lm));  // kept a mask: one v_and per client
      if constexpr (NB >= 1) acc[0] += part<KMAX, 0, B, 1, 0>(x, a, lm, lane);
      if constexpr (NB >= 2) acc[1] += part<KMAX, 64, B, 1, 0>(x, a, lm, lane);
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

int groups_for(int32_t K, int64_t n_chunks, int64_t work_len) {
  int64_t G = n_chunks < kMaxGroups ? n_chunks : kMaxGroups;
  if (work_len >= 0 && G > work_len / K) G = work_len / K;
  return int(G);
}

template <int KMAX>
void launch_tier(const float* const* src, const float* wdev, const InlW& winl, int K, const int64_t* chunks,
                 int64_t n_chunks, int G, float* z, double* work, hipStream_t st) {
  if (K == KMAX)
    hipLaunchKernelGGL((wsum_dist2_kernel<KMAX, true>), dim3(unsigned(G)), dim3(kBS), 0, st, src, wdev, winl, K,
                       chunks, n_chunks, G, z, work);
  else
    hipLaunchKernelGGL((wsum_dist2_kernel<KMAX, false>), dim3(unsigned(G)), dim3(kBS), 0, st, src, wdev, winl, K,
                       chunks, n_chunks, G, z, work);
}

void launch_k(const float* const* src, const float* wdev, const InlW& winl, int K, const int64_t* chunks,
              int64_t n_chunks, int G, float* z, double* work, hipStream_t st) {
  if (K <= 8) return launch_tier<8>(src, wdev, winl, K, chunks, n_chunks, G, z, work, st);
  if (K <= 16) return launch_tier<16>(src, wdev, winl, K, chunks, n_chunks, G, z, work, st);
  if (K <= 32) return launch_tier<32>(src, wdev, winl, K, chunks, n_chunks, G, z, work, st);
  if (K <= 64) return launch_tier<64>(src, wdev, winl, K, chunks, n_chunks, G, z, work, st);
  return launch_tier<128>(src, wdev, winl, K, chunks, n_chunks, G, z, work, st);
}

}  // namespace

extern "C" {

int64_t fedagg_wsum_dist2_work_len_internal(int32_t K, int64_t n_chunks) {
  if (K < 1 || K > FEDAGG_GEOMED_MAX_CLIENTS || n_chunks < 0) return -1;
  return int64_t(K) * groups_for(K, n_chunks, -1);
}

int fedagg_wsum_dist2_f32(const float* const* d_src, const float* d_w, int32_t K, const int64_t* d_chunks,
                          int64_t n_chunks, float* d_z, double* d_dist2, double* d_work, int64_t work_len,
                          uint32_t flags, fedagg_stream_t stream) {
  if (K < 1 || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_f32: K must be >= 1 and n_chunks >= 0");
  if (!d_src || !d_w || !d_z || !d_dist2 || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_f32: null pointer");
  if (K > FEDAGG_GEOMED_MAX_CLIENTS)
    return set_error(FEDAGG_ENOKERNEL, "fedagg_wsum_dist2_f32: the kernel holds at most " +
                                           std::to_string(FEDAGG_GEOMED_MAX_CLIENTS) + " clients (K = " +
                                           std::to_string(K) + "): run fedagg_wsum_f32, then fedagg_dist2_f32");
  if (n_chunks > 0 && work_len < K)
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_dist2_f32: workspace smaller than K doubles");
  auto st = reinterpret_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_dist2, 0, sizeof(double) * K, st) != hipSuccess) return check_launch("fedagg_wsum_dist2_f32");
    return FEDAGG_OK;
  }
  // one lane per column and 4-byte accesses: the same code, and so the same
  // arithmetic, for every alignment (FEDAGG_ALIGNED16 changes nothing)
  const int G = groups_for(K, n_chunks, work_len);
  InlW iw;
  const bool host_w = (flags & FEDAGG_HOST_WEIGHTS) != 0;
  for (int i = 0; i < FEDAGG_GEOMED_MAX_CLIENTS; ++i) iw.v[i] = host_w && i < K ? d_w[i] : 0.f;
  launch_k(d_src, host_w ? nullptr : d_w, iw, K, d_chunks, n_chunks, G, d_z, d_work, st);
  hipLaunchKernelGGL(wd_finish_kernel, dim3(unsigned(K)), dim3(256), 0, st, d_work, G, K, d_dist2);
  return check_launch("fedagg_wsum_dist2_f32");
}

}  // extern "C"
