// fltrust16.hip — the two passes of the FLTrust defense for bf16 / f16 rows,
// exported through include/fedagg.h (fedagg_dotnorm2_16, fedagg_wsum_diff_16,
// where the operations are specified) and linked into libfedagg.so beside
// robust.hip, which holds the fp32 pair.
//
// The rows stay 16-bit on the card and are widened exactly in registers; every
// operation after the load is the fp32 / fp64 one of the fp32 kernels.  The
// layouts are made for 16-bit rows, not the fp32 ones with a narrower load:
//
//   dotnorm2_16_kernel.  dotnorm2_kernel's split (a block owns the chunks
//   g, g + G, ... for every client, wave w streams clients w, w + 4, ...), but
//   a lane's sixteen columns of a 1,024-column chunk are two runs of eight
//   (columns lane*8 + 512u): a client's chunk is TWO 16-byte loads of raw
//   16-bit words, four VGPRs each, where the fp32 kernel holds sixteen.  The
//   reference and b = fl32(dir - ref) are widened once per chunk and stay in
//   registers as fp32; a client's packed pairs are widened as they are used
//   (bf16: v << 16 and v & 0xffff0000; f16: one v_cvt_f32_f16 per half).
//   A row takes the 16-byte loads where its chunk's first element lies on a
//   16-byte boundary (a 16-byte aligned row pointer and a chunk start that is
//   a multiple of 8, or any other pair that adds up to one), decided per row
//   and chunk, wave-uniform; every other row, and the runs of a ragged chunk
//   end, load 2-byte elements into the same packed registers, so nothing past
//   a chunk's last column is read and a column past it holds +0.  After the
//   load the two forms are the same instructions: the sums are the same bits
//   at every alignment.
//
//   wsum_diff_16_kernel.  A streaming kernel, every load and store
//   non-temporal: a thread owns kWdVec runs of eight columns of a tile
//   (2,048 columns apart: a wave's load is 1 KB contiguous) and keeps
//   kWdClients clients in flight, 4 x 2 16-byte loads per lane as the fp32
//   kernel's, over twice its columns.  The chain is fp32 per column; the
//   result is rounded once (v_cvt_pk_bf16_f32 / v_cvt_f16_f32, nearest even)
//   and leaves as one 16-byte store per run.
//
// This unit is compiled without packed fp32 VALU instructions (build.py,
// UNIT_FLAGS, which gives the reason): the differences and the chain are
// v_sub_f32 / v_mul_f32 / v_add_f32.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fedagg.h"
#include "host_util.h"

namespace {

constexpr int kBS = 256;
constexpr int kWaves = kBS / 64;
constexpr int kRuns = FEDAGG_DIST_CHUNK / (64 * 8);  // runs of eight columns per lane per chunk
static_assert(kRuns * 512 == FEDAGG_DIST_CHUNK, "a chunk is whole 512-column rounds of the wave");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <class T>
__device__ __forceinline__ const T __attribute__((address_space(1)))* gptr(const T* p) {
  return (const T __attribute__((address_space(1)))*)(p);
}

// the two columns of a packed pair -> fp32, exactly
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

// fp32 -> the rows' type, nearest even (overflow to inf for f16, NaN stays NaN)
template <bool BF>
__device__ __forceinline__ uint32_t narrow(float f) {
  if constexpr (BF) return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f));  // v_cvt_pk_bf16_f32
  return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));                  // v_cvt_f16_f32
}

// eight columns at p as four packed pairs: one 16-byte load (p 16-byte aligned)
template <bool NT>
__device__ __forceinline__ u32x4 ld8(const uint16_t* p) {
  const auto q = reinterpret_cast<const u32x4 __attribute__((address_space(1)))*>(gptr(p));
  if constexpr (NT) return __builtin_nontemporal_load(q);
  return *q;
}

// the same eight columns by 2-byte loads, those at or past `n` reading +0
template <bool NT, class I>
__device__ __forceinline__ u32x4 ld8_elems(const uint16_t* p, I col, I n) {
  u32x4 v;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    uint32_t lo = 0, hi = 0;
    if (col + 2 * h < n) lo = NT ? __builtin_nontemporal_load(gptr(p) + col + 2 * h) : gptr(p)[col + 2 * h];
    if (col + 2 * h + 1 < n) hi = NT ? __builtin_nontemporal_load(gptr(p) + col + 2 * h + 1) : gptr(p)[col + 2 * h + 1];
    v[h] = lo | (hi << 16);
  }
  return v;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Columns lane*8 + 512u (u < kRuns) of a chunk of `len` columns at `p`, packed.
template <bool NT>
__device__ __forceinline__ void load_chunk16(const uint16_t* p, int len, int lane, u32x4 (&v)[kRuns]) {
  const bool al = aligned16(p);
  if (al && len == FEDAGG_DIST_CHUNK) {  // wave-uniform: a full aligned chunk, no per-lane conditions
#pragma unroll
    for (int u = 0; u < kRuns; ++u) v[u] = ld8<NT>(p + lane * 8 + 512 * u);
    return;
  }
#pragma unroll
  for (int u = 0; u < kRuns; ++u) {
    const int c = lane * 8 + 512 * u;
    if (al && c + 8 <= len)
      v[u] = ld8<NT>(p + c);
    else
      v[u] = ld8_elems<NT, int>(p, c, len);
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ---------------------------------------------------------------------------
// Clients per wave per pass.  A client in flight is 8 VGPRs here (16 in the
// fp32 kernel), r and b 32, the accumulators 4 per client: 8 clients fit four
// waves per SIMD, 16 are held to three.  FEDAGG_DOTNORM16_BATCH builds the
// other size for tools/fltrust16_probe.py; the measured pair is in NOTES.md.
#ifndef FEDAGG_DOTNORM16_BATCH
#define FEDAGG_DOTNORM16_BATCH 8
#endif
constexpr int kDotBatch = FEDAGG_DOTNORM16_BATCH;
constexpr int kDotWavesPerSimd = kDotBatch <= 8 ? 4 : 3;

__device__ __forceinline__ void dot_norm(float x, float r, float b, double& dot, double& nrm) {
  const double a = double(x - r);          // the fp32 difference of the widened values, widened
  dot = __builtin_fma(a, double(b), dot);  // exact products, fp64 sums
  nrm = __builtin_fma(a, a, nrm);
}

template <bool BF>
__global__ __launch_bounds__(kBS, kDotWavesPerSimd) void dotnorm2_16_kernel(
    const uint16_t* const* __restrict__ src, int K, const uint16_t* __restrict__ ref,
    const uint16_t* __restrict__ dir, const int64_t* __restrict__ chunks, int64_t n_chunks, int G,
    double* __restrict__ partial) {
  const int g = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int cb = 0; cb < K; cb += kWaves * kDotBatch) {
    double dot[kDotBatch], nrm[kDotBatch];
#pragma unroll
    for (int j = 0; j < kDotBatch; ++j) dot[j] = nrm[j] = 0.0;
    for (int64_t c = g; c < n_chunks; c += G) {
      const int64_t start = chunks[2 * c];
      const int len = int(chunks[2 * c + 1]);
      float r[kRuns][8], b[kRuns][8];
      {
        // plain loads: all four waves read these two rows (L2 serves three of them)
        u32x4 rw[kRuns], dw[kRuns];
        load_chunk16<false>(ref + start, len, lane, rw);
        load_chunk16<false>(dir + start, len, lane, dw);
#pragma unroll
        for (int u = 0; u < kRuns; ++u) {
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            r[u][2 * h] = widen_lo<BF>(rw[u][h]);
            r[u][2 * h + 1] = widen_hi<BF>(rw[u][h]);
            b[u][2 * h] = widen_lo<BF>(dw[u][h]) - r[u][2 * h];  // columns past len: 0 - 0
            b[u][2 * h + 1] = widen_hi<BF>(dw[u][h]) - r[u][2 * h + 1];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kDotBatch; ++j) {
        const int i = cb + w + kWaves * j;
        if (i < K) {  // wave-uniform
          u32x4 x[kRuns];
          load_chunk16<true>(src[i] + start, len, lane, x);
#pragma unroll
          for (int u = 0; u < kRuns; ++u) {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
              dot_norm(widen_lo<BF>(x[u][h]), r[u][2 * h], b[u][2 * h], dot[j], nrm[j]);
              dot_norm(widen_hi<BF>(x[u][h]), r[u][2 * h + 1], b[u][2 * h + 1], dot[j], nrm[j]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kDotBatch; ++j) {
      const int i = cb + w + kWaves * j;
      if (i < K) {
        const double td = wave_sum(dot[j]), tn = wave_sum(nrm[j]);
        if (lane == 0) {
          partial[int64_t(i) * G + g] = td;
          partial[(int64_t(K) + i) * G + g] = tn;
        }
      }
    }
  }
}

// out[i] = sum over g of partial[i][g]: robust.hip's sum_rows_kernel (one block
// per row, thread t sums g = t, t + 256, ... in order, then a fixed LDS tree),
// copied so that robust.hip's object stays what its profiles were taken on
__global__ __launch_bounds__(256) void sum_rows16_kernel(const double* __restrict__ partial, int G,
                                                         double* __restrict__ out) {
  __shared__ double red[256];
  const int i = blockIdx.x, t = threadIdx.x;
  const double* p = partial + int64_t(i) * G;
  double s = 0.0;
  for (int g = t; g < G; g += 256) s += p[g];
  red[t] = s;
  __syncthreads();
#pragma unroll
  for (int m = 128; m > 0; m >>= 1) {
    if (t < m) red[t] += red[t + m];
    __syncthreads();
  }
  if (t == 0) out[i] = red[0];
}

// n_chunks == 0: the 2K results are 0 (a kernel, so the call can be captured into a graph)
__global__ __launch_bounds__(256) void zero_kernel(double* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = 0.0;
}

// ---------------------------------------------------------------------------
// FLTrust's rebuild on 16-bit rows: wsum_diff_kernel's chain (robust.hip) on
// the widened values, the result rounded once.  A row (and ref, and out)
// takes 16-byte accesses when its pointer is 16-byte aligned and the tile lies
// whole inside N, 2-byte accesses otherwise: the row pointers live in device
// memory, so the choice is made per pointer here (wave-uniform).
constexpr int kWdVec = 2;      // runs of eight columns per thread per tile
constexpr int kWdClients = 4;  // clients in flight: 4 x 2 16-byte loads per lane, the fp32 kernel's bytes
constexpr int kWdRun = kBS * 8;
constexpr int kWdTile = FEDAGG_WSUM_DIFF16_TILE;
static_assert(kWdTile == kWdRun * kWdVec, "FEDAGG_WSUM_DIFF16_TILE is the block's columns per tile");
constexpr int kWdMaxBlocks = 1 << 20;  // tiles above that go round the grid

__device__ __forceinline__ u32x4 wd_load(const uint16_t* p, int64_t col, int64_t N, bool vec) {
  if (vec) return ld8<true>(p + col);
  return ld8_elems<true, int64_t>(p, col, N);
}

template <bool BF>
__device__ __forceinline__ void widen8(u32x4 v, float (&f)[8]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    f[2 * h] = widen_lo<BF>(v[h]);
    f[2 * h + 1] = widen_hi<BF>(v[h]);
  }
}

// acc = fl(c * fl(x - r)) (FIRST) or fl(acc + fl(c * fl(x - r))): the build never contracts
template <bool BF, bool FIRST>
__device__ __forceinline__ void wd_chain(u32x4 xv, const float (&r)[8], float c, float (&acc)[8]) {
  float x[8];
  widen8<BF>(xv, x);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = (x[e] - r[e]) * c;
    acc[e] = FIRST ? t : acc[e] + t;
  }
}

template <bool BF>
__global__ __launch_bounds__(kBS) void wsum_diff_16_kernel(const uint16_t* const* __restrict__ src,
                                                           const float* __restrict__ cs, int K,
                                                           const uint16_t* __restrict__ ref, int64_t N,
                                                           uint16_t* __restrict__ out, int64_t tiles) {
  const int t = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kWdTile + 8 * t;
    const bool full = (tile + 1) * kWdTile <= N;  // block-uniform: no per-lane bounds in the tile
    float r[kWdVec][8], acc[kWdVec][8];
    {
      const bool vec = full && aligned16(ref);
#pragma unroll
      for (int u = 0; u < kWdVec; ++u) {
        widen8<BF>(wd_load(ref, base + kWdRun * u, N, vec), r[u]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[u][e] = 0.f;
      }
    }
    if (K > 0) {  // the chain starts AT client 0's term, not at 0 + it (-0 stays -0)
      const uint16_t* p = src[0];
      const bool vec = full && aligned16(p);
      const float c = cs[0];
#pragma unroll
      for (int u = 0; u < kWdVec; ++u) wd_chain<BF, true>(wd_load(p, base + kWdRun * u, N, vec), r[u], c, acc[u]);
    }
    int i = 1;
    for (; i + kWdClients <= K; i += kWdClients) {
      u32x4 x[kWdClients][kWdVec];
#pragma unroll
      for (int j = 0; j < kWdClients; ++j) {
        const uint16_t* p = src[i + j];
        const bool vec = full && aligned16(p);
#pragma unroll
        for (int u = 0; u < kWdVec; ++u) x[j][u] = wd_load(p, base + kWdRun * u, N, vec);
      }
#pragma unroll
      for (int j = 0; j < kWdClients; ++j) {
        const float c = cs[i + j];
#pragma unroll
        for (int u = 0; u < kWdVec; ++u) wd_chain<BF, false>(x[j][u], r[u], c, acc[u]);
      }
    }
    for (; i < K; ++i) {  // the last < kWdClients clients
      const uint16_t* p = src[i];
      const bool vec = full && aligned16(p);
      const float c = cs[i];
#pragma unroll
      for (int u = 0; u < kWdVec; ++u) wd_chain<BF, false>(wd_load(p, base + kWdRun * u, N, vec), r[u], c, acc[u]);
    }
    const bool vec = full && aligned16(out);
#pragma unroll
    for (int u = 0; u < kWdVec; ++u) {
      uint32_t y[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = narrow<BF>(K > 0 ? r[u][e] + acc[u][e] : r[u][e]);
      const int64_t col = base + kWdRun * u;
      if (vec) {
        const u32x4 v = {y[0] | (y[1] << 16), y[2] | (y[3] << 16), y[4] | (y[5] << 16), y[6] | (y[7] << 16)};
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(out + col));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < N) __builtin_nontemporal_store(uint16_t(y[e]), out + col + e);
      }
    }
  }
}

bool dtype16(int32_t dtype) { return dtype == FEDAGG_DT_BF16 || dtype == FEDAGG_DT_F16; }

}  // namespace

extern "C" {

int fedagg_dotnorm2_16(int32_t dtype, const void* const* d_src, int32_t K, const void* d_ref, const void* d_dir,
                       const int64_t* d_chunks, int64_t n_chunks, double* d_out, double* d_work, int64_t work_len,
                       fedagg_stream_t stream) {
  if (!dtype16(dtype))
    return set_error(FEDAGG_EINVAL, "fedagg_dotnorm2_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
  if (K < 1 || n_chunks < 0) return set_error(FEDAGG_EINVAL, "fedagg_dotnorm2_16: K must be >= 1 and n_chunks >= 0");
  if (!d_src || !d_ref || !d_dir || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_dotnorm2_16: null pointer");
  if (n_chunks > 0 && work_len < int64_t(2) * K)
    return set_error(FEDAGG_EINVAL, "fedagg_dotnorm2_16: workspace smaller than 2K doubles");
  auto st = reinterpret_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    hipLaunchKernelGGL(zero_kernel, dim3(unsigned(2 * K + 255) / 256), dim3(256), 0, st, d_out, 2 * K);
    return check_launch("fedagg_dotnorm2_16");
  }
  // fedagg_dotnorm2_f32's chunk groups: 1,024 blocks, fewer for a short table or a small workspace
  int64_t G = n_chunks < 1024 ? n_chunks : 1024;
  if (G > work_len / (int64_t(2) * K)) G = work_len / (int64_t(2) * K);
  auto src = reinterpret_cast<const uint16_t* const*>(d_src);
  auto ref = static_cast<const uint16_t*>(d_ref), dir = static_cast<const uint16_t*>(d_dir);
  if (dtype == FEDAGG_DT_BF16)
    hipLaunchKernelGGL(dotnorm2_16_kernel<true>, dim3(unsigned(G)), dim3(kBS), 0, st, src, K, ref, dir, d_chunks,
                       n_chunks, int(G), d_work);
  else
    hipLaunchKernelGGL(dotnorm2_16_kernel<false>, dim3(unsigned(G)), dim3(kBS), 0, st, src, K, ref, dir, d_chunks,
                       n_chunks, int(G), d_work);
  hipLaunchKernelGGL(sum_rows16_kernel, dim3(2u * unsigned(K)), dim3(256), 0, st, d_work, int(G), d_out);
  return check_launch("fedagg_dotnorm2_16");
}

int fedagg_wsum_diff_16(int32_t dtype, const void* const* d_src, const float* d_c, int32_t K, const void* d_ref,
                        int64_t N, void* d_out, fedagg_stream_t stream) {
  if (!dtype16(dtype))
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_diff_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
  if (K < 0 || N < 0) return set_error(FEDAGG_EINVAL, "fedagg_wsum_diff_16: K must be >= 0 and N >= 0");
  if (!d_ref || !d_out || (K > 0 && (!d_src || !d_c)))
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_diff_16: null pointer");
  if (N == 0) return FEDAGG_OK;
  const int64_t tiles = (N + kWdTile - 1) / kWdTile;
  const unsigned blocks = unsigned(tiles < kWdMaxBlocks ? tiles : kWdMaxBlocks);
  auto st = reinterpret_cast<hipStream_t>(stream);
  auto src = reinterpret_cast<const uint16_t* const*>(d_src);
  auto ref = static_cast<const uint16_t*>(d_ref);
  auto out = static_cast<uint16_t*>(d_out);
  if (dtype == FEDAGG_DT_BF16)
    hipLaunchKernelGGL(wsum_diff_16_kernel<true>, dim3(blocks), dim3(kBS), 0, st, src, d_c, K, ref, N, out, tiles);
  else
    hipLaunchKernelGGL(wsum_diff_16_kernel<false>, dim3(blocks), dim3(kBS), 0, st, src, d_c, K, ref, N, out, tiles);
  return check_launch("fedagg_wsum_diff_16");
}

}  // extern "C"
