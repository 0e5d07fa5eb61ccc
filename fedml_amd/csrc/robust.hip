// robust.hip — gfx950 kernels for FedML's distance-based robust aggregation
// (the Krum / multi-Krum and norm-difference-clipping defenses), exported
// through include/fedagg.h and linked into libfedagg.so beside fedagg.hip.
//
// What this replaces (python/fedml/core/security/):
//   defense/krum_defense.py:47-60          K(K-1) torch norms of client differences
//   defense/norm_diff_clipping_defense.py:20-54   one norm per client + the clipped rebuild
//   defense/cclip_defense.py:30-80         bucket distances to the guess + the scaled differences
//   common/utils.py:8-13, 24-27            vectorize_weight / compute_euclidean_distance
//
// Rows are K device pointers (client updates laid out as bucket rows); the
// columns that count ("weight" keys, common/utils.py:16-21) arrive as a chunk
// table of (start, length) pairs built on the host from the key segments.
//
//   fedagg_dist2_f32     out[i] = sum_e (x_i[e] - r[e])^2        (HBM-bound, one pass)
//   fedagg_pairdist2_f32 out[i][j] = sum_e (x_i[e] - x_j[e])^2   (VALU-bound, packed fp32)
//   fedagg_clip_diff_f32 y_i[e] = fl(fl(fl(x_i[e] - r[e]) / c_i) + r[e])
//   fedagg_scale_diff_f32 y_i[e] = fl(fl(x_i[e] - r[e]) * s_i)   (CClip)
//   fedagg_dotnorm2_f32  out[i] = sum_e (x_i[e] - r[e]) (d[e] - r[e]), out[K + i] = sum_e (x_i[e] - r[e])^2
//   fedagg_wsum_diff_f32 y[e] = fl(r[e] + chain_i fl(c_i * fl(x_i[e] - r[e])))   (both: FLTrust, ours)
//
// Every difference is the fp32 difference the reference forms
// (vec_local - vec_global, v1 - v2).  dist2 squares it exactly in fp64 and sums
// in fp64: the exact sum up to fp64 rounding.  pairdist2 squares and sums in
// packed fp32 over a stage of at most 64 columns (relative error ~sqrt(64)
// ulp typical, 64 ulp at worst) and adds the stage sums in fp64: about the
// accuracy of the reference's own fp32 torch.norm (~1e-7 relative).
// Partial sums go to a workspace and are combined in a fixed order: results
// are deterministic run to run.

#include <hip/hip_runtime.h>

#include <type_traits>
#include <stdint.h>

#include <string>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "pairdist.h"

extern "C" int64_t fedagg_wsum_dist2_work_len_internal(int32_t K, int64_t n_chunks);
extern "C" int64_t fedagg_histgram_work_len_internal(int32_t K, int64_t n_chunks);
extern "C" int64_t fedagg_wsum_dist2_wide_work_len_internal(int32_t K, int64_t n_chunks);

namespace {

constexpr int kWaves = kBS / 64;
constexpr int kLaneCols = FEDAGG_DIST_CHUNK / 64;  // columns per lane per chunk (kLaneCols / 4 f32x4)
// clients per wave per pass of dist2_kernel (kWaves * kBatch per block).  32
// would cover 128 clients in one pass but costs the occupancy: 2.61 vs 1.99 ms
// at config 3 (tools/robust_variants.py, profiles/r03/dist/); with the
// reference row cached in L2 (ld4<false>) the second pass's re-read is cheap
constexpr int kBatch = 16;  // dist2: clients per batch (16 vs 32: profiles/r03/dist/)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Columns lane*4 + 256*u (u < kLaneCols/4) of a chunk of `len` columns at
// `p`: 16-byte loads where a whole f32x4 lies in the chunk and p is 16-byte
// aligned (bucket rows and key offsets are), 4-byte loads otherwise; columns
// past len read 0.
template <bool NT = true>
__device__ __forceinline__ void load_chunk(const float* p, int len, int lane, f32x4 (&v)[kLaneCols / 4]) {
  const bool al = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  if (al && len == FEDAGG_DIST_CHUNK) {  // wave-uniform: a full aligned chunk, no per-lane conditions
#pragma unroll
    for (int u = 0; u < kLaneCols / 4; ++u) v[u] = ld4<NT>(p + lane * 4 + 256 * u);
    return;
  }
#pragma unroll
  for (int u = 0; u < kLaneCols / 4; ++u) {
    const int c = lane * 4 + 256 * u;
    if (al && c + 4 <= len) {
      v[u] = ld4<NT>(p + c);
    } else {
      v[u].x = c < len ? gptr(p)[c] : 0.f;
      v[u].y = c + 1 < len ? gptr(p)[c + 1] : 0.f;
      v[u].z = c + 2 < len ? gptr(p)[c + 2] : 0.f;
      v[u].w = c + 3 < len ? gptr(p)[c + 3] : 0.f;
    }
  }
}

__device__ __forceinline__ double sq_diff(float x, float r, double acc) {
  const float d = x - r;  // the reference's fp32 difference
  return __builtin_fma(double(d), double(d), acc);  // exact square, fp64 sum
}

// ---------------------------------------------------------------------------
// Per-client squared distance to a reference row.  A block owns the chunks
// g, g + G, ... (a column range) for every client: per chunk each lane holds
// its reference columns in registers, and wave w streams clients
// w, w + 4, ... (kBatch of them per pass, one fp64 accumulator each) against
// them.  The reference row is read from HBM once per pass, not once per
// client (a client-major grid re-read it ~57x: 1.43x the algorithmic bytes).
__global__ __launch_bounds__(kBS) void dist2_kernel(const float* const* __restrict__ src, int K,
                                                    const float* __restrict__ ref, const int64_t* __restrict__ chunks,
                                                    int64_t n_chunks, int G, double* __restrict__ partial) {
  const int g = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int cb = 0; cb < K; cb += kWaves * kBatch) {
    double acc[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) acc[j] = 0.0;
    for (int64_t c = g; c < n_chunks; c += G) {
      const int64_t start = chunks[2 * c];
      const int len = int(chunks[2 * c + 1]);
      f32x4 r[kLaneCols / 4];
      if (ref) {
        load_chunk<false>(ref + start, len, lane, r);
      } else {
#pragma unroll
        for (int u = 0; u < kLaneCols / 4; ++u) r[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int i = cb + w + kWaves * j;
        if (i < K) {  // wave-uniform
          f32x4 x[kLaneCols / 4];
          load_chunk<true>(src[i] + start, len, lane, x);
#pragma unroll
          for (int u = 0; u < kLaneCols / 4; ++u) {
            acc[j] = sq_diff(x[u].x, r[u].x, acc[j]);
            acc[j] = sq_diff(x[u].y, r[u].y, acc[j]);
            acc[j] = sq_diff(x[u].z, r[u].z, acc[j]);
            acc[j] = sq_diff(x[u].w, r[u].w, acc[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int i = cb + w + kWaves * j;
      if (i < K) {
        const double t = wave_sum(acc[j]);
        if (lane == 0) partial[int64_t(i) * G + g] = t;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// FLTrust's cosines: per client the dot product of a_i = x_i - ref with
// b = dir - ref and |a_i|^2, in ONE pass over the rows.  dist2_kernel's shape:
// a block owns the chunks g, g + G, ... for every client, each lane holds its
// ref columns AND its b columns (the fp32 difference, formed once per chunk)
// in registers, and wave w streams clients w, w + 4, ... against them with two
// fp64 accumulators per client.  Both products of fp32 values are exact in
// fp64, so each sum is the exact sum up to fp64 rounding, as dist2's.
// Partials are laid out [2K][G] (dots, then squared norms): sum_rows_kernel
// finishes them with 2K blocks.
//
// Clients per wave per pass: twice dist2's accumulators plus b sit in
// registers, so the batch is dist2's question again (kBatch's note) with more
// at stake.  FEDAGG_DOTNORM_BATCH builds the other size for
// tools/fltrust_probe.py; the measured pair is in NOTES.md §7c.
#ifndef FEDAGG_DOTNORM_BATCH
#define FEDAGG_DOTNORM_BATCH 8
#endif
constexpr int kDotBatch = FEDAGG_DOTNORM_BATCH;
// 8 clients fit 4 waves per SIMD when the compiler is held to it (119 VGPRs,
// no spill; 135 and 3 waves when it is not), which is what the grid of 1,024
// blocks needs to be resident at once; 16 clients need 159 and spill under
// that cap, so they run at 3
constexpr int kDotWavesPerSimd = kDotBatch <= 8 ? 4 : 3;

__device__ __forceinline__ void dot_norm(float x, float r, float b, double& dot, double& nrm) {
  const double a = double(x - r);  // the fp32 difference, widened
  dot = __builtin_fma(a, double(b), dot);  // exact products, fp64 sums
  nrm = __builtin_fma(a, a, nrm);
}

__global__ __launch_bounds__(kBS, kDotWavesPerSimd) void dotnorm2_kernel(
    const float* const* __restrict__ src, int K, const float* __restrict__ ref, const float* __restrict__ dir,
    const int64_t* __restrict__ chunks, int64_t n_chunks, int G, double* __restrict__ partial) {
  const int g = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int cb = 0; cb < K; cb += kWaves * kDotBatch) {
    double dot[kDotBatch], nrm[kDotBatch];
#pragma unroll
    for (int j = 0; j < kDotBatch; ++j) dot[j] = nrm[j] = 0.0;
    for (int64_t c = g; c < n_chunks; c += G) {
      const int64_t start = chunks[2 * c];
      const int len = int(chunks[2 * c + 1]);
      f32x4 r[kLaneCols / 4], b[kLaneCols / 4];
      load_chunk<false>(ref + start, len, lane, r);
      load_chunk<false>(dir + start, len, lane, b);
#pragma unroll
      for (int u = 0; u < kLaneCols / 4; ++u) b[u] = b[u] - r[u];  // columns past len: 0 - 0
#pragma unroll
      for (int j = 0; j < kDotBatch; ++j) {
        const int i = cb + w + kWaves * j;
        if (i < K) {  // wave-uniform
          f32x4 x[kLaneCols / 4];
          load_chunk<true>(src[i] + start, len, lane, x);
#pragma unroll
          for (int u = 0; u < kLaneCols / 4; ++u) {
            dot_norm(x[u].x, r[u].x, b[u].x, dot[j], nrm[j]);
            dot_norm(x[u].y, r[u].y, b[u].y, dot[j], nrm[j]);
            dot_norm(x[u].z, r[u].z, b[u].z, dot[j], nrm[j]);
            dot_norm(x[u].w, r[u].w, b[u].w, dot[j], nrm[j]);
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

// out[i] = sum over g of partial[i][g]: one block per row, thread t sums
// g = t, t + 256, ... in order, then a fixed LDS tree (deterministic).  The
// first version, one thread per row summing all G in sequence, was a chain of
// G dependent loads: 0.218 ms per call at config 3 (G = 1,024), a tenth of
// the whole dist2 call.
__global__ __launch_bounds__(256) void sum_rows_kernel(const double* __restrict__ partial, int G,
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

// K = 113..128 (8 groups): the 36 tiles as 2 x 2 group blocks, so one read
// of a group's fragments feeds two tiles.  Wave s (s < 4) takes a full block
// (4 tiles: rows {A0, A1} x columns {B0, B1}); wave s + 4, on the same SIMD,
// a diagonal block (3 tiles) and half of a full block (2 tiles, one column):
// 9 tiles per SIMD, 27 fragment reads per SIMD and k-step where the row-run
// schedule needs 36.
constexpr int kBlk8[8][2][5] = {
    // {A0, A1, B0, B1, diag} x 2 blocks (A0 < 0: none)
    {{0, 1, 2, 3, 0}, {-1, -1, -1, -1, 0}}, {{0, 1, 4, 5, 0}, {-1, -1, -1, -1, 0}},
    {{0, 1, 6, 7, 0}, {-1, -1, -1, -1, 0}}, {{2, 3, 4, 5, 0}, {-1, -1, -1, -1, 0}},
    {{0, 1, 0, 1, 1}, {2, 3, 6, -1, 0}},    {{2, 3, 2, 3, 1}, {2, 3, 7, -1, 0}},
    {{4, 5, 4, 5, 1}, {4, 5, 6, -1, 0}},    {{6, 7, 6, 7, 1}, {4, 5, 7, -1, 0}}};
// the (row, column) group of each accumulator slot, in gblock's order
__constant__ constexpr int kBlk8Tile[8][5][2] = {
    {{0, 2}, {0, 3}, {1, 2}, {1, 3}, {-1, -1}}, {{0, 4}, {0, 5}, {1, 4}, {1, 5}, {-1, -1}},
    {{0, 6}, {0, 7}, {1, 6}, {1, 7}, {-1, -1}}, {{2, 4}, {2, 5}, {3, 4}, {3, 5}, {-1, -1}},
    {{0, 0}, {0, 1}, {1, 1}, {2, 6}, {3, 6}},   {{2, 2}, {2, 3}, {3, 3}, {2, 7}, {3, 7}},
    {{4, 4}, {4, 5}, {5, 5}, {4, 6}, {5, 6}},   {{6, 6}, {6, 7}, {7, 7}, {4, 7}, {5, 7}}};

// one block's tiles for k-step ks: (A0,B0), (A0,B1), (A1,B0) unless diagonal,
// (A1,B1), into acc[S0 ..]; a diagonal block reads its rows once (B = A)
template <int PLANE, int A0, int A1, int B0, int B1, bool DIAG, int S0, int TPW>
__device__ __forceinline__ void gblock(const unsigned char* fp, int ks, f32x4v (&acc)[TPW]) {
  bf16x8v FA0[3], FA1[3], FB0[3], FB1[3];
  split_frag<PLANE>(fp, A0, ks, FA0);
  split_frag<PLANE>(fp, A1, ks, FA1);
  if constexpr (!DIAG) {
    split_frag<PLANE>(fp, B0, ks, FB0);
    if constexpr (B1 >= 0) split_frag<PLANE>(fp, B1, ks, FB1);
  }
  const bf16x8v(&b0)[3] = DIAG ? FA0 : FB0;
  const bf16x8v(&b1)[3] = DIAG ? FA1 : FB1;
  constexpr int s1 = S0 + 1, s2 = S0 + (B1 >= 0 ? 2 : 1), s3 = s2 + (DIAG ? 0 : 1);
  acc[S0] = split_mfma6(FA0, b0, acc[S0]);
  if constexpr (B1 >= 0) acc[s1] = split_mfma6(FA0, b1, acc[s1]);
  if constexpr (!DIAG) acc[s2] = split_mfma6(FA1, b0, acc[s2]);
  if constexpr (B1 >= 0) acc[s3] = split_mfma6(FA1, b1, acc[s3]);
}

template <int PLANE, int W, int TPW>
__device__ __forceinline__ void gblocks8(const unsigned char* fp, f32x4v (&acc)[TPW]) {
  constexpr int d0 = kBlk8[W][0][4], d1 = kBlk8[W][1][4];
  constexpr int n0 = d0 ? 3 : (kBlk8[W][0][3] >= 0 ? 4 : 2);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    gblock<PLANE, kBlk8[W][0][0], kBlk8[W][0][1], kBlk8[W][0][2], kBlk8[W][0][3], d0 != 0, 0, TPW>(fp, ks, acc);
    if constexpr (kBlk8[W][1][0] >= 0)
      gblock<PLANE, kBlk8[W][1][0], kBlk8[W][1][1], kBlk8[W][1][2], kBlk8[W][1][3], d1 != 0, n0, TPW>(fp, ks, acc);
  }
}

// pairgram16_kernel (robust16.hip) is this kernel for bf16 / f16 rows, copied
// step for step (tile runs, fetch, stage_sums, fold, prologue, iter): a fix to
// the pipeline or the tile schedule here belongs there too.
template <int NB>
__global__ __launch_bounds__(kSplit8BS, 1) void pairgram_split8_kernel(const float* const* __restrict__ src, int K,
                                                                     const int64_t* __restrict__ chunks,
                                                                     int64_t n_chunks, int G,
                                                                     double* __restrict__ partial) {
  constexpr int ROWS = NB * 16;
  constexpr int NT = NB * (NB + 1) / 2;
  constexpr int TPW = (NB + 2) / 2;  // ceil((NB + 1) / 2) tiles per wave, at most
  constexpr int RPW = ROWS / 8;      // staged rows per wave
  constexpr int LPW = (RPW + 3) / 4; // 16-byte loads per lane and stage (4 rows per wave-load)
  constexpr int PLANE = ROWS * kSplitRB;
  __shared__ __attribute__((aligned(16))) unsigned char sP[2][3 * PLANE];
  __shared__ float sSum[2][8][kStage];
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i16 = lane & 15, q = lane >> 4;
  const float* rowp[LPW];
  bool rlive[LPW];
#pragma unroll
  for (int u = 0; u < LPW; ++u) {
    const int lr = 4 * u + q;  // row within the wave's RPW (NB = 1, 2: RPW < 4, lanes past it idle)
    const int cl = wave * RPW + lr;
    rlive[u] = lr < RPW && cl < K;
    rowp[u] = src[rlive[u] ? cl : 0];
  }
  // the row pair of this wave and its share of the pair's tiles
  const int p = wave & 3;
  const int pr1 = p, pr2 = NB - 1 - p;
  const int len1 = p < (NB + 1) / 2 ? NB - p : 0;  // row pr1's tiles (b = pr1 .. NB - 1)
  const int len2 = len1 && pr2 > pr1 ? p + 1 : 0;  // row pr2's tiles (b = pr2 .. NB - 1)
  const int half = (len1 + len2 + 1) / 2;
  const int first = wave < 4 ? 0 : half;                    // this wave's tiles: pair tiles first .. first + nmine - 1
  const int nmine = wave < 4 ? half : len1 + len2 - half;
  // as (row, first column group, count) runs: at most two
  const int r1 = first < len1 ? pr1 : pr2;
  const int b1 = first < len1 ? pr1 + first : pr2 + (first - len1);
  const int n1 = first < len1 ? (len1 - first < nmine ? len1 - first : nmine) : nmine;
  const int r2 = pr2, b2 = pr2 + (first + n1 - len1 > 0 ? first + n1 - len1 : 0);
  const int n2 = nmine - n1;
  double acc64[TPW][4];
  f32x4v acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    acc[j] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc64[j][r] = 0.0;
  }
  const float invK = 1.0f / float(K);
  int64_t c = g;
  int s0 = 0;
  f32x4 v[2][LPW];
  auto fetch = [&](f32x4 (&vv)[LPW]) __attribute__((always_inline)) {
    if (c >= n_chunks) return false;
    const int len = int(chunks[2 * c + 1]);
    const int64_t col0 = chunks[2 * c] + s0;
    const int w = len - s0 < kStage ? len - s0 : kStage;
    const int c4 = 4 * i16;
    if (w == kStage) {
#pragma unroll
      for (int u = 0; u < LPW; ++u) vv[u] = ld4<true>(rowp[u] + col0 + c4);
    } else {
#pragma unroll
      for (int u = 0; u < LPW; ++u) {
        const float* pp = rowp[u] + col0;
        const bool ok = rlive[u];
        vv[u].x = ok && c4 < w ? gptr(pp)[c4] : 0.f;
        vv[u].y = ok && c4 + 1 < w ? gptr(pp)[c4 + 1] : 0.f;
        vv[u].z = ok && c4 + 2 < w ? gptr(pp)[c4 + 2] : 0.f;
        vv[u].w = ok && c4 + 3 < w ? gptr(pp)[c4 + 3] : 0.f;
      }
    }
    s0 += kStage;
    if (s0 >= len) {
      s0 = 0;
      c += G;
    }
    return true;
  };
  auto masked = [&](const f32x4& x, int u) __attribute__((always_inline)) {
    const uint32_t m = rlive[u] ? 0xffffffffu : 0u;
    return f32x4{__uint_as_float(__float_as_uint(x.x) & m), __uint_as_float(__float_as_uint(x.y) & m),
                 __uint_as_float(__float_as_uint(x.z) & m), __uint_as_float(__float_as_uint(x.w) & m)};
  };
  auto stage_sums = [&](const f32x4 (&vv)[LPW], int sb) __attribute__((always_inline)) {
    f32x4 cs = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < LPW; ++u) cs += masked(vv[u], u);
#pragma unroll
    for (int m = 16; m <= 32; m <<= 1) {
      cs.x += __shfl_xor(cs.x, m, 64);
      cs.y += __shfl_xor(cs.y, m, 64);
      cs.z += __shfl_xor(cs.z, m, 64);
      cs.w += __shfl_xor(cs.w, m, 64);
    }
    if (q == 0) *reinterpret_cast<f32x4*>(&sSum[sb][wave][4 * i16]) = cs;
  };
  auto stage_split = [&](const f32x4 (&vv)[LPW], int sb, unsigned char* P) __attribute__((always_inline)) {
    f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      f32x4 s8[8];
#pragma unroll
      for (int w = 0; w < 8; ++w) s8[w] = *reinterpret_cast<const f32x4*>(&sSum[sb][w][4 * i16]);
      r = (((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]))) * invK;
    }
#pragma unroll
    for (int u = 0; u < LPW; ++u) {
      if (4 * u + q < RPW) {
        const f32x4 cc = masked(vv[u], u) - r;
        const uint32_t h01 = pk_bf16(cc.x, cc.y), h23 = pk_bf16(cc.z, cc.w);
        const float e0 = cc.x - bf16_lo(h01), e1 = cc.y - bf16_hi(h01);
        const float e2 = cc.z - bf16_lo(h23), e3 = cc.w - bf16_hi(h23);
        const uint32_t m01 = pk_bf16(e0, e1), m23 = pk_bf16(e2, e3);
        const uint32_t l01 = pk_bf16(e0 - bf16_lo(m01), e1 - bf16_hi(m01));
        const uint32_t l23 = pk_bf16(e2 - bf16_lo(m23), e3 - bf16_hi(m23));
        unsigned char* d = P + (wave * RPW + 4 * u + q) * kSplitRB + 8 * i16;
        *reinterpret_cast<u32x2v*>(d) = u32x2v{h01, h23};
        *reinterpret_cast<u32x2v*>(d + PLANE) = u32x2v{m01, m23};
        *reinterpret_cast<u32x2v*>(d + 2 * PLANE) = u32x2v{l01, l23};
      }
    }
  };
  int unfolded = 0;
  auto fold = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      // 16 wait states between the last MFMA writing acc[j] and this VALU
      // read: the compiler once left only 3 where the fold follows the MFMA
      // chain directly (NB = 1: wrong sums on the box); tools/mfma_hazards.py
      // checks every shipped build
      asm volatile("s_nop 15" : "+v"(acc[j]));
      acc64[j][0] += double(acc[j].x);
      acc64[j][1] += double(acc[j].y);
      acc64[j][2] += double(acc[j].z);
      acc64[j][3] += double(acc[j].w);
      acc[j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    }
    unfolded = 0;
  };
  const int fo = i16 * kSplitRB + 16 * q;
  auto compute = [&](const unsigned char* P) __attribute__((always_inline)) {
    if constexpr (NB == 8) {
      const unsigned char* fp = P + fo;
      switch (wave) {
        case 0: gblocks8<PLANE, 0>(fp, acc); break;
        case 1: gblocks8<PLANE, 1>(fp, acc); break;
        case 2: gblocks8<PLANE, 2>(fp, acc); break;
        case 3: gblocks8<PLANE, 3>(fp, acc); break;
        case 4: gblocks8<PLANE, 4>(fp, acc); break;
        case 5: gblocks8<PLANE, 5>(fp, acc); break;
        case 6: gblocks8<PLANE, 6>(fp, acc); break;
        default: gblocks8<PLANE, 7>(fp, acc); break;
      }
      if (++unfolded == kSplitFold) fold();
      return;
    }
    if (nmine > 0) {
      const unsigned char* fp = P + fo;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8v A1[3], A2[3], B[2][3];
        split_frag<PLANE>(fp, r1, ks, A1);
        split_frag<PLANE>(fp, b1, ks, B[0]);
        if (n2) split_frag<PLANE>(fp, r2, ks, A2);
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if (j < nmine) {
            if (j + 1 < nmine)
              split_frag<PLANE>(fp, j + 1 < n1 ? b1 + j + 1 : b2 + (j + 1 - n1), ks, B[(j + 1) & 1]);
            acc[j] = j < n1 ? split_mfma6(A1, B[j & 1], acc[j]) : split_mfma6(A2, B[j & 1], acc[j]);
          }
        }
      }
    }
    if (++unfolded == kSplitFold) fold();
  };
  // prologue: stages 0 and 1 loaded, stage 0 split, stage 1's sums published
  bool h0 = fetch(v[0]);
  bool h1 = h0 && fetch(v[1]);
  if (h0) {
    stage_sums(v[0], 0);
    lds_barrier();
    stage_split(v[0], 0, sP[0]);
    bool h2 = h1 && fetch(v[0]);  // stage 2
    if (h1) stage_sums(v[1], 1);
    lds_barrier();
    // iteration k (two at a time, so the register sets are static)
    auto iter = [&](auto cur_tag, bool& hn, bool& hnn) __attribute__((always_inline)) {
      constexpr int C = decltype(cur_tag)::value;  // k % 2
      // hn: stage k + 1 exists (in v[C ^ 1], sums in sSum[C ^ 1]); hnn: stage k + 2 (in v[C])
      bool hnnn = false;
      if (hn) {
        stage_split(v[C ^ 1], C ^ 1, sP[C ^ 1]);
        hnnn = hnn && fetch(v[C ^ 1]);  // stage k + 3
      }
      compute(sP[C]);
      if (hnn) stage_sums(v[C], C);
      lds_barrier();
      const bool more = hn;
      hn = hnn;
      hnn = hnnn;
      return more;
    };
    bool hn = h1, hnn = h2;
    while (true) {
      if (!iter(std::integral_constant<int, 0>{}, hn, hnn)) break;
      if (!iter(std::integral_constant<int, 1>{}, hn, hnn)) break;
    }
  }
  if (unfolded) fold();
  const int nout = NB == 8 ? (wave < 4 ? 4 : 5) : nmine;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (j < nout) {
      int a = j < n1 ? r1 : r2, b = j < n1 ? b1 + j : b2 + (j - n1);
      if constexpr (NB == 8) {
        a = kBlk8Tile[wave][j][0];
        b = kBlk8Tile[wave][j][1];
      }
      const int tt = a * NB - a * (a - 1) / 2 + (b - a);
      double* out = partial + (int64_t(g) * NT + tt) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(4 * q + r) * 16 + i16] = acc64[j][r];
    }
  }
}

// ---------------------------------------------------------------------------
// The split Gram for up to 1024 clients (fedagg_pairgram2_wide_f32):
// pairdist_kernel's decomposition with pairgram_split8_kernel's inner loop.
// The K x K pair matrix is cut into 64-client tiles (I <= J); a block owns one
// tile pair over the chunk groups g, g + G, ...  No block sees all K rows, so
// the centre r of c = fl(x - r) is an argument: one fp32 row indexed like the
// client rows (the caller passes the client mean; D is translation invariant,
// r only decides conditioning).
//
// Per 64-column stage the 8 waves stage I's 64 rows and J's 64 rows (16 rows
// a wave, four 16-byte loads per lane), subtract the centre and split once per
// element into the three bf16 planes: 128 plane rows of kSplitRB bytes, the
// NB = 8 budget of pairgram_split8_kernel, double-buffered, one barrier per
// stage, raw rows prefetched two stages ahead.  An off-diagonal pair has the
// 4 x 4 = 16 cross group-tiles: wave w takes A group w / 2 against the two B
// groups 2 (w % 2), + 1, so its A fragments are read once for two tiles.  A
// diagonal pair stages 64 rows (waves 0 - 3) and has the 10 tiles of the group
// triangle (kWideDiag: 3, 3, 2, 2 per SIMD).  Rows are read with plain loads,
// not non-temporal ones: each 64-row panel is read by every block whose pair
// holds its tile, and the grid runs tile pairs fastest, chunk groups slowest,
// so blocks resident together read the same columns.  At K = 1024 the L2
// absorbs about a third of the 17-fold re-read (FETCH_SIZE 11.8x the rows);
// an XCD-grouped block order did not change the time (NOTES.md 5c).
// Partials: [g][tile pair][16 group-tiles a * 4 + b][16 x 16]; a diagonal pair
// writes the slots a <= b only and gram_wide_sum_kernel reads no other.
// (kWideBS, kWidePlane, kWideDiag, gram_wide_sum_kernel and wide_group_blocks
// are in pairdist.h: pairgram_wide16.hip's kernel for 16-bit rows shares them.)
__global__ __launch_bounds__(kWideBS, 1) void pairgram_wide_kernel(const float* const* __restrict__ src, int K,
                                                                   const float* __restrict__ center,
                                                                   const int64_t* __restrict__ chunks,
                                                                   int64_t n_chunks, int G,
                                                                   double* __restrict__ partial) {
  constexpr int LPW = 4;  // 16-byte loads per lane and stage: 16 rows a wave, 4 rows per wave-load
  __shared__ __attribute__((aligned(16))) unsigned char sP[2][3 * kWidePlane];
  const int tp = blockIdx.x, g = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i16 = lane & 15, q = lane >> 4;
  const int2 tile = tile_of(tp, (K + kPT - 1) / kPT);
  const bool diag = tile.x == tile.y;
  const bool stager = !diag || wave < 4;  // a diagonal pair has 64 rows to stage
  const float* rowp[LPW];
  bool rlive[LPW];
#pragma unroll
  for (int u = 0; u < LPW; ++u) {
    const int lr = wave * 16 + 4 * u + q;  // plane row
    const int cl = lr < kPT ? tile.x * kPT + lr : tile.y * kPT + (lr - kPT);
    rlive[u] = stager && cl < K;
    rowp[u] = src[rlive[u] ? cl : 0];  // a row past K reads row 0: its Gram entries are never summed
  }
  // this wave's tiles: A group ga against B groups gb, gb + 1 (nt of them)
  const int ga = diag ? kWideDiag[wave][0] : wave >> 1;
  const int gb = diag ? kWideDiag[wave][1] : 4 + 2 * (wave & 1);
  const int nt = diag ? kWideDiag[wave][2] : 2;
  double acc64[2][4];
  f32x4v acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    acc[j] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc64[j][r] = 0.0;
  }
  int64_t c = g;
  int s0 = 0;
  f32x4 v[2][LPW], cen[2];
  auto fetch = [&](f32x4 (&vv)[LPW], f32x4& rr) __attribute__((always_inline)) {
    if (c >= n_chunks) return false;
    const int len = int(chunks[2 * c + 1]);
    const int64_t col0 = chunks[2 * c] + s0;
    const int w = len - s0 < kStage ? len - s0 : kStage;
    const int c4 = 4 * i16;
    if (stager) {
      if (w == kStage) {
#pragma unroll
        for (int u = 0; u < LPW; ++u) vv[u] = ld4<false>(rowp[u] + col0 + c4);
        rr = ld4<false>(center + col0 + c4);
      } else {  // columns past w read 0 in the rows and in the centre: c = 0
#pragma unroll
        for (int u = 0; u < LPW; ++u) {
          const float* pp = rowp[u] + col0;
          const bool ok = rlive[u];
          vv[u].x = ok && c4 < w ? gptr(pp)[c4] : 0.f;
          vv[u].y = ok && c4 + 1 < w ? gptr(pp)[c4 + 1] : 0.f;
          vv[u].z = ok && c4 + 2 < w ? gptr(pp)[c4 + 2] : 0.f;
          vv[u].w = ok && c4 + 3 < w ? gptr(pp)[c4 + 3] : 0.f;
        }
        const float* pc = center + col0;
        rr.x = c4 < w ? gptr(pc)[c4] : 0.f;
        rr.y = c4 + 1 < w ? gptr(pc)[c4 + 1] : 0.f;
        rr.z = c4 + 2 < w ? gptr(pc)[c4 + 2] : 0.f;
        rr.w = c4 + 3 < w ? gptr(pc)[c4 + 3] : 0.f;
      }
    }
    s0 += kStage;
    if (s0 >= len) {
      s0 = 0;
      c += G;
    }
    return true;
  };
  auto stage_split = [&](const f32x4 (&vv)[LPW], const f32x4& rr, unsigned char* P) __attribute__((always_inline)) {
    if (!stager) return;
#pragma unroll
    for (int u = 0; u < LPW; ++u)
      split3_store(vv[u] - rr, P + (wave * 16 + 4 * u + q) * kSplitRB + 8 * i16, kWidePlane);
  };
  int unfolded = 0;
  auto fold = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      // the 16 wait states between the MFMA chain and this VALU read, as in
      // pairgram_split8_kernel (tools/mfma_hazards.py checks every build)
      asm volatile("s_nop 15" : "+v"(acc[j]));
      acc64[j][0] += double(acc[j].x);
      acc64[j][1] += double(acc[j].y);
      acc64[j][2] += double(acc[j].z);
      acc64[j][3] += double(acc[j].w);
      acc[j] = f32x4v{0.f, 0.f, 0.f, 0.f};
    }
    unfolded = 0;
  };
  const int fo = i16 * kSplitRB + 16 * q;
  auto compute = [&](const unsigned char* P) __attribute__((always_inline)) {
    if (nt > 0) {
      const unsigned char* fp = P + fo;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8v A[3], B[2][3];
        split_frag<kWidePlane>(fp, ga, ks, A);
        split_frag<kWidePlane>(fp, gb, ks, B[0]);
        split_frag<kWidePlane>(fp, nt > 1 ? gb + 1 : gb, ks, B[1]);
        acc[0] = split_mfma6(A, B[0], acc[0]);
        if (nt > 1) acc[1] = split_mfma6(A, B[1], acc[1]);
      }
    }
    if (++unfolded == kSplitFold) fold();
  };
  // prologue: stages 0 and 1 loaded, stage 0 split
  bool h0 = fetch(v[0], cen[0]);
  bool h1 = h0 && fetch(v[1], cen[1]);
  if (h0) {
    stage_split(v[0], cen[0], sP[0]);
    bool h2 = h1 && fetch(v[0], cen[0]);  // stage 2
    lds_barrier();
    // iteration k (two at a time, so the register sets are static): split
    // stage k + 1 into the free plane buffer, issue stage k + 3's loads into
    // the freed registers, compute stage k, barrier
    auto iter = [&](auto cur_tag, bool& hn, bool& hnn) __attribute__((always_inline)) {
      constexpr int C = decltype(cur_tag)::value;  // k % 2
      // hn: stage k + 1 exists (in v[C ^ 1]); hnn: stage k + 2 (in v[C])
      bool hnnn = false;
      if (hn) {
        stage_split(v[C ^ 1], cen[C ^ 1], sP[C ^ 1]);
        hnnn = hnn && fetch(v[C ^ 1], cen[C ^ 1]);  // stage k + 3
      }
      compute(sP[C]);
      lds_barrier();
      const bool more = hn;
      hn = hnn;
      hnn = hnnn;
      return more;
    };
    bool hn = h1, hnn = h2;
    while (true) {
      if (!iter(std::integral_constant<int, 0>{}, hn, hnn)) break;
      if (!iter(std::integral_constant<int, 1>{}, hn, hnn)) break;
    }
  }
  if (unfolded) fold();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < nt) {
      const int slot = ga * 4 + (gb + j - (diag ? 0 : 4));
      double* out = partial + ((int64_t(g) * gridDim.x + tp) * 16 + slot) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(4 * q + r) * 16 + i16] = acc64[j][r];
    }
  }
}

// ---------------------------------------------------------------------------
// Clipped rebuild (norm_diff_clipping_defense.py:38-54): y = (x - r) / c + r
// in fp32 with the reference's three roundings (c = fl32 of the clip divisor;
// torch divides an fp32 tensor by a Python scalar in fp32).  Same shape as
// dist2: a block owns column tiles g, g + G, ... of FEDAGG_DIST_CHUNK columns,
// the reference tile sits in registers, wave w rebuilds clients w, w + 4, ...
// An unclipped client (c == 1) skips the division: x / 1 == x exactly.
// CClip's scaled difference (cclip_defense.py:47-52), MUL = true:
// y = fl32(fl32(x - r) * s), s = fl32 of the Python score.
template <bool MUL>
__device__ __forceinline__ f32x4 clip4(f32x4 x, f32x4 r, float c, bool one) {
  f32x4 d = f32x4{x.x - r.x, x.y - r.y, x.z - r.z, x.w - r.w};
  if constexpr (MUL) return f32x4{d.x * c, d.y * c, d.z * c, d.w * c};
  if (!one) d = f32x4{d.x / c, d.y / c, d.z / c, d.w / c};
  return f32x4{d.x + r.x, d.y + r.y, d.z + r.z, d.w + r.w};
}

// one client's rebuilt chunk -> its destination row
template <bool MUL>
__device__ __forceinline__ void clip_store(float* y, const f32x4 (&x)[kLaneCols / 4], const f32x4 (&r)[kLaneCols / 4],
                                           float c, int len, int lane) {
  const bool one = c == 1.0f;
  const bool al = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
#pragma unroll
  for (int u = 0; u < kLaneCols / 4; ++u) {
    const int col = lane * 4 + 256 * u;
    const f32x4 v = clip4<MUL>(x[u], r[u], c, one);
    if (al && col + 4 <= len) {
      __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(y + col));
    } else {
      if (col < len) y[col] = v.x;
      if (col + 1 < len) y[col + 1] = v.y;
      if (col + 2 < len) y[col + 2] = v.z;
      if (col + 3 < len) y[col + 3] = v.w;
    }
  }
}

// CU clients per wave and step: all their loads are issued before the first
// store, so a lane keeps CU * kLaneCols / 4 16-byte loads in flight (one
// client at a time kept only 4, and stalled on every load before storing)
template <bool MUL, int CU>
__global__ __launch_bounds__(kBS) void clip_diff_kernel(const float* const* __restrict__ src, int K,
                                                        const float* __restrict__ ref, const float* __restrict__ div,
                                                        int64_t N, float* const* __restrict__ dst, int G) {
  const int g = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t tiles = (N + FEDAGG_DIST_CHUNK - 1) / FEDAGG_DIST_CHUNK;
  for (int64_t t = g; t < tiles; t += G) {
    const int64_t start = t * FEDAGG_DIST_CHUNK;
    const int len = int(N - start < FEDAGG_DIST_CHUNK ? N - start : FEDAGG_DIST_CHUNK);
    f32x4 r[kLaneCols / 4];
    load_chunk<false>(ref + start, len, lane, r);
    int i = w;
    for (; i + kWaves * (CU - 1) < K; i += kWaves * CU) {
      f32x4 x[CU][kLaneCols / 4];
#pragma unroll
      for (int j = 0; j < CU; ++j) load_chunk(src[i + kWaves * j] + start, len, lane, x[j]);
#pragma unroll
      for (int j = 0; j < CU; ++j)
        clip_store<MUL>(dst[i + kWaves * j] + start, x[j], r, div[i + kWaves * j], len, lane);
    }
    for (; i < K; i += kWaves) {  // the last < CU clients of this wave
      f32x4 x[kLaneCols / 4];
      load_chunk(src[i] + start, len, lane, x);
      clip_store<MUL>(dst[i] + start, x, r, div[i], len, lane);
    }
  }
}

constexpr int kClipClients = 2;  // clients in flight per wave in clip_diff_kernel

// ---------------------------------------------------------------------------
// FLTrust's rebuild: out = ref + sum_i c_i (x_i - ref) as the fp32 chain
//   acc = fl(c_0 * fl(x_0 - ref)); acc = fl(acc + fl(c_i * fl(x_i - ref))); out = fl(ref + acc)
// (K == 0: out = ref).  A streaming kernel: every byte is read once, so all
// loads are non-temporal.  A block owns tiles of FEDAGG_WSUM_DIFF_TILE columns,
// a thread kWdVec f32x4 columns of each (1,024 columns apart: a wave's load is
// 1 KB contiguous); it loads ref once, then walks the clients kWdClients at a
// time, all their loads issued before the first use (kWdClients * kWdVec
// 16-byte loads in flight per lane).  c_i is wave-uniform.  A row (and ref,
// and out) takes 16-byte accesses when its pointer is 16-byte aligned and the
// tile lies whole inside N, 4-byte accesses otherwise: the row pointers live
// in device memory, so the choice is made per pointer here (wave-uniform), not
// on the host.
constexpr int kWdVec = 2;
constexpr int kWdClients = 4;
constexpr int kWdTile = FEDAGG_WSUM_DIFF_TILE;
static_assert(kWdTile == kBS * 4 * kWdVec, "FEDAGG_WSUM_DIFF_TILE is the block's columns per tile");

// the thread's f32x4 at column `col` of a row of N columns; columns past N read 0
__device__ __forceinline__ f32x4 wd_load(const float* p, int64_t col, int64_t N, bool vec) {
  if (vec) return ld4<true>(p + col);
  f32x4 v;
  v.x = col < N ? __builtin_nontemporal_load(gptr(p) + col) : 0.f;
  v.y = col + 1 < N ? __builtin_nontemporal_load(gptr(p) + col + 1) : 0.f;
  v.z = col + 2 < N ? __builtin_nontemporal_load(gptr(p) + col + 2) : 0.f;
  v.w = col + 3 < N ? __builtin_nontemporal_load(gptr(p) + col + 3) : 0.f;
  return v;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// fl(c * fl(x - r)): two roundings (the build never contracts)
__device__ __forceinline__ f32x4 wd_term(f32x4 x, f32x4 r, float c) {
  const f32x4 d = x - r;
  return f32x4{d.x * c, d.y * c, d.z * c, d.w * c};
}

__global__ __launch_bounds__(kBS) void wsum_diff_kernel(const float* const* __restrict__ src,
                                                        const float* __restrict__ cs, int K,
                                                        const float* __restrict__ ref, int64_t N,
                                                        float* __restrict__ out, int64_t tiles) {
  const int t = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kWdTile + 4 * t;
    const bool full = (tile + 1) * kWdTile <= N;  // block-uniform: no per-lane bounds in the tile
    f32x4 r[kWdVec], acc[kWdVec] = {};
    {
      const bool vec = full && aligned16(ref);
#pragma unroll
      for (int u = 0; u < kWdVec; ++u) r[u] = wd_load(ref, base + 1024 * u, N, vec);
    }
    if (K > 0) {  // the chain starts AT client 0's term, not at 0 + it (-0 stays -0)
      const float* p = src[0];
      const bool vec = full && aligned16(p);
#pragma unroll
      for (int u = 0; u < kWdVec; ++u) acc[u] = wd_term(wd_load(p, base + 1024 * u, N, vec), r[u], cs[0]);
    }
    int i = 1;
    for (; i + kWdClients <= K; i += kWdClients) {
      f32x4 x[kWdClients][kWdVec];
#pragma unroll
      for (int j = 0; j < kWdClients; ++j) {
        const float* p = src[i + j];
        const bool vec = full && aligned16(p);
#pragma unroll
        for (int u = 0; u < kWdVec; ++u) x[j][u] = wd_load(p, base + 1024 * u, N, vec);
      }
#pragma unroll
      for (int j = 0; j < kWdClients; ++j) {
        const float c = cs[i + j];
#pragma unroll
        for (int u = 0; u < kWdVec; ++u) acc[u] = acc[u] + wd_term(x[j][u], r[u], c);
      }
    }
    for (; i < K; ++i) {  // the last < kWdClients clients
      const float* p = src[i];
      const bool vec = full && aligned16(p);
      const float c = cs[i];
#pragma unroll
      for (int u = 0; u < kWdVec; ++u) acc[u] = acc[u] + wd_term(wd_load(p, base + 1024 * u, N, vec), r[u], c);
    }
    const bool vec = full && aligned16(out);
#pragma unroll
    for (int u = 0; u < kWdVec; ++u) {
      const f32x4 y = K > 0 ? r[u] + acc[u] : r[u];
      const int64_t col = base + 1024 * u;
      if (vec) {
        __builtin_nontemporal_store(y, reinterpret_cast<f32x4*>(out + col));
      } else {
        if (col < N) out[col] = y.x;
        if (col + 1 < N) out[col + 1] = y.y;
        if (col + 2 < N) out[col + 2] = y.z;
        if (col + 3 < N) out[col + 3] = y.w;
      }
    }
  }
}

constexpr int kWdMaxBlocks = 1 << 20;  // tiles above that (N > 2^31 columns) go round the grid

template <bool MUL>
int launch_diff(const char* what, const float* const* d_src, int32_t K, const float* d_ref, const float* d_c, int64_t N,
                float* const* d_dst, fedagg_stream_t stream) {
  if (K < 1 || N < 0) return set_error(FEDAGG_EINVAL, std::string(what) + ": K must be >= 1 and N >= 0");
  if (!d_src || !d_ref || !d_c || !d_dst) return set_error(FEDAGG_EINVAL, std::string(what) + ": null pointer");
  if (N == 0) return FEDAGG_OK;
  const int G = grid_groups(2, (N + FEDAGG_DIST_CHUNK - 1) / FEDAGG_DIST_CHUNK, 0, 0);
  hipLaunchKernelGGL((clip_diff_kernel<MUL, kClipClients>), dim3(unsigned(G)), dim3(kBS), 0,
                     static_cast<hipStream_t>(stream), d_src, K, d_ref, d_c, N, d_dst, G);
  return check_launch(what);
}

}  // namespace

extern "C" {

int64_t fedagg_robust_work_len(int32_t kind, int32_t K, int64_t n_chunks) {
  if (K < 1 || n_chunks < 0) return -1;
  if (n_chunks == 0) return 0;
  // dist2: 1,024 blocks, the kernel's residency (4 waves per SIMD): every
  // block streams its column ranges from start to end with no second round
  // of blocks (2,048: 2.31 ms at config 3, 1,024: 2.22 ms)
  if (kind == FEDAGG_WORK_DIST2) return int64_t(K) * grid_groups(4, n_chunks, 0, 0);
  if (kind == FEDAGG_WORK_PAIRGRAM) {
    if (K > kGramMax) return -1;
    // the groups the split kernel runs, not the 512 a two-blocks-per-CU grid would
    int G = grid_groups(4096 / (256 * kGramBlocksPerCU), n_chunks, 0, 0);
    if (G > kGramMaxGroups) G = kGramMaxGroups;
    return int64_t(G) * gram_tiles(K) * 256 + int64_t(K) * K;
  }
  if (kind == FEDAGG_WORK_PAIRDIST2) {
    if (K <= kTriMax) return int64_t(16) * tri_blocks(K) * grid_groups(4, n_chunks, 0, 0);
    const int NT = pair_tiles(K);
    return int64_t(NT) * grid_groups(NT, n_chunks, 0, 0) * (kPT * kPT);
  }
  if (kind == FEDAGG_WORK_PAIRGRAM_WIDE) {
    if (K > kWideMax) return -1;
    const int NT = pair_tiles(K);
    return int64_t(NT) * grid_groups(wide_group_blocks(NT), n_chunks, 0, 0) * (kPT * kPT) + int64_t(K) * K;
  }
  if (kind == FEDAGG_WORK_WSUM_DIST2) return fedagg_wsum_dist2_work_len_internal(K, n_chunks);  // geomed.hip
  if (kind == FEDAGG_WORK_WSUM_DIST2_WIDE) return fedagg_wsum_dist2_wide_work_len_internal(K, n_chunks);  // geomed_wide.hip
  if (kind == FEDAGG_WORK_DOTNORM2) return int64_t(2) * K * grid_groups(4, n_chunks, 0, 0);  // dist2's grid, two rows a client
  if (kind == FEDAGG_WORK_HISTGRAM) return fedagg_histgram_work_len_internal(K, n_chunks);  // histgram.hip
  return -1;
}

int fedagg_dotnorm2_f32(const float* const* d_src, int32_t K, const float* d_ref, const float* d_dir,
                        const int64_t* d_chunks, int64_t n_chunks, double* d_out, double* d_work, int64_t work_len,
                        fedagg_stream_t stream) {
  if (K < 1 || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_dotnorm2_f32: K must be >= 1 and n_chunks >= 0");
  if (!d_src || !d_ref || !d_dir || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_dotnorm2_f32: null pointer");
  if (n_chunks > 0 && work_len < int64_t(2) * K)
    return set_error(FEDAGG_EINVAL, "fedagg_dotnorm2_f32: workspace smaller than 2K doubles");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * 2 * K, st) != hipSuccess) return check_launch("fedagg_dotnorm2_f32");
    return FEDAGG_OK;
  }
  const int G = grid_groups(4, n_chunks, work_len, int64_t(2) * K);
  hipLaunchKernelGGL(dotnorm2_kernel, dim3(unsigned(G)), dim3(kBS), 0, st, d_src, K, d_ref, d_dir, d_chunks, n_chunks,
                     G, d_work);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(2u * unsigned(K)), dim3(256), 0, st, d_work, G, d_out);
  return check_launch("fedagg_dotnorm2_f32");
}

int fedagg_wsum_diff_f32(const float* const* d_src, const float* d_c, int32_t K, const float* d_ref, int64_t N,
                         float* d_out, fedagg_stream_t stream) {
  if (K < 0 || N < 0) return set_error(FEDAGG_EINVAL, "fedagg_wsum_diff_f32: K must be >= 0 and N >= 0");
  if (!d_ref || !d_out || (K > 0 && (!d_src || !d_c)))
    return set_error(FEDAGG_EINVAL, "fedagg_wsum_diff_f32: null pointer");
  if (N == 0) return FEDAGG_OK;
  const int64_t tiles = (N + kWdTile - 1) / kWdTile;
  const unsigned blocks = unsigned(tiles < kWdMaxBlocks ? tiles : kWdMaxBlocks);
  hipLaunchKernelGGL(wsum_diff_kernel, dim3(blocks), dim3(kBS), 0, static_cast<hipStream_t>(stream), d_src, d_c, K,
                     d_ref, N, d_out, tiles);
  return check_launch("fedagg_wsum_diff_f32");
}

int fedagg_dist2_f32(const float* const* d_src, int32_t K, const float* d_ref, const int64_t* d_chunks,
                     int64_t n_chunks, double* d_out, double* d_work, int64_t work_len, fedagg_stream_t stream) {
  if (K < 1 || n_chunks < 0) return set_error(FEDAGG_EINVAL, "fedagg_dist2_f32: K must be >= 1 and n_chunks >= 0");
  if (!d_src || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_dist2_f32: null pointer");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * K, st) != hipSuccess) return check_launch("fedagg_dist2_f32");
    return FEDAGG_OK;
  }
  if (work_len < K) return set_error(FEDAGG_EINVAL, "fedagg_dist2_f32: workspace smaller than K doubles");
  const int G = grid_groups(4, n_chunks, work_len, K);
  hipLaunchKernelGGL(dist2_kernel, dim3(unsigned(G)), dim3(kBS), 0, st, d_src, K, d_ref, d_chunks, n_chunks, G,
                     d_work);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(unsigned(K)), dim3(256), 0, st, d_work, G, d_out);
  return check_launch("fedagg_dist2_f32");
}

int fedagg_pairdist2_f32(const float* const* d_src, int32_t K, const int64_t* d_chunks, int64_t n_chunks,
                         double* d_out, double* d_work, int64_t work_len, fedagg_stream_t stream) {
  return launch_pairdist<float>("fedagg_pairdist2_f32", d_src, K, d_chunks, n_chunks, d_out, d_work, work_len, stream);
}

int fedagg_pairgram2_f32(const float* const* d_src, int32_t K, const int64_t* d_chunks, int64_t n_chunks,
                         double* d_out, double* d_work, int64_t work_len, fedagg_stream_t stream) {
  if (K < 1 || K > kGramMax || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_f32: K must be in [1, 128] and n_chunks >= 0");
  if (!d_src || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_f32: null pointer");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * K * K, st) != hipSuccess) return check_launch("fedagg_pairgram2_f32");
    return FEDAGG_OK;
  }
  const int64_t per = int64_t(gram_tiles(K)) * 256;
  const int64_t mat = int64_t(K) * K;
  if (work_len < per + mat)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_f32: workspace too small (fedagg_robust_work_len)");
  int G = grid_groups(4096 / (256 * kGramBlocksPerCU), n_chunks, work_len - mat, per);
  if (G > kGramMaxGroups) G = kGramMaxGroups;  // one block per CU
  double* M = d_work + int64_t(G) * per;
  {
    auto kern = pairgram_split8_kernel<8>;
    switch (gram_groups(K)) {
      case 1: kern = pairgram_split8_kernel<1>; break;
      case 2: kern = pairgram_split8_kernel<2>; break;
      case 3: kern = pairgram_split8_kernel<3>; break;
      case 4: kern = pairgram_split8_kernel<4>; break;
      case 5: kern = pairgram_split8_kernel<5>; break;
      case 6: kern = pairgram_split8_kernel<6>; break;
      case 7: kern = pairgram_split8_kernel<7>; break;
      default: break;
    }
    hipLaunchKernelGGL(kern, dim3(unsigned(G)), dim3(kSplit8BS), 0, st, d_src, K, d_chunks, n_chunks, G, d_work);
  }
  hipLaunchKernelGGL(gram_sum_kernel, dim3(unsigned((per + 63) / 64)), dim3(256), 0, st, d_work, G, K, M);
  hipLaunchKernelGGL(gram_dist_kernel, dim3(unsigned((mat + 255) / 256)), dim3(256), 0, st, M, K, d_out);
  return check_launch("fedagg_pairgram2_f32");
}

int fedagg_pairgram2_wide_f32(const float* const* d_src, int32_t K, const float* d_center, const int64_t* d_chunks,
                              int64_t n_chunks, double* d_out, double* d_work, int64_t work_len,
                              fedagg_stream_t stream) {
  if (K < 1 || K > kWideMax || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_wide_f32: K must be in [1, 1024] and n_chunks >= 0");
  if (!d_src || !d_center || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_wide_f32: null pointer");
  const int NT = pair_tiles(K);
  const int64_t per = int64_t(NT) * kPT * kPT;
  const int64_t mat = int64_t(K) * K;
  if (n_chunks > 0 && work_len < per + mat)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_wide_f32: workspace too small (fedagg_robust_work_len)");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * K * K, st) != hipSuccess)
      return check_launch("fedagg_pairgram2_wide_f32");
    return FEDAGG_OK;
  }
  const int G = grid_groups(wide_group_blocks(NT), n_chunks, work_len - mat, per);
  double* M = d_work + int64_t(G) * per;
  hipLaunchKernelGGL(pairgram_wide_kernel, dim3(unsigned(NT), unsigned(G)), dim3(kWideBS), 0, st, d_src, K, d_center,
                     d_chunks, n_chunks, G, d_work);
  hipLaunchKernelGGL(gram_wide_sum_kernel, dim3(unsigned(per / 64)), dim3(256), 0, st, d_work, G, K, M);
  hipLaunchKernelGGL(gram_dist_kernel, dim3(unsigned((mat + 255) / 256)), dim3(256), 0, st, M, K, d_out);
  return check_launch("fedagg_pairgram2_wide_f32");
}

int fedagg_clip_diff_f32(const float* const* d_src, int32_t K, const float* d_ref, const float* d_div, int64_t N,
                         float* const* d_dst, fedagg_stream_t stream) {
  return launch_diff<false>("fedagg_clip_diff_f32", d_src, K, d_ref, d_div, N, d_dst, stream);
}

int fedagg_scale_diff_f32(const float* const* d_src, int32_t K, const float* d_ref, const float* d_scale, int64_t N,
                          float* const* d_dst, fedagg_stream_t stream) {
  return launch_diff<true>("fedagg_scale_diff_f32", d_src, K, d_ref, d_scale, N, d_dst, stream);
}

}  // extern "C"
