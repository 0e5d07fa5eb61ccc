// pairdist.h — the pair-distance pieces that robust.hip (fp32 rows) and
// robust16.hip (bf16 / f16 rows) share: the exact-difference kernels,
// templated on the row element type, the split Gram's fragment reads, MFMA
// chains and tile schedules, templated on the number of bf16 planes, and the
// finish kernels.  Everything here is internal to the including unit.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/fedagg.h"
#include "host_util.h"

namespace {

template <class T>
__device__ __forceinline__ const T __attribute__((address_space(1)))* gptr(const T* p) {
  return (const T __attribute__((address_space(1)))*)(p);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kBS = 256;

// A 16-byte load of four fp32 columns (any 4-byte alignment), non-temporal or plain.
// NT = false for a row every wave of the block reads (the reference row):
// a plain load leaves it in L2 for the other three waves; non-temporal loads
// made each wave fetch it from HBM again (dist2's traffic was 1.05x the
// algorithmic bytes, ~7 extra reference rows per call at config 3)
template <bool NT = true>
__device__ __forceinline__ f32x4 ld4(const float* p) {
  const auto q = reinterpret_cast<const f32x4 __attribute__((address_space(1)))*>(gptr(p));
  if constexpr (NT) return __builtin_nontemporal_load(q);
  return *q;
}

// Row element types.  A 16-bit row is read as raw 16-bit words and widened to
// fp32 exactly in registers: bf16 by a shift, f16 by v_cvt_f32_f16 (denormals
// kept).  Everything after the load works on fp32 values, whatever the rows are.
struct bf16_t { uint16_t bits; };
struct f16_t { uint16_t bits; };
__device__ __forceinline__ float widen_bf16(uint32_t b) { return __uint_as_float(b << 16); }
__device__ __forceinline__ float widen_f16(uint32_t b) { return float(__builtin_bit_cast(_Float16, uint16_t(b))); }

// element i of row p, non-temporal, as fp32
template <class T>
__device__ __forceinline__ float ld_elem(const T* p, int64_t i) {
  if constexpr (std::is_same_v<T, float>) {
    return __builtin_nontemporal_load(gptr(p) + i);
  } else {
    const uint32_t b = __builtin_nontemporal_load(gptr(reinterpret_cast<const uint16_t*>(p)) + i);
    if constexpr (std::is_same_v<T, bf16_t>) return widen_bf16(b);
    return widen_f16(b);
  }
}

// A workgroup barrier that waits for this wave's LDS operations only.
// __syncthreads() carries a release fence that waits for EVERY outstanding
// memory operation (s_waitcnt vmcnt(0) lgkmcnt(0) before s_barrier), so the
// next stage's global loads, issued just before it, were drained at every
// barrier instead of overlapping the stage's compute.  The "memory" clobber
// keeps the compiler from moving LDS accesses across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------
// Pairwise squared distances.  The K x K pair matrix is cut into 64 x 64
// client tiles (I <= J); a block owns one tile over the chunk group g.  Per
// stage of 64 columns each wave loads 16 client rows of tile I (and of J) as
// coalesced 256-B row segments into registers one stage ahead, then writes
// them four rows at a time as one 16-byte LDS write per lane: sX[column][client], rows padded by one group so
// both the staging writes and the compute reads are bank-conflict free.  Thread (ti, tj) then owns clients 4ti..4ti+3 of I x 4tj..4tj+3 of J:
// per column one 16-byte LDS read per side and 16 squared differences, as 8
// packed fp32 subtracts and 8 packed fp32 FMAs (v_pk_add_f32 / v_pk_fma_f32) in
// robust.hip's build; robust16.hip is built without packed fp32 operations
// (build.py, UNIT_FLAGS) and gets 16 v_sub_f32 and 16 v_fmac_f32 from the same
// source: the same IEEE operations and values at twice the VALU issue.
// fp32 sums over one stage (<= 64 columns) are flushed into fp64
// accumulators, which go to the workspace per block.
constexpr int kPT = 64;      // clients per tile side
constexpr int kStage = 64;   // columns per LDS stage

// [column][client] tile rows padded by one 4-client group (272 B): a staging
// write (lane = column, 16 B) walks the banks 16 B apart, and a compute read's
// address is the thread's group base plus a constant per unrolled column (an
// immediate offset; the earlier XOR swizzle cost two VALU ops per column)
constexpr int kRowF = kPT + 4;
__device__ __forceinline__ int swz(int c, int grp) { return c * kRowF + (grp << 2); }

// The 16 client rows (4 groups of 4) a wave stages for one 64-client side:
// wave-uniform pointers, read once per block (kept in SGPRs); a row past K
// points at row 0 and is zeroed by `live`.
template <class T>
struct SideRows {
  const T* p[4][4];
  bool live[4][4];
};

template <class T>
__device__ __forceinline__ SideRows<T> side_rows(const T* const* __restrict__ src, int K, int base, int wave) {
  SideRows<T> r;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cl = base + (wave * 4 + q) * 4 + k;
      r.live[q][k] = cl < K;
      r.p[q][k] = src[cl < K ? cl : 0];
    }
  return r;
}

// A stage's global loads for one side, into registers (lane = column):
// unconditional loads at a clamped column, then zeroed past w / past K, so
// all 16 are in flight together.  Issued one stage ahead, they overlap the
// current stage's compute.
template <class T>
__device__ __forceinline__ void stage_load(f32x4 (&v)[4], const SideRows<T>& rows, int64_t col0, int w, int lane) {
  const int c = lane < w ? lane : 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[q][k] = ld_elem(rows.p[q][k], col0 + c);
}

// the staged values, zeroed past column w and past K: a mask applied here,
// when the stage is written to LDS, not right after the loads, so nothing
// consumes them early and they stay in flight through the current stage's
// compute (a select on the uniform `live` had become a branch around each
// load with a full vmcnt(0) wait at every join)
template <class T>
__device__ __forceinline__ void stage_store(f32x4* __restrict__ s, const f32x4 (&v)[4], const SideRows<T>& rows,
                                            int w, int t) {
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t m = (rows.live[q][k] && lane < w) ? 0xffffffffu : 0u;
      x[k] = __uint_as_float(__float_as_uint(v[q][k]) & m);
    }
    s[swz(lane, wave * 4 + q) >> 2] = x;
  }
}

// one column of the thread's 4 x 4 pair block: acc[2k + h] holds pairs
// (4ti + k, 4tj + 2h) and (4ti + k, 4tj + 2h + 1); a = the column's values of
// clients 4ti.., b = of clients 4tj..
__device__ __forceinline__ void pair_ab(f32x4 a, f32x4 b, f32x2 (&acc)[8]) {
  const f32x2 b01 = {b[0], b[1]}, b23 = {b[2], b[3]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f32x2 ak = {a[k], a[k]};
    const f32x2 d0 = ak - b01, d1 = ak - b23;  // robust.hip: v_pk_add_f32 (neg, op_sel broadcast)
    acc[2 * k] = __builtin_elementwise_fma(d0, d0, acc[2 * k]);  // robust.hip: v_pk_fma_f32
    acc[2 * k + 1] = __builtin_elementwise_fma(d1, d1, acc[2 * k + 1]);
  }
}

// The columns [0, w) of a stage; pa / pb point at column 0 of the thread's
// two 4-client groups, RS = row stride in f32x4.  A full stage reads column
// c + 1 before column c computes (the last prefetch reads a pad row past the
// stage), so a wave does not wait a whole LDS round trip in front of every
// column: SQ_WAIT_ANY was 52 % of the triangle kernel's wave cycles.
template <int RS>
__device__ __forceinline__ void pair_stage(const f32x4* pa, const f32x4* pb, int w, f32x2 (&acc)[8]) {
  if (w == kStage) {
    f32x4 an = pa[0], bn = pb[0];
#pragma unroll 8
    for (int col = 0; col < kStage; ++col) {
      const f32x4 a = an, b = bn;
      an = pa[(col + 1) * RS];
      bn = pb[(col + 1) * RS];
      __builtin_amdgcn_sched_barrier(0);  // keep the scheduler from sinking the prefetch to its use
      pair_ab(a, b, acc);
    }
  } else {
    for (int col = 0; col < w; ++col) pair_ab(pa[col * RS], pb[col * RS], acc);
  }
}

// tile pair tp -> (a, b), a <= b, row-major over the upper triangle of T x T
__device__ __forceinline__ int2 tile_of(int tp, int T) {
  int a = 0;
  while (tp >= T - a) {
    tp -= T - a;
    ++a;
  }
  return int2{a, a + tp};
}

template <class T>
__global__ __launch_bounds__(kBS) void pairdist_kernel(const T* const* __restrict__ src, int K,
                                                       const int64_t* __restrict__ chunks, int64_t n_chunks, int G,
                                                       double* __restrict__ partial) {
  __shared__ f32x4 sA[(kStage + 1) * kRowF / 4];  // + the pad row pair_stage's last prefetch reads
  __shared__ f32x4 sB[(kStage + 1) * kRowF / 4];
  const int tp = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
  const int2 tile = tile_of(tp, (K + kPT - 1) / kPT);
  const int I = tile.x * kPT, J = tile.y * kPT;
  const bool diag = tile.x == tile.y;
  const f32x4* sJ = diag ? sA : sB;
  const int ti = t >> 4, tj = t & 15;
  double acc64[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc64[k] = 0.0;
  // the stages of chunks g, g + G, ... in order; (c, s0) is the next stage
  int64_t c = g;
  int s0 = 0;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const SideRows<T> rowsA = side_rows(src, K, I, wave);
  const SideRows<T> rowsB = side_rows(src, K, diag ? I : J, wave);
  f32x4 va[4], vb[4];
  int64_t col_next = 0;
  int w_next = 0;
  auto fetch = [&]() {  // issue the next stage's loads; false past the last stage
    if (c >= n_chunks) return false;
    const int len = int(chunks[2 * c + 1]);
    col_next = chunks[2 * c] + s0;
    w_next = len - s0 < kStage ? len - s0 : kStage;
    stage_load(va, rowsA, col_next, w_next, lane);
    if (!diag) stage_load(vb, rowsB, col_next, w_next, lane);
    s0 += kStage;
    if (s0 >= len) {
      s0 = 0;
      c += G;
    }
    return true;
  };
  bool have = fetch();
  while (have) {
    const int w = w_next;
    lds_barrier();  // the previous stage's LDS reads are done
    stage_store(sA, va, rowsA, w, t);
    if (!diag) stage_store(sB, vb, rowsB, w, t);
    have = fetch();  // next stage's loads in flight during this stage's compute
    lds_barrier();
    f32x2 acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = f32x2{0.f, 0.f};
    pair_stage<kRowF / 4>(sA + (swz(0, ti) >> 2), sJ + (swz(0, tj) >> 2), w, acc);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      acc64[2 * k] += double(acc[k][0]);
      acc64[2 * k + 1] += double(acc[k][1]);
    }
  }
  // pair (4ti + k, 4tj + m) of the tile at acc64[4k + m]
  double* out = partial + (int64_t(tp) * G + g) * (kPT * kPT);
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int m = 0; m < 4; ++m) out[(4 * ti + k) * kPT + 4 * tj + m] = acc64[4 * k + m];
}

// D[a][b] and D[b][a] from the tiles' partials.  A block owns 64 pairs of a
// tile (one coalesced 512-B row of the partials per chunk group); its four
// waves sum the chunk groups g = q, q + 4, ... (8 loads in flight per lane),
// and the four quarter sums are added in a fixed order: deterministic.  (One
// thread per pair summing all G in sequence kept 16 blocks per tile busy:
// 0.33 ms at config 3.)
__global__ __launch_bounds__(256) void pair_finish_kernel(const double* __restrict__ partial, int G, int K,
                                                          double* __restrict__ D) {
  __shared__ double quarter[4][64];
  const int tp = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;  // pair index in the tile
  const double* p = partial + int64_t(tp) * G * (kPT * kPT) + e;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int g = q;
  for (; g + 28 < G; g += 32) {
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += p[int64_t(g + 4 * u) * (kPT * kPT)];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)  // the last < 8 of this quarter's groups
    if (g + 4 * u < G) s[u] += p[int64_t(g + 4 * u) * (kPT * kPT)];
  quarter[q][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (q != 0) return;
  const double t = (quarter[0][lane] + quarter[1][lane]) + (quarter[2][lane] + quarter[3][lane]);
  const int2 tile = tile_of(tp, (K + kPT - 1) / kPT);
  const int a = tile.x * kPT + e / kPT, b = tile.y * kPT + e % kPT;
  if (a >= K || b >= K) return;
  D[int64_t(a) * K + b] = a == b ? 0.0 : t;
  if (tile.x != tile.y) D[int64_t(b) * K + a] = t;
}

// ---------------------------------------------------------------------------
// Up to 128 clients: the pair triangle in ONE block per chunk group.  The
// tiled kernel above runs a 64 x 64 diagonal tile as a full square (256 4x4
// pair blocks for the 136 of its upper triangle): at K = 128 that is 768
// block-threads for 528 useful blocks, at K = 64 256 for 136.  Here every
// client sits in LDS per stage (128 clients x 64 columns = 33 KB,
// [column][client], rows padded by one 4-client group) and thread t owns
// the t-th 4x4 block (bi <= bj, row-major) of the upper triangle: 576 threads
// (9 waves) at K = 128, 192 at K = 64.  Per column and thread the work is the
// tiled kernel's (two 16-byte LDS reads, 8 packed subtracts, 8 packed FMAs, or 16 + 16 unpacked in robust16.hip,
// fp32 stage sums flushed into fp64).  A diagonal block computes all 16
// slots; its mirrored halves are the same fp32 values.  Partials are laid out
// [g][slot][block] so both their stores and the finish kernel's reads are
// coalesced.
constexpr int kTriMax = 128;   // clients the triangle kernel holds
constexpr int kTriBS = 576;    // 9 waves: 528 blocks at K = 128
constexpr int kTriLoads = 6;   // 4-client groups a wave stages per stage

// rows of NB 4-client groups padded by one group (an odd number of 16-byte
// slots: conflict-free staging writes, as the tiles' rows); the kernel is
// instantiated for NB = 16 (K <= 64) and 32 (K <= 128) so its two stage
// buffers take 35 / 69 KB of LDS
template <int NB>
constexpr int tri_row_f() { return 4 * (NB + 1); }
template <int NB>
__device__ __forceinline__ int tri_swz(int c, int grp) { return c * tri_row_f<NB>() + (grp << 2); }

__host__ __device__ inline int tri_blocks(int K) {
  const int nb = (K + 3) / 4;
  return nb * (nb + 1) / 2;
}
// threads of the triangle kernel: every block owned, every 4-client group staged
inline int tri_threads(int K) {
  const int nb = (K + 3) / 4, nblk = tri_blocks(K);
  int w = (nblk + 63) / 64;
  const int wl = (nb + kTriLoads - 1) / kTriLoads;
  return 64 * (w > wl ? w : wl);
}

// block index -> (bi, bj), row-major over the upper triangle of nb x nb
__device__ __forceinline__ int2 tri_block(int t, int nb) {
  int bi = 0;
  while (t >= nb - bi) {
    t -= nb - bi;
    ++bi;
  }
  return int2{bi, bi + t};
}

template <class T, int NBMAX>
__global__ __launch_bounds__(kTriBS) void pairtri_kernel(const T* const* __restrict__ src, int K,
                                                        const int64_t* __restrict__ chunks, int64_t n_chunks, int G,
                                                        double* __restrict__ partial) {
  // two stage buffers (one barrier per stage), each with the pad row
  // pair_stage's last prefetch reads
  __shared__ f32x4 sX[2][(kStage + 1) * tri_row_f<NBMAX>() / 4];
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), W = blockDim.x >> 6;
  const int nb = (K + 3) >> 2, nblk = nb * (nb + 1) / 2;
  const bool active = t < nblk;
  const int2 blk = tri_block(active ? t : 0, nb);
  // the groups this wave stages: wave, wave + W, ... (wave-uniform pointers
  // in SGPRs; a row past K points at row 0 and is zeroed by the mask)
  const T* rp[kTriLoads][4];
  bool live[kTriLoads][4];
#pragma unroll
  for (int q = 0; q < kTriLoads; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cl = 4 * (wave + W * q) + k;
      live[q][k] = cl < K;
      rp[q][k] = src[cl < K ? cl : 0];
    }
  double acc64[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc64[k] = 0.0;
  int64_t c = g;
  int s0 = 0;
  f32x4 v[kTriLoads];
  int w_next = 0;
  auto fetch = [&]() {  // the next stage's loads; false past the last stage
    if (c >= n_chunks) return false;
    const int len = int(chunks[2 * c + 1]);
    const int64_t col0 = chunks[2 * c] + s0;
    w_next = len - s0 < kStage ? len - s0 : kStage;
    const int cc = lane < w_next ? lane : 0;
#pragma unroll
    for (int q = 0; q < kTriLoads; ++q)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[q][k] = ld_elem(rp[q][k], col0 + cc);
    s0 += kStage;
    if (s0 >= len) {
      s0 = 0;
      c += G;
    }
    return true;
  };
  // the staged registers -> a stage buffer, zeroed past the stage's width w
  // and past K here (not in fetch: the loads stay in flight until now)
  auto stage_to = [&](f32x4* buf, int w) {
#pragma unroll
    for (int q = 0; q < kTriLoads; ++q)
      if (wave + W * q < nb) {
        f32x4 x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t m = (live[q][k] && lane < w) ? 0xffffffffu : 0u;
          x[k] = __uint_as_float(__float_as_uint(v[q][k]) & m);
        }
        buf[tri_swz<NBMAX>(lane, wave + W * q) >> 2] = x;
      }
  };
  // Stage s computes from buffer s & 1 while stage s + 1 is written into the
  // other one and stage s + 2's loads are in flight: one barrier per stage.
  // A buffer is rewritten only after the barrier that ends its readers' stage.
  bool have = fetch();
  if (have) {
    int w = w_next;
    stage_to(sX[0], w);
    have = fetch();
    lds_barrier();
    for (int buf = 0;; buf ^= 1) {
      if (active) {
        f32x2 acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = f32x2{0.f, 0.f};
        pair_stage<tri_row_f<NBMAX>() / 4>(sX[buf] + (tri_swz<NBMAX>(0, blk.x) >> 2),
                                           sX[buf] + (tri_swz<NBMAX>(0, blk.y) >> 2), w, acc);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          acc64[2 * k] += double(acc[k][0]);
          acc64[2 * k + 1] += double(acc[k][1]);
        }
      }
      if (!have) break;
      const int wn = w_next;
      stage_to(sX[buf ^ 1], wn);
      have = fetch();
      lds_barrier();
      w = wn;
    }
  }
  if (active) {
    double* out = partial + int64_t(g) * 16 * nblk + t;
#pragma unroll
    for (int j = 0; j < 16; ++j) out[int64_t(j) * nblk] = acc64[j];  // slot j = 4k + m: pair (4bi + k, 4bj + m)
  }
}

// D from the triangle kernel's partials: entry e = slot * nblk + block, the
// chunk groups summed in four fixed-order quarters as in pair_finish_kernel
__global__ __launch_bounds__(256) void tri_finish_kernel(const double* __restrict__ partial, int G, int K,
                                                         double* __restrict__ D) {
  __shared__ double quarter[4][64];
  const int nb = (K + 3) >> 2, nblk = nb * (nb + 1) / 2, E = 16 * nblk;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int ec = e < E ? e : E - 1;
  const double* p = partial + ec;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int g = q;
  for (; g + 28 < G; g += 32) {
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += p[int64_t(g + 4 * u) * E];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (g + 4 * u < G) s[u] += p[int64_t(g + 4 * u) * E];
  quarter[q][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (q != 0 || e >= E) return;
  const double tsum = (quarter[0][lane] + quarter[1][lane]) + (quarter[2][lane] + quarter[3][lane]);
  const int j = e / nblk;
  const int2 blk = tri_block(e - j * nblk, nb);
  const int a = 4 * blk.x + (j >> 2), b = 4 * blk.y + (j & 3);
  if (a >= K || b >= K) return;
  // a diagonal block holds (a, b) and (b, a) as equal values: both write both
  D[int64_t(a) * K + b] = a == b ? 0.0 : tsum;
  D[int64_t(b) * K + a] = a == b ? 0.0 : tsum;
}

// ---------------------------------------------------------------------------
// Pairwise squared distances as a CENTRED Gram on fp32 MFMA (K <= 128).
//
// D_ij = sum_e (x_i[e] - x_j[e])^2 = sum_e (c_i[e] - c_j[e])^2 with c = x - r
// for ANY per-column r, so D = G_ii + G_jj - 2 G_ij over the Gram G of the
// centred rows: one FMA per client pair and column on the matrix cores
// (v_mfma_f32_16x16x4_f32) instead of the exact-difference kernel's packed
// subtract + packed FMA on the VALU.  Centring is what keeps the Gram form
// accurate: honest clients are close to one another (base + small
// updates), so uncentred |x|^2 would dwarf D and cancel.  Per 64-column stage
// r is the column mean over the K clients, so |c|^2 is of the order of the
// distances themselves.
//
// Layout: a block owns chunk groups g, g + G, ... (like pairtri_kernel); per
// stage its 4 waves stage all NB*16 client rows of 64 columns into LDS
// ([client][column], rows of kGramRS floats; lane = column, so every global
// load is one coalesced 256-B row segment with a wave-uniform base) and
// write per-wave column sums beside them.  After one barrier each wave
// builds, for each of its tiles (a 16 x 16 block of the client-group
// triangle, row-major, a wave owning a contiguous run of them), the A / B
// fragments of the 16x16x4 MFMA: lane (i = l & 15, q = l >> 4) supplies
// client 16a + i (A) / 16b + i (B) at columns 16q + m of MFMA m, centred by
// the stage's column mean, so 16 MFMAs cover the stage.  Stage sums are fp32
// (MFMA accumulation: an fmaf chain over 64 columns) and are added into fp64
// per stage.  Partials go to the workspace [g][tile][16 x 16]; the finish
// kernels sum them over g in a fixed order into the K x K Gram M (fp64) and
// form D = max(0, M_ii + M_jj - 2 M_ij).
//
// Accuracy: each centred value is one fp32 rounding of x - r, each stage's
// Gram entry an fp32 fmaf chain over 64 products (~1e-7 relative to
// sum |c_i c_j|), so |D - D_exact| is ~1e-7 * (|c_i|^2 + |c_j|^2): the same
// order as the reference's own fp32 torch.norm when the clients' spread is
// of the order of their distances (tests/test_gpu_dist_defenses.py checks
// the Krum selections and D against the exact-difference kernel).
constexpr int kGramMax = 128;          // clients the Gram kernel holds (8 groups of 16)
constexpr int kGramBlocksPerCU = 2;    // 2 x (2 stage buffers of 128 rows) = 143 KB of LDS per CU
constexpr int kGramMaxGroups = 256;    // pairgram_split8_kernel: one block per CU, so at most 256 chunk groups

__host__ __device__ inline int gram_groups(int K) { return (K + 15) / 16; }
__host__ __device__ inline int gram_tiles(int K) {
  const int nb = gram_groups(K);
  return nb * (nb + 1) / 2;
}

// tile index -> (a, b), row-major over the upper triangle of nb x nb
__device__ __forceinline__ int2 gram_tile(int t, int nb) {
  int a = 0;
  while (t >= nb - a) {
    t -= nb - a;
    ++a;
  }
  return int2{a, a + t};
}

typedef float f32x4v __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// The centred Gram on the bf16 matrix cores (the shipped kernel; the fp32-MFMA form
// it replaced, 5.3 ms at config 3, is recorded in NOTES.md §5c).
//
// Every centred value is split EXACTLY into three bf16 parts, c = h + m + l
// (h = bf16(c) rounded to nearest, m = bf16(c - h), l = c - h - m: each
// remainder is exact in fp32 and the last one has at most 8 significant bits,
// so it IS a bf16), and
//   c_i c_j = h_i h_j + h_i m_j + m_i h_j + m_i m_j + h_i l_j + l_i h_j + e,
//   |e| <= |m_i l_j| + |l_i m_j| + |l_i l_j| <= 2^-23 |c_i| |c_j|
// (|m| <= 2^-8 |c|, |l| <= 2^-8 |m|; tests/test_gram_split.py), the order of
// the fp32 rounding of each product on the f32 MFMA (2^-24).  bf16 x bf16
// products are exact in fp32 and the MFMA accumulates in fp32, so each Gram
// entry is a sum of exact products at fp32 accumulation, as on the f32 MFMA.
// Six v_mfma_f32_16x16x32_bf16 (16 cycles each) cover 32 columns of a tile
// where the f32 form needs eight 16x16x4 (32 cycles each): 96 against 256
// cycles, so the 3.0 ms matrix floor at config 3 drops to 1.1 ms, under the
// 1.64 ms of reading the rows once.
//
// LDS: the three planes of one stage, [plane][client][64 columns] bf16, rows
// of kSplitRB (160) bytes.  gfx950 serves a ds_read_b128 in the lane
// groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59},
// {36-43,48-51,60-63}, i.e. (rows 0-3, 12-15 at k-block q) with (rows 4-11 at
// q + 1): with 160-byte rows those 16 reads hit 16 distinct 16-byte bank
// groups for both k-steps (tools/lds_layout.py checks it); the 144-byte rows
// of the first version made every group 2-way.  The stores (ds_write_b64,
// 16 contiguous lanes = one 128-byte row) are conflict-free either way.  The
// split is done once per element when a stage is written, never per tile.
// Fragments (16x16x32, lane i = l & 15, q = l >> 4): A[row i][k = 8q + j] and
// B[k = 8q + j][col i] are both 16 bytes of row (16 g + i) at columns
// 32 ks + 8q .. + 7.  A wave's tiles are a contiguous run in row-major order,
// so consecutive tiles share their A group: its fragments are read once per run.
constexpr int kSplitFold = 4;  // stages summed in fp32 by the MFMAs before one fp64 fold
constexpr int kSplitRB = 160;  // bytes per plane row: 64 bf16 + padding

typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));

// two floats -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
[[maybe_unused]] __device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2v{a, b}, bf16x2v));
}
[[maybe_unused]] __device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
[[maybe_unused]] __device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// The split kernel's tile schedule: wave w takes the two rows of tiles w and
// NB - 1 - w of the group triangle (NB - w and w + 1 tiles: NB + 1 in all, the
// same for every wave at even NB; an odd NB's middle row goes alone).  Both
// rows' A fragments are read once per k-step, the B fragments ping-pong by
// tile, so tile j + 1's reads overlap tile j's six MFMAs, and every wave runs
// ONE code path (per-wave compile-time schedules spilled).
// NP: the planes a stage needs (fp32 rows: always 3; 16-bit rows decide per
// stage, robust16.hip).  Only the first NP planes' fragments are read.
template <int PLANE, int NP = 3>
__device__ __forceinline__ void split_frag(const unsigned char* fp, int grp, int ks, bf16x8v (&F)[3]) {
  const unsigned char* p = fp + grp * (16 * kSplitRB) + 64 * ks;
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) F[pl] = __builtin_bit_cast(bf16x8v, *reinterpret_cast<const u32x4v*>(p + pl * PLANE));
}

[[maybe_unused]] __device__ __forceinline__ f32x4v split_mfma6(const bf16x8v (&A)[3], const bf16x8v (&B)[3], f32x4v x) {
  x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[0], x, 0, 0, 0);
  x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[1], x, 0, 0, 0);
  x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[0], x, 0, 0, 0);
  x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[1], x, 0, 0, 0);
  x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[2], x, 0, 0, 0);
  x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[2], B[0], x, 0, 0, 0);
  return x;
}

// The products NP planes need: hh alone when every c of the stage is a bf16
// (m = l = 0), hh, hm, mh, mm when l = 0 (all four exact, so their sum is the
// exact c_i c_j), the six of split_mfma6 otherwise.
template <int NP>
__device__ __forceinline__ f32x4v split_mfma(const bf16x8v (&A)[3], const bf16x8v (&B)[3], f32x4v x) {
  if constexpr (NP == 3) return split_mfma6(A, B, x);
  x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[0], x, 0, 0, 0);
  if constexpr (NP == 2) {
    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[1], x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[0], x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[1], x, 0, 0, 0);
  }
  return x;
}

// c = h + m + l, four columns of one row, into the three planes at d
[[maybe_unused]] __device__ __forceinline__ void split3_store(f32x4 cc, unsigned char* d, int plane) {
  const uint32_t h01 = pk_bf16(cc.x, cc.y), h23 = pk_bf16(cc.z, cc.w);
  const float e0 = cc.x - bf16_lo(h01), e1 = cc.y - bf16_hi(h01);
  const float e2 = cc.z - bf16_lo(h23), e3 = cc.w - bf16_hi(h23);
  const uint32_t m01 = pk_bf16(e0, e1), m23 = pk_bf16(e2, e3);
  const uint32_t l01 = pk_bf16(e0 - bf16_lo(m01), e1 - bf16_hi(m01));
  const uint32_t l23 = pk_bf16(e2 - bf16_lo(m23), e3 - bf16_hi(m23));
  *reinterpret_cast<u32x2v*>(d) = u32x2v{h01, h23};
  *reinterpret_cast<u32x2v*>(d + plane) = u32x2v{m01, m23};
  *reinterpret_cast<u32x2v*>(d + 2 * plane) = u32x2v{l01, l23};
}

// pairgram_split8_kernel: the split Gram with 8 waves per block and ONE
// block per CU, so the planes can be double-buffered (2 x 55 KB) and a stage
// needs one barrier, and each lane's raw rows are prefetched two stages
// ahead (two register sets; 16 rows per wave).  Iteration k: split stage
// k + 1 into the free plane buffer (its column sums were published before
// the last barrier), issue stage k + 3's loads into the freed registers,
// compute stage k, publish stage k + 2's column sums, barrier.  A stage's
// loads have two iterations to land.  Tiles: the row pair p (rows p and
// NB - 1 - p, as the 4-wave kernel) is shared by waves p and p + 4, which sit
// on the same SIMD: wave p takes its first ceil(n / 2) tiles, wave p + 4 the
// rest, so every SIMD runs one pair's MFMAs per stage.
constexpr int kSplit8BS = 512;

// sum over g < G of p[g * stride] for the 256 threads of a finish block
// (lane = element, wave qq = quarter): wave qq adds the groups qq, qq + 4, ...
// eight loads in flight, and the four quarter sums are added in a fixed
// order.  Every thread returns its lane's total.
__device__ __forceinline__ double quartered_sum(const double* __restrict__ p, int64_t stride, int G,
                                                double (&quarter)[4][64], int lane, int qq) {
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int gg = qq;
  for (; gg + 28 < G; gg += 32) {
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += p[int64_t(gg + 4 * u) * stride];
  }
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (gg + 4 * u < G) s[u] += p[int64_t(gg + 4 * u) * stride];
  quarter[qq][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  return (quarter[0][lane] + quarter[1][lane]) + (quarter[2][lane] + quarter[3][lane]);
}

// M (K x K, fp64, both triangles) = the tiles' partials summed over the chunk
// groups in four fixed-order quarters (as tri_finish_kernel)
__global__ __launch_bounds__(256) void gram_sum_kernel(const double* __restrict__ partial, int G, int K,
                                                       double* __restrict__ M) {
  __shared__ double quarter[4][64];
  const int nb = gram_groups(K), NT = nb * (nb + 1) / 2, E = NT * 256;
  const int lane = threadIdx.x & 63, qq = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int ec = e < E ? e : E - 1;
  const double v = quartered_sum(partial + ec, E, G, quarter, lane, qq);
  if (qq != 0 || e >= E) return;
  const int2 ab = gram_tile(e >> 8, nb);
  const int row = 16 * ab.x + ((e >> 4) & 15), col = 16 * ab.y + (e & 15);
  if (row >= K || col >= K) return;
  M[int64_t(row) * K + col] = v;  // a diagonal tile writes both orders itself (the same fp32 chains)
  if (ab.x != ab.y) M[int64_t(col) * K + row] = v;
}

// D[i][j] = max(0, M_ii + M_jj - 2 M_ij), 0 on the diagonal
__global__ __launch_bounds__(256) void gram_dist_kernel(const double* __restrict__ M, int K, double* __restrict__ D) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= int64_t(K) * K) return;
  const int i = int(e / K), j = int(e % K);
  // M_ij + M_ji: a diagonal tile of the split kernel computes the two in a
  // different MFMA order (h_i m_j before m_i h_j), so they may differ in the
  // last bits; the sum keeps D exactly symmetric (= 2 M_ij when M is)
  const double d = (M[int64_t(i) * K + i] + M[int64_t(j) * K + j]) - (M[e] + M[int64_t(j) * K + i]);
  // negative rounding residue clamps to 0; NaN and inf pass through, so a
  // non-finite client (inf elements, or squares beyond fp32) reaches
  // gram_condition and sends "auto" to the exact kernel
  D[e] = i == j ? 0.0 : (d < 0.0 ? 0.0 : d);
}

// ---------------------------------------------------------------------------
// What the 16-bit Grams share (robust16.hip, pairgram_wide16.hip).

// four columns of a row as loaded (two packed 16-bit pairs) -> fp32, exactly
template <class T>
__device__ __forceinline__ f32x4 widen4(u32x2v r) {
  if constexpr (std::is_same_v<T, bf16_t>) return f32x4{bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y)};
  return f32x4{widen_f16(r.x & 0xffffu), widen_f16(r.x >> 16), widen_f16(r.y & 0xffffu), widen_f16(r.y >> 16)};
}

// fp32 -> the nearest value of the rows' dtype (ties to even), as fp32
template <class T>
__device__ __forceinline__ f32x4 round_dt4(f32x4 r) {
  if constexpr (std::is_same_v<T, bf16_t>) {
    const uint32_t a = pk_bf16(r.x, r.y), b = pk_bf16(r.z, r.w);
    return f32x4{bf16_lo(a), bf16_hi(a), bf16_lo(b), bf16_hi(b)};
  }
  return f32x4{float(_Float16(r.x)), float(_Float16(r.y)), float(_Float16(r.z)), float(_Float16(r.w))};
}

// Ends a plane-count branch: 8 wait states between the branch's last MFMA and
// whatever follows the join.  No wrong value was ever observed without it.  It
// is there for tools/mfma_hazards.py, whose rule is conservative (every
// instruction counts one wait state, and the hardware's own interlock is not
// modelled): the three branches leave the accumulators in registers of their
// own choice, and by that count the moves that reunite them (NB = 2, 3) came 7
// states after the MFMA that wrote their source, one short of the 8 the rule
// asks before a VALU read.  One s_nop 7 per stage and wave keeps every shipped
// build inside the rule instead of arguing an exception to it.
template <int N>
__device__ __forceinline__ void mfma_settle(f32x4v (&a)[N]) {
  static_assert(N >= 1 && N <= 5, "one operand per accumulator");
  if constexpr (N == 1) asm volatile("s_nop 7" : "+v"(a[0]));
  if constexpr (N == 2) asm volatile("s_nop 7" : "+v"(a[0]), "+v"(a[1]));
  if constexpr (N == 3) asm volatile("s_nop 7" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]));
  if constexpr (N == 4) asm volatile("s_nop 7" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));
  if constexpr (N == 5) asm volatile("s_nop 7" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]));
}

// ---------------------------------------------------------------------------
// What the wide (tile-pair) Grams share: pairgram_wide_kernel (robust.hip,
// which describes the decomposition) and pairgram_wide16_kernel
// (pairgram_wide16.hip).
constexpr int kWideMax = FEDAGG_PAIRGRAM_WIDE_MAX_CLIENTS;
constexpr int kWideBS = 512;
constexpr int kWidePlane = 2 * kPT * kSplitRB;  // a plane: tile I's 64 rows, then tile J's
constexpr int kWideBlocks = 2048;               // blocks the grid aims for (one per CU resident)
// a diagonal pair's tiles per wave: {A group, first B group, tiles}; waves w
// and w + 4 sit on one SIMD
[[maybe_unused]] __constant__ constexpr int kWideDiag[8][3] = {{0, 0, 2}, {1, 1, 2}, {2, 2, 2}, {1, 3, 1},
                                                               {0, 2, 1}, {0, 3, 1}, {0, 0, 0}, {3, 3, 1}};

// M (K x K, fp64, both triangles) = the tile pairs' partials summed over the
// chunk groups (gram_sum_kernel's order).  A block owns 64 entries of one
// 16 x 16 group-tile; a diagonal pair's tiles a > b do not exist and come from
// their mirrors.
[[maybe_unused]] __global__ __launch_bounds__(256) void gram_wide_sum_kernel(const double* __restrict__ partial,
                                                                             int G, int K, double* __restrict__ M) {
  __shared__ double quarter[4][64];
  const int T = (K + kPT - 1) / kPT;
  const int64_t E = int64_t(T * (T + 1) / 2) * (kPT * kPT);
  const int lane = threadIdx.x & 63, qq = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  const int2 tile = tile_of(e >> 12, T);
  const int a = (e >> 10) & 3, b = (e >> 8) & 3;
  const bool dg = tile.x == tile.y;
  if (dg && a > b) return;  // block-uniform
  const double v = quartered_sum(partial + e, E, G, quarter, lane, qq);
  if (qq != 0) return;
  const int row = tile.x * kPT + 16 * a + ((e >> 4) & 15), col = tile.y * kPT + 16 * b + (e & 15);
  if (row >= K || col >= K) return;
  M[int64_t(row) * K + col] = v;  // a diagonal group-tile writes both orders itself
  if (!(dg && a == b)) M[int64_t(col) * K + row] = v;
}

// grid_groups' blocks per group that make a wide kernel's grid about
// kWideBlocks blocks (grid_groups aims for 4096)
[[maybe_unused]] int wide_group_blocks(int NT) { return NT * (4096 / kWideBlocks); }

int grid_groups(int per_group_blocks, int64_t n_chunks, int64_t work_len, int64_t per_group_work) {
  int64_t G = (4096 + per_group_blocks - 1) / per_group_blocks;
  if (G > n_chunks) G = n_chunks;
  if (per_group_work > 0 && G > work_len / per_group_work) G = work_len / per_group_work;
  if (G > 65535) G = 65535;
  return int(G < 1 ? 1 : G);
}

int pair_tiles(int K) { const int T = (K + kPT - 1) / kPT; return T * (T + 1) / 2; }

// fedagg_pairdist2_f32 / fedagg_pairdist2_16: the argument checks, the kernel
// for K (the one-block triangle up to 128 clients, 64-client tile pairs above)
// and its finish, for rows of element type T
template <class T>
int launch_pairdist(const char* what, const T* const* d_src, int32_t K, const int64_t* d_chunks, int64_t n_chunks,
                    double* d_out, double* d_work, int64_t work_len, fedagg_stream_t stream) {
  if (K < 1 || n_chunks < 0) return set_error(FEDAGG_EINVAL, std::string(what) + ": K must be >= 1 and n_chunks >= 0");
  if (!d_src || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, std::string(what) + ": null pointer");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * K * K, st) != hipSuccess) return check_launch(what);
    return FEDAGG_OK;
  }
  if (K <= kTriMax) {  // the whole triangle in one block per chunk group
    const int64_t per = int64_t(16) * tri_blocks(K);
    if (work_len < per) return set_error(FEDAGG_EINVAL, std::string(what) + ": workspace too small (fedagg_robust_work_len)");
    const int G = grid_groups(4, n_chunks, work_len, per);
    if (K <= 64)
      hipLaunchKernelGGL((pairtri_kernel<T, 16>), dim3(unsigned(G)), dim3(unsigned(tri_threads(K))), 0, st, d_src, K,
                         d_chunks, n_chunks, G, d_work);
    else
      hipLaunchKernelGGL((pairtri_kernel<T, 32>), dim3(unsigned(G)), dim3(unsigned(tri_threads(K))), 0, st, d_src, K,
                         d_chunks, n_chunks, G, d_work);
    hipLaunchKernelGGL(tri_finish_kernel, dim3(unsigned((per + 63) / 64)), dim3(256), 0, st, d_work, G, K, d_out);
    return check_launch(what);
  }
  const int NT = pair_tiles(K);
  if (work_len < int64_t(NT) * kPT * kPT)
    return set_error(FEDAGG_EINVAL, std::string(what) + ": workspace too small (fedagg_robust_work_len)");
  const int G = grid_groups(NT, n_chunks, work_len, int64_t(NT) * kPT * kPT);
  hipLaunchKernelGGL(pairdist_kernel<T>, dim3(unsigned(NT), unsigned(G)), dim3(kBS), 0, st, d_src, K, d_chunks, n_chunks,
                     G, d_work);
  hipLaunchKernelGGL(pair_finish_kernel, dim3(unsigned(kPT * kPT / 64), unsigned(NT)), dim3(256), 0, st, d_work, G,
                     K, d_out);
  return check_launch(what);
}

}  // namespace
