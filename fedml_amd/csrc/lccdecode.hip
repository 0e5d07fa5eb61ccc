// lccdecode.hip — LightSecAgg's mask decode (LCC_decoding_with_points,
// core/mpc/lightsecagg.py): out = (coef · F) mod p, coef R x U, F U x M, all
// int64, numpy semantics (products and sums wrap mod 2^64, floor modulo).
// It is a GEMM over a prime field and the one model-sized step of the
// LightSecAgg server round that FedML leaves to numpy, which has no BLAS for
// int64.  Two kernels (include/fedagg.h, fedagg_lcc_decode_i64):
//
// lcc_exact_kernel — the specification for every input.  One lane per column,
// kRT output rows per lane in 64-bit accumulators; consecutive blocks walk the
// row tiles of the same columns, so F is re-read through L2, not HBM.  The
// coefficients and the row pointers are wave-uniform: scalar loads.  The
// wrapping product is lo·lo (one v_mad_u64_u32 into the accumulator) plus the
// two cross terms, which only reach bits 32..63 and are summed in a 32-bit
// side accumulator; when no coefficient of the row tile and no element of the
// wave's 64 columns has a high word (field data: always) the cross terms are
// skipped by one wave-uniform branch per source row.
//
// lcc_mfma_kernel — field data (0 <= coef, F < p, p <= kMaxBytePrime) on the
// int8 matrix cores.  Only the residue matters and nothing wraps, so each value
// is replaced by its centred representative r (|r| <= p / 2) and split as
// r = 256 hi + lo with lo = the sign-extended low byte.  hi is in [-128, 127]
// iff -32896 <= r <= 32639, and |r| <= floor(p / 2), so p <= 65279.  Then
//   Σ c x = 65536 Σ ch xh + 256 Σ (ch xl + cl xh) + Σ cl xl,
// three int32 accumulators of v_mfma_i32_16x16x64_i8 (hl and lh share one):
// |digit| <= 128, so |Σ| <= 2 · 2^14 · 1024 = 2^25, exact.  A block owns 64
// columns for ALL U rows: it reads each int64 of F once from HBM, range-checks,
// centres, splits, and writes the two byte planes to LDS transposed (column-
// major, u contiguous: the B operand's 16 consecutive k per lane, one
// ds_read_b128).  A lane converts 16 consecutive rows of one column, so the
// global reads are coalesced along the columns and the LDS writes are 16 B.
// The coefficients' planes come from lcc_coef_planes_kernel once per call
// (R and U zero-padded to 32 and 64; a zero digit adds nothing) and are read
// from L2 16 B per lane, the A operand's layout.  Each wave holds 2 row tiles
// x 2 column tiles (12 accumulators), so every operand fetched feeds two
// MFMAs.  Whatever order the hardware gives the 64 k of a lane group, A and B
// are laid out alike, and a dot product does not depend on the order.
// The epilogue combines the three sums in fp64 (integers below 2^42, exact)
// and reduces mod p with one multiply by 1 / p and a correction.
//
// Data outside the field never meets the matrix cores: a block that sees an
// element outside [0, p) writes flags[tile] = 1 and stops; an out-of-range
// coefficient (lcc_coef_planes_kernel's per-row flag) does so for every tile.
// A second launch of lcc_exact_kernel then computes exactly the flagged tiles
// (each wave reads its flag and returns early), so the result is the
// specification bit for bit without a host synchronisation.
#include "host_util.h"

#include <cstdint>

namespace {

constexpr int kNT = 64;   // columns of a tile: a wave of the exact kernel, a block of the matrix-core kernel
constexpr int kRT = 16;   // output rows a lane of the exact kernel holds
constexpr int kLdsPad = 16;  // bytes between the LDS columns beyond Kp (keeps 16-byte alignment, spreads the banks)
constexpr int64_t kMaxBytePrime = FEDAGG_LCC_MFMA_MAX_PRIME;

typedef int i32x4v __attribute__((ext_vector_type(4)));

// numpy's np.mod on int64 (as fedagg.hip's floor_mod); p > 0 here
__device__ __forceinline__ int64_t floor_mod(int64_t a, int64_t p) {
  int64_t r = a % p;
  if (r < 0) r += p;
  return r;
}

// NU source rows of the exact kernel: NU independent column loads in flight,
// then per output row NU consecutive coefficients (scalar loads) and products
template <int NU>
__device__ __forceinline__ void lcc_exact_rows(const int64_t* const* __restrict__ src, int u, int64_t n, bool live,
                                               const int64_t* __restrict__ coef, const uint32_t (&off)[kRT],
                                               uint64_t (&acc)[kRT], uint32_t (&cross)[kRT]) {
  uint32_t xl[NU], xh[NU], x_h = 0;
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const uint64_t x = live ? uint64_t(src[u + i][n]) : 0;
    xl[i] = uint32_t(x);
    xh[i] = uint32_t(x >> 32);
    x_h |= xh[i];
  }
  uint32_t cl[kRT][NU], ch[kRT][NU], any_h = __any(x_h != 0) ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < kRT; ++j)
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const uint64_t c = uint64_t(coef[off[j] + uint32_t(u + i)]);
      cl[j][i] = uint32_t(c);
      ch[j][i] = uint32_t(c >> 32);
      any_h |= ch[j][i];
    }
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int j = 0; j < kRT; ++j) acc[j] += uint64_t(cl[j][i]) * xl[i];
  if (any_h) {  // wave-uniform; never taken on field data
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
      for (int j = 0; j < kRT; ++j) cross[j] += ch[j][i] * xl[i] + cl[j][i] * xh[i];
  }
}

// flags == nullptr: every tile; else only the tiles whose flag is set
__global__ __launch_bounds__(256) void lcc_exact_kernel(const int64_t* const* __restrict__ src, int U, int64_t M,
                                                        const int64_t* __restrict__ coef, int R, int64_t p,
                                                        int64_t* __restrict__ out, int64_t n_out, int n_rt,
                                                        const int32_t* __restrict__ flags) {
  const int64_t cb = blockIdx.x / unsigned(n_rt);
  const int t0 = int(blockIdx.x - cb * n_rt) * kRT;
  const int64_t tile = cb * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (tile * kNT >= M || int64_t(t0) * M >= n_out) return;  // wave-uniform, as the next
  if (flags && flags[tile] == 0) return;
  const int64_t n = tile * kNT + (threadIdx.x & 63);
  const bool live = n < M;
  uint64_t acc[kRT];
  uint32_t cross[kRT], off[kRT];
#pragma unroll
  for (int j = 0; j < kRT; ++j) {
    acc[j] = 0;
    cross[j] = 0;
    off[j] = uint32_t(t0 + j < R ? t0 + j : R - 1) * uint32_t(U);  // rows past R repeat the last one, not stored
  }
  int u = 0;
  for (; u + 2 <= U; u += 2) lcc_exact_rows<2>(src, u, n, live, coef, off, acc, cross);
  if (u < U) lcc_exact_rows<1>(src, u, n, live, coef, off, acc, cross);
  if (!live) return;
#pragma unroll
  for (int j = 0; j < kRT; ++j) {
    const int64_t idx = int64_t(t0 + j) * M + n;
    if (t0 + j < R && idx < n_out) out[idx] = floor_mod(int64_t(acc[j] + (uint64_t(cross[j]) << 32)), p);
  }
}

// centred representative of a field element and its two signed bytes
__device__ __forceinline__ void split_digits(int32_t v, int32_t p, int32_t& hi, int32_t& lo) {
  const int32_t r = v > (p >> 1) ? v - p : v;
  lo = int32_t(int8_t(r));
  hi = (r - lo) >> 8;
}

// One block per padded coefficient row: the row's two byte planes (Kp bytes
// each, zero beyond R x U) and whether it holds a value outside [0, p).
__global__ __launch_bounds__(256) void lcc_coef_planes_kernel(const int64_t* __restrict__ coef, int U, int R, int Kp,
                                                              int32_t p, int8_t* __restrict__ a_hi,
                                                              int8_t* __restrict__ a_lo, int32_t* __restrict__ rowbad) {
  const int t = blockIdx.x;
  int bad = 0;
  for (int k = threadIdx.x; k < Kp; k += 256) {
    int64_t v = (t < R && k < U) ? coef[int64_t(t) * U + k] : 0;
    if (uint64_t(v) >= uint64_t(p)) { bad = 1; v = 0; }
    int32_t hi, lo;
    split_digits(int32_t(v), p, hi, lo);
    a_hi[int64_t(t) * Kp + k] = int8_t(hi);
    a_lo[int64_t(t) * Kp + k] = int8_t(lo);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) rowbad[t] = bad;
}

// floor_mod(65536 hh + 256 mid + ll, p) for |hh|, |ll| <= 2^24, |mid| <= 2^25, p < 2^16
__device__ __forceinline__ int64_t combine_mod(int32_t hh, int32_t mid, int32_t ll, double pd, double inv_p) {
  const double v = __builtin_fma(65536.0, double(hh), __builtin_fma(256.0, double(mid), double(ll)));
  const double q = __builtin_floor(v * inv_p);  // off by one at the most
  double r = __builtin_fma(-q, pd, v);          // exact: an integer in [-p, 2p)
  if (r < 0.0) r += pd;
  if (r >= pd) r -= pd;
  return int64_t(int32_t(r));
}

__global__ __launch_bounds__(256) void lcc_mfma_kernel(const int64_t* const* __restrict__ src, int U, int Kp, int64_t M,
                                                       const int8_t* __restrict__ a_hi,
                                                       const int8_t* __restrict__ a_lo, int R, int Rp, int32_t p,
                                                       int64_t* __restrict__ out, int64_t n_out,
                                                       const int32_t* __restrict__ rowbad,
                                                       int32_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) int8_t lds[];
  const int stride = Kp + kLdsPad;
  int8_t* b_hi = lds;
  int8_t* b_lo = lds + kNT * stride;
  const int64_t tile = blockIdx.x, n0 = tile * kNT;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int bad = 0;
  for (int i = threadIdx.x; i < Rp; i += 256) bad |= rowbad[i];

  // F -> centred byte planes in LDS; wave w converts the row groups w, w + 4, ...
  const bool live = n0 + lane < M;
  for (int g = w; g < (Kp >> 4); g += 4) {
    int64_t x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = (live && g * 16 + j < U) ? src[g * 16 + j][n0 + lane] : 0;
    uint32_t h4[4] = {0, 0, 0, 0}, l4[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const bool in = uint64_t(x[j]) < uint64_t(p);
      bad |= !in;
      int32_t hi, lo;
      split_digits(in ? int32_t(x[j]) : 0, p, hi, lo);
      h4[j >> 2] |= uint32_t(hi & 255) << (8 * (j & 3));
      l4[j >> 2] |= uint32_t(lo & 255) << (8 * (j & 3));
    }
    *reinterpret_cast<uint4*>(b_hi + lane * stride + g * 16) = uint4{h4[0], h4[1], h4[2], h4[3]};
    *reinterpret_cast<uint4*>(b_lo + lane * stride + g * 16) = uint4{l4[0], l4[1], l4[2], l4[3]};
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) flags[tile] = bad;
  if (bad) return;  // the exact kernel's second launch computes this tile

  // wave w: column tiles 2 (w & 1), + 1; row-tile pairs w >> 1, + 2, ...
  const int li = lane & 15, g4 = lane >> 4, c0 = (w & 1) * 32;
  const double pd = double(p), inv_p = 1.0 / pd;
  for (int r0 = (w >> 1) * 32; r0 < Rp && int64_t(r0) * M < n_out; r0 += 64) {
    const i32x4v zero = {0, 0, 0, 0};
    i32x4v hh[2][2] = {{zero, zero}, {zero, zero}}, mid[2][2] = {{zero, zero}, {zero, zero}},
           ll[2][2] = {{zero, zero}, {zero, zero}};
    for (int k0 = g4 * 16; k0 < Kp; k0 += 64) {
      i32x4v ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int64_t off = int64_t(r0 + a * 16 + li) * Kp + k0;
        ah[a] = *reinterpret_cast<const i32x4v*>(a_hi + off);
        al[a] = *reinterpret_cast<const i32x4v*>(a_lo + off);
        const int boff = (c0 + a * 16 + li) * stride + k0;
        bh[a] = *reinterpret_cast<const i32x4v*>(b_hi + boff);
        bl[a] = *reinterpret_cast<const i32x4v*>(b_lo + boff);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          hh[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[a], bh[b], hh[a][b], 0, 0, 0);
          mid[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[a], bl[b], mid[a][b], 0, 0, 0);
          ll[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[a], bl[b], ll[a][b], 0, 0, 0);
          mid[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[a], bh[b], mid[a][b], 0, 0, 0);
        }
    }
    // 21 wait states between the last MFMA and the first vector read of an
    // accumulator (tools/mfma_hazards.py asks 20 of a mnemonic it has no figure for)
    asm volatile("s_nop 15\n\ts_nop 4"
                 : "+v"(hh[0][0]), "+v"(hh[0][1]), "+v"(hh[1][0]), "+v"(hh[1][1]), "+v"(mid[0][0]), "+v"(mid[0][1]),
                   "+v"(mid[1][0]), "+v"(mid[1][1]), "+v"(ll[0][0]), "+v"(ll[0][1]), "+v"(ll[1][0]), "+v"(ll[1][1]));
    // accumulator register i of lane (g4, li): row 4 g4 + i, column li of the 16 x 16 tile
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = r0 + a * 16 + g4 * 4 + i;
          const int64_t n = n0 + c0 + b * 16 + li, idx = int64_t(t) * M + n;
          if (t < R && n < M && idx < n_out) out[idx] = combine_mod(hh[a][b][i], mid[a][b][i], ll[a][b][i], pd, inv_p);
        }
  }
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct WorkLayout {
  int Kp, Rp;
  int64_t planes, rowbad, flags, total;  // byte offsets; planes: one plane's size
};

WorkLayout work_layout(int32_t U, int32_t R, int64_t M) {
  WorkLayout l;
  l.Kp = round_up(U, 64);
  l.Rp = round_up(R, 32);
  l.planes = int64_t(l.Kp) * l.Rp;
  l.rowbad = 2 * l.planes;
  l.flags = l.rowbad + 4 * int64_t(l.Rp);
  l.total = l.flags + 4 * ((M + kNT - 1) / kNT);
  return l;
}

}  // namespace

extern "C" {

int64_t fedagg_lcc_work_bytes(int32_t U, int32_t R, int64_t M) {
  if (U < 1 || R < 1 || M < 0 || U > FEDAGG_LCC_MAX_DIM || R > FEDAGG_LCC_MAX_DIM) return -1;
  return work_layout(U, R, M).total;
}

int fedagg_lcc_decode_i64(const int64_t* const* d_src, int32_t U, int64_t M, const int64_t* d_coef, int32_t R,
                          int64_t p, int64_t* d_out, int64_t n_out, int32_t method, void* d_work, int64_t work_bytes,
                          fedagg_stream_t stream) {
  const std::string what = "fedagg_lcc_decode_i64";
  if (U < 1 || R < 1 || M < 0) return set_error(FEDAGG_EINVAL, what + ": U and R must be >= 1 and M >= 0");
  if (p <= 0) return set_error(FEDAGG_EINVAL, what + ": the prime must be positive");
  if (method != FEDAGG_LCC_VALU && method != FEDAGG_LCC_MFMA)
    return set_error(FEDAGG_EINVAL, what + ": method must be FEDAGG_LCC_VALU or FEDAGG_LCC_MFMA");
  if (n_out < 0 || (M == 0 ? n_out != 0 : (n_out / M > R || (n_out / M == R && n_out % M != 0))))
    return set_error(FEDAGG_EINVAL, what + ": n_out must be in [0, R * M]");
  if (!d_src || !d_coef || !d_out) return set_error(FEDAGG_EINVAL, what + ": null pointer");
  if (U > FEDAGG_LCC_MAX_DIM || R > FEDAGG_LCC_MAX_DIM)
    return set_error(FEDAGG_ENOKERNEL, what + ": at most " + std::to_string(FEDAGG_LCC_MAX_DIM) +
                                           " source rows and coefficient rows (U = " + std::to_string(U) +
                                           ", R = " + std::to_string(R) + ")");
  const bool mfma = method == FEDAGG_LCC_MFMA && p <= kMaxBytePrime;
  const WorkLayout l = work_layout(U, R, M);
  if (mfma && (!d_work || work_bytes < l.total || (reinterpret_cast<uintptr_t>(d_work) & 15)))
    return set_error(FEDAGG_EINVAL, what + ": d_work must be 16-byte aligned and hold fedagg_lcc_work_bytes(U, R, M) = " +
                                        std::to_string(l.total) + " bytes");
  const int64_t tiles = (M + kNT - 1) / kNT;
  const int n_rt = (R + kRT - 1) / kRT;
  const int64_t exact_blocks = (tiles + 3) / 4 * n_rt;
  if (exact_blocks > 0x7fffffffLL) return set_error(FEDAGG_EINVAL, what + ": M too large");
  if (n_out == 0) return FEDAGG_OK;
  auto st = reinterpret_cast<hipStream_t>(stream);
  const int32_t* d_flags = nullptr;
  if (mfma) {
    auto* base = static_cast<int8_t*>(d_work);
    int8_t* a_hi = base;
    int8_t* a_lo = base + l.planes;
    auto* rowbad = reinterpret_cast<int32_t*>(base + l.rowbad);
    auto* flags = reinterpret_cast<int32_t*>(base + l.flags);
    const int lds_bytes = 2 * kNT * (l.Kp + kLdsPad);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lcc_mfma_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return set_error(static_cast<int>(e), what + ": " + hipGetErrorString(e));
    hipLaunchKernelGGL(lcc_coef_planes_kernel, dim3(unsigned(l.Rp)), dim3(256), 0, st, d_coef, U, R, l.Kp, int32_t(p),
                       a_hi, a_lo, rowbad);
    hipLaunchKernelGGL(lcc_mfma_kernel, dim3(unsigned(tiles)), dim3(256), lds_bytes, st, d_src, U, l.Kp, M, a_hi, a_lo,
                       R, l.Rp, int32_t(p), d_out, n_out, rowbad, flags);
    d_flags = flags;
  }
  hipLaunchKernelGGL(lcc_exact_kernel, dim3(unsigned(exact_blocks)), dim3(256), 0, st, d_src, U, M, d_coef, R, p, d_out,
                     n_out, n_rt, d_flags);
  return check_launch(what.c_str());
}

}  // extern "C"
