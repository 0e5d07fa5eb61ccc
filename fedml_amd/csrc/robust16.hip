// robust16.hip — Krum's pair distances from bf16 / f16 rows (gfx950), exported
// through include/fedagg.h and linked into libfedagg.so beside robust.hip.
//
//   fedagg_pairgram2_16  the centred Gram on the bf16 matrix cores, K <= 128
//   fedagg_pairdist2_16  the exact-difference kernels of robust.hip on 16-bit rows
//
// The Gram is robust.hip's pairgram_split8_kernel (8 waves, one block per CU,
// double-buffered bf16 planes, raw rows prefetched two stages ahead, its
// row-pair tile schedule at every group count, the same partial layout) with
// two changes that 16-bit rows allow.  (The fp32 kernel's 2 x 2 group blocks at
// 8 groups exist to share fragment reads among six-product tiles; a stage of
// one plane reads a third of them, so this kernel keeps one schedule.)
//
// 1. The stage's centre is ROUNDED TO THE ROWS' DTYPE:
//      r = rne_dtype(fl32(column sum over the K clients * fl32(1 / K))).
//    D is translation invariant, so any centre is correct.  With x and r values
//    of one format, Sterbenz' lemma makes c = x - r a value of that format
//    whenever r/2 <= x <= 2r: clients that are a common base plus small updates
//    give a c with at most 8 significant bits from bf16 rows (c IS a bf16:
//    m = l = 0 in the split c = h + m + l) and at most 11 from f16 rows (l = 0).
//
// 2. The kernel finds that out per stage while it splits, and multiplies only
//    the planes that are there.  Each lane ORs the bits of every m and every l
//    it writes; a wave ballots the two and leaves two words in its slot of
//    sNeed[stage buffer][wave] (no atomics, kept as sSum is).  After the stage's
//    barrier every wave reads the 8 slots and takes the block-uniform branch
//      P = 1: hh                   (1 MFMA per tile and k-step, 1 plane read)
//      P = 2: hh, hm, mh, mm       (4; every product exact: the exact c_i c_j)
//      P = 3: split_mfma6          (6; the fp32 kernel's terms and its bound)
//    into the same fp32 accumulators, folded into fp64 every kSplitFold stages.
//    A non-finite c needs no case of its own: h = bf16(c) is inf or NaN, so
//    c - h is NaN and so are m and l, whose bits are not zero: the stage runs
//    P = 3 and the NaN reaches the Gram as it does from fp32 rows.
//
// Rows are loaded as raw 16-bit words, four columns (8 bytes) per lane and row,
// half the fp32 kernel's prefetch registers, and widened in registers.  The
// 8-byte loads need the row pointers 8-byte aligned and the stage's first
// column a multiple of 4 (bucket rows and weight_chunks' cuts are 16-byte
// aligned multiples of 8); any other start and a partial stage load by element.
//
// pairgram16_kernel follows pairgram_split8_kernel (robust.hip) step for step:
// the tile-run arithmetic, fetch, stage_sums, fold, the prologue and the iter
// pipeline are that kernel's with 16-bit loads, the rounded centre and the
// plane count added.  It is a copy and not a template of it so that the fp32
// kernel's code stays what its profiles were taken on; A FIX TO THE PIPELINE
// OR THE TILE SCHEDULE OF EITHER KERNEL BELONGS IN BOTH.
//
// This unit is compiled without packed fp32 VALU instructions (build.py,
// UNIT_FLAGS, which gives the reason and the measured price).

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/fedagg.h"
#include "host_util.h"
#include "pairdist.h"

namespace {

// widen4, round_dt4 and mfma_settle are in pairdist.h (pairgram_wide16.hip shares them)

template <class T, int NB>
__global__ __launch_bounds__(kSplit8BS, 1) void pairgram16_kernel(const T* const* __restrict__ src, int K,
                                                                const int64_t* __restrict__ chunks, int64_t n_chunks,
                                                                int G, double* __restrict__ partial) {
  constexpr int ROWS = NB * 16;
  constexpr int NT = NB * (NB + 1) / 2;
  constexpr int TPW = (NB + 2) / 2;  // tiles per wave, at most
  constexpr int RPW = ROWS / 8;      // staged rows per wave
  constexpr int LPW = (RPW + 3) / 4; // 8-byte loads per lane and stage (4 rows per wave-load)
  constexpr int PLANE = ROWS * kSplitRB;
  __shared__ __attribute__((aligned(16))) unsigned char sP[2][3 * PLANE];
  __shared__ float sSum[2][8][kStage];
  __shared__ __attribute__((aligned(16))) uint32_t sNeed[2][8][2];  // per wave: any m bit, any l bit of the stage
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i16 = lane & 15, q = lane >> 4;
  const uint16_t* rowp[LPW];
  bool rlive[LPW];
  bool al = true;
#pragma unroll
  for (int u = 0; u < LPW; ++u) {
    const int lr = 4 * u + q;  // row within the wave's RPW (NB = 1: RPW < 4, lanes past it idle)
    const int cl = wave * RPW + lr;
    rlive[u] = lr < RPW && cl < K;
    rowp[u] = reinterpret_cast<const uint16_t*>(src[rlive[u] ? cl : 0]);
    al = al && (reinterpret_cast<uintptr_t>(rowp[u]) & 7) == 0;
  }
  const bool rows_al = __builtin_amdgcn_ballot_w64(!al) == 0;  // wave-uniform: every row takes 8-byte loads
  // the row pair of this wave and its share of the pair's tiles (pairgram_split8_kernel's schedule)
  const int p = wave & 3;
  const int pr1 = p, pr2 = NB - 1 - p;
  const int len1 = p < (NB + 1) / 2 ? NB - p : 0;
  const int len2 = len1 && pr2 > pr1 ? p + 1 : 0;
  const int half = (len1 + len2 + 1) / 2;
  const int first = wave < 4 ? 0 : half;
  const int nmine = wave < 4 ? half : len1 + len2 - half;
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
  u32x2v v[2][LPW];  // raw 16-bit words: columns 4 i16 .. + 3 of the lane's rows
  auto fetch = [&](u32x2v (&vv)[LPW]) __attribute__((always_inline)) {
    if (c >= n_chunks) return false;
    const int len = int(chunks[2 * c + 1]);
    const int64_t col0 = chunks[2 * c] + s0;
    const int w = len - s0 < kStage ? len - s0 : kStage;
    const int c4 = 4 * i16;
    if (w == kStage && rows_al && (col0 & 3) == 0) {
#pragma unroll
      for (int u = 0; u < LPW; ++u)
        vv[u] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x2v __attribute__((address_space(1)))*>(gptr(rowp[u] + col0 + c4)));
    } else {  // any start, a partial stage: by element, columns past w read 0
#pragma unroll
      for (int u = 0; u < LPW; ++u) {
        const uint16_t* pp = rowp[u] + col0;
        const bool ok = rlive[u];
        const uint32_t e0 = ok && c4 < w ? gptr(pp)[c4] : 0u;
        const uint32_t e1 = ok && c4 + 1 < w ? gptr(pp)[c4 + 1] : 0u;
        const uint32_t e2 = ok && c4 + 2 < w ? gptr(pp)[c4 + 2] : 0u;
        const uint32_t e3 = ok && c4 + 3 < w ? gptr(pp)[c4 + 3] : 0u;
        vv[u] = u32x2v{e0 | (e1 << 16), e2 | (e3 << 16)};
      }
    }
    s0 += kStage;
    if (s0 >= len) {
      s0 = 0;
      c += G;
    }
    return true;
  };
  // the lane's four columns of row u as fp32, 0 for a row past K
  auto row4 = [&](const u32x2v& x, int u) __attribute__((always_inline)) {
    const uint32_t m = rlive[u] ? 0xffffffffu : 0u;
    return widen4<T>(u32x2v{x.x & m, x.y & m});
  };
  // per-wave column sums, as the fp32 kernel forms them (fixed order)
  auto stage_sums = [&](const u32x2v (&vv)[LPW], int sb) __attribute__((always_inline)) {
    f32x4 cs = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < LPW; ++u) cs += row4(vv[u], u);
#pragma unroll
    for (int m = 16; m <= 32; m <<= 1) {
      cs.x += __shfl_xor(cs.x, m, 64);
      cs.y += __shfl_xor(cs.y, m, 64);
      cs.z += __shfl_xor(cs.z, m, 64);
      cs.w += __shfl_xor(cs.w, m, 64);
    }
    if (q == 0) *reinterpret_cast<f32x4*>(&sSum[sb][wave][4 * i16]) = cs;
  };
  auto stage_split = [&](const u32x2v (&vv)[LPW], int sb, unsigned char* P) __attribute__((always_inline)) {
    f32x4 r;
    {
      f32x4 s8[8];
#pragma unroll
      for (int w = 0; w < 8; ++w) s8[w] = *reinterpret_cast<const f32x4*>(&sSum[sb][w][4 * i16]);
      r = round_dt4<T>((((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]))) * invK);
    }
    uint32_t mbits = 0, lbits = 0;
#pragma unroll
    for (int u = 0; u < LPW; ++u) {
      if (4 * u + q < RPW) {
        f32x4 cc = row4(vv[u], u) - r;
        if (!rlive[u]) cc = f32x4{0.f, 0.f, 0.f, 0.f};  // a row past K: no say in the stage's plane count
        const uint32_t h01 = pk_bf16(cc.x, cc.y), h23 = pk_bf16(cc.z, cc.w);
        const float e0 = cc.x - bf16_lo(h01), e1 = cc.y - bf16_hi(h01);
        const float e2 = cc.z - bf16_lo(h23), e3 = cc.w - bf16_hi(h23);
        const uint32_t m01 = pk_bf16(e0, e1), m23 = pk_bf16(e2, e3);
        const uint32_t l01 = pk_bf16(e0 - bf16_lo(m01), e1 - bf16_hi(m01));
        const uint32_t l23 = pk_bf16(e2 - bf16_lo(m23), e3 - bf16_hi(m23));
        mbits |= m01 | m23;
        lbits |= l01 | l23;
        unsigned char* d = P + (wave * RPW + 4 * u + q) * kSplitRB + 8 * i16;
        *reinterpret_cast<u32x2v*>(d) = u32x2v{h01, h23};
        *reinterpret_cast<u32x2v*>(d + PLANE) = u32x2v{m01, m23};
        *reinterpret_cast<u32x2v*>(d + 2 * PLANE) = u32x2v{l01, l23};
      }
    }
    // a zero of either sign is no plane; NaN bits are (see the head of the file)
    const bool anyM = __builtin_amdgcn_ballot_w64((mbits & 0x7fff7fffu) != 0) != 0;
    const bool anyL = __builtin_amdgcn_ballot_w64((lbits & 0x7fff7fffu) != 0) != 0;
    if (lane == 0) *reinterpret_cast<u32x2v*>(&sNeed[sb][wave][0]) = u32x2v{anyM ? 1u : 0u, anyL ? 1u : 0u};
  };
  int unfolded = 0;
  auto fold = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
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
  // one stage's tiles with NP planes
  auto tiles = [&](auto np_tag, const unsigned char* P) __attribute__((always_inline)) {
    constexpr int NP = decltype(np_tag)::value;
    const unsigned char* fp = P + fo;
    if (nmine > 0) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8v A1[3], A2[3], B[2][3];
        split_frag<PLANE, NP>(fp, r1, ks, A1);
        split_frag<PLANE, NP>(fp, b1, ks, B[0]);
        if (n2) split_frag<PLANE, NP>(fp, r2, ks, A2);
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if (j < nmine) {
            if (j + 1 < nmine)
              split_frag<PLANE, NP>(fp, j + 1 < n1 ? b1 + j + 1 : b2 + (j + 1 - n1), ks, B[(j + 1) & 1]);
            acc[j] = j < n1 ? split_mfma<NP>(A1, B[j & 1], acc[j]) : split_mfma<NP>(A2, B[j & 1], acc[j]);
          }
        }
      }
    }
    mfma_settle(acc);
  };
  auto compute = [&](const unsigned char* P, int sb) __attribute__((always_inline)) {
    // the 8 waves' words of this stage (written before the last barrier): block-uniform
    const u32x4v* nd = reinterpret_cast<const u32x4v*>(&sNeed[sb][0][0]);
    const u32x4v n01 = nd[0], n23 = nd[1], n45 = nd[2], n67 = nd[3];
    const uint32_t needM = (n01.x | n01.z) | (n23.x | n23.z) | (n45.x | n45.z) | (n67.x | n67.z);
    const uint32_t needL = (n01.y | n01.w) | (n23.y | n23.w) | (n45.y | n45.w) | (n67.y | n67.w);
    const int np = __builtin_amdgcn_readfirstlane(needL ? 3 : (needM ? 2 : 1));
    if (np == 1)
      tiles(std::integral_constant<int, 1>{}, P);
    else if (np == 2)
      tiles(std::integral_constant<int, 2>{}, P);
    else
      tiles(std::integral_constant<int, 3>{}, P);
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
    // iteration k (two at a time, so the register sets are static): split
    // stage k + 1 into the free plane buffer and leave its plane words, issue
    // stage k + 3's loads, compute stage k, publish stage k + 2's sums, barrier.
    // sNeed[b] is rewritten two barriers after the compute that read it.
    auto iter = [&](auto cur_tag, bool& hn, bool& hnn) __attribute__((always_inline)) {
      constexpr int C = decltype(cur_tag)::value;  // k % 2
      bool hnnn = false;
      if (hn) {
        stage_split(v[C ^ 1], C ^ 1, sP[C ^ 1]);
        hnnn = hnn && fetch(v[C ^ 1]);  // stage k + 3
      }
      compute(sP[C], C);
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
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (j < nmine) {
      const int a = j < n1 ? r1 : r2, b = j < n1 ? b1 + j : b2 + (j - n1);
      const int tt = a * NB - a * (a - 1) / 2 + (b - a);
      double* out = partial + (int64_t(g) * NT + tt) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(4 * q + r) * 16 + i16] = acc64[j][r];
    }
  }
}

template <class T>
int launch_pairgram16(const T* const* d_src, int32_t K, const int64_t* d_chunks, int64_t n_chunks, double* d_out,
                      double* d_work, int64_t work_len, hipStream_t st) {
  const int64_t per = int64_t(gram_tiles(K)) * 256;
  const int64_t mat = int64_t(K) * K;
  int G = grid_groups(4096 / (256 * kGramBlocksPerCU), n_chunks, work_len - mat, per);
  if (G > kGramMaxGroups) G = kGramMaxGroups;  // one block per CU
  double* M = d_work + int64_t(G) * per;
  auto kern = pairgram16_kernel<T, 8>;
  switch (gram_groups(K)) {
    case 1: kern = pairgram16_kernel<T, 1>; break;
    case 2: kern = pairgram16_kernel<T, 2>; break;
    case 3: kern = pairgram16_kernel<T, 3>; break;
    case 4: kern = pairgram16_kernel<T, 4>; break;
    case 5: kern = pairgram16_kernel<T, 5>; break;
    case 6: kern = pairgram16_kernel<T, 6>; break;
    case 7: kern = pairgram16_kernel<T, 7>; break;
    default: break;
  }
  hipLaunchKernelGGL(kern, dim3(unsigned(G)), dim3(kSplit8BS), 0, st, d_src, K, d_chunks, n_chunks, G, d_work);
  hipLaunchKernelGGL(gram_sum_kernel, dim3(unsigned((per + 63) / 64)), dim3(256), 0, st, d_work, G, K, M);
  hipLaunchKernelGGL(gram_dist_kernel, dim3(unsigned((mat + 255) / 256)), dim3(256), 0, st, M, K, d_out);
  return check_launch("fedagg_pairgram2_16");
}

}  // namespace

extern "C" {

int fedagg_pairgram2_16(int32_t dtype, const void* const* d_src, int32_t K, const int64_t* d_chunks,
                        int64_t n_chunks, double* d_out, double* d_work, int64_t work_len, fedagg_stream_t stream) {
  if (dtype != FEDAGG_DT_BF16 && dtype != FEDAGG_DT_F16)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
  if (K < 1 || K > kGramMax || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_16: K must be in [1, 128] and n_chunks >= 0");
  if (!d_src || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_16: null pointer");
  if (n_chunks > 0 && work_len < int64_t(gram_tiles(K)) * 256 + int64_t(K) * K)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_16: workspace too small (fedagg_robust_work_len)");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * K * K, st) != hipSuccess) return check_launch("fedagg_pairgram2_16");
    return FEDAGG_OK;
  }
  if (dtype == FEDAGG_DT_BF16)
    return launch_pairgram16(reinterpret_cast<const bf16_t* const*>(d_src), K, d_chunks, n_chunks, d_out, d_work,
                             work_len, st);
  return launch_pairgram16(reinterpret_cast<const f16_t* const*>(d_src), K, d_chunks, n_chunks, d_out, d_work,
                           work_len, st);
}

int fedagg_pairdist2_16(int32_t dtype, const void* const* d_src, int32_t K, const int64_t* d_chunks,
                        int64_t n_chunks, double* d_out, double* d_work, int64_t work_len, fedagg_stream_t stream) {
  if (dtype == FEDAGG_DT_BF16)
    return launch_pairdist("fedagg_pairdist2_16", reinterpret_cast<const bf16_t* const*>(d_src), K, d_chunks,
                           n_chunks, d_out, d_work, work_len, stream);
  if (dtype == FEDAGG_DT_F16)
    return launch_pairdist("fedagg_pairdist2_16", reinterpret_cast<const f16_t* const*>(d_src), K, d_chunks,
                           n_chunks, d_out, d_work, work_len, stream);
  return set_error(FEDAGG_EINVAL, "fedagg_pairdist2_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
}

}  // extern "C"
