// pairgram_wide16.hip — Krum's pair distances from bf16 / f16 rows for up to
// 1024 clients (gfx950), exported through include/fedagg.h and linked into
// libfedagg.so beside robust.hip and robust16.hip.
//
//   fedagg_pairgram2_wide_16  the centred Gram by 64-client tile pairs on 16-bit rows
//
// The block and the grid are pairgram_wide_kernel's (robust.hip): the K x K
// pair matrix cut into 64-client tiles (I <= J), a block of 8 waves owning one
// tile pair over the chunk groups g, g + G, ..., one block per CU, the grid
// running tile pairs fastest so that resident blocks share 64-row panels
// through L2 (plain loads, not non-temporal ones).  128 plane rows of kSplitRB
// bytes, double-buffered, one lds_barrier per stage, raw rows prefetched two
// stages ahead.  An off-diagonal pair is 4 x 4 group tiles (wave w: A group
// w / 2 against two B groups), a diagonal pair the 10-tile triangle of
// kWideDiag, staged by waves 0 - 3 only.  The partial layout
// [g][tile pair][16 group-tiles][16 x 16], gram_wide_sum_kernel and the
// distance finish are that kernel's, and so is the workspace.
//
// The stage front is pairgram16_kernel's (robust16.hip), with two differences
// that the tile-pair form brings.
//
// 1. No block sees all K rows, so the centre is an argument: one device row OF
//    THE ROWS' DTYPE.  x and r are then values of one format and, for clients
//    that are a base plus small updates, c = x - r is a value of that format
//    (Sterbenz): a bf16 from bf16 rows (m = l = 0 in c = h + m + l), at most 11
//    bits from f16 rows (l = 0).  There are no column sums and no sSum
//    exchange, so a stage needs ONE barrier and nothing before its split.
//
// 2. The plane count is per stage AND PER BLOCK, i.e. per tile pair.  Each lane
//    ORs the m and l bits it writes, a wave ballots them into its slot
//    sNeed[buffer][wave], and after the stage's barrier the block takes the
//    uniform branch P = 1 (hh), 2 (hh, hm, mh, mm: every product exact) or 3
//    (split_mfma6).  EVERY wave writes its slot in every stage it splits: a
//    wave that stages nothing (waves 4 - 7 of a diagonal pair) writes zeros,
//    so no slot is ever read stale.  A row past K is zeroed before the split
//    and has no say.  One outlier element raises the MFMA count only in its
//    stage and only in the T + 1 tile pairs that hold its client.
//    A non-finite c gives NaN m and l (robust16.hip), so its stage runs P = 3
//    and the NaN reaches the Gram.
//
// Rows and the centre load as raw 16-bit words, four columns per lane and row
// in one 8-byte load, widened in registers.  A wave's stage takes that path
// when its 16 row pointers and the centre pointer are 8-byte aligned, the
// stage is full and its first column is a multiple of 4; it loads by element
// otherwise.
//
// pairgram_wide16_kernel follows pairgram_wide_kernel step for step (tile
// arithmetic, fetch, fold, the prologue and the iter pipeline) and takes
// stage_split's plane words and the P = 1 / 2 / 3 branch from
// pairgram16_kernel.  It is a copy and not a template of either so that their
// code stays what their profiles were taken on; A FIX TO THE PIPELINE OR THE
// TILE SCHEDULE OF pairgram_wide_kernel, OR TO THE SPLIT AND PLANE COUNT OF
// pairgram16_kernel, BELONGS HERE TOO, AND THE OTHER WAY ROUND.
//
// This unit is compiled without packed fp32 VALU instructions (build.py,
// UNIT_FLAGS, which gives the reason).

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/fedagg.h"
#include "host_util.h"
// pairdist.h also holds the exact-difference and the narrow Gram's pieces,
// which this unit does not launch
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "pairdist.h"

namespace {

typedef const u32x2v __attribute__((address_space(1))) * gu32x2p;

template <class T>
__global__ __launch_bounds__(kWideBS, 1) void pairgram_wide16_kernel(const T* const* __restrict__ src, int K,
                                                                     const T* __restrict__ center_t,
                                                                     const int64_t* __restrict__ chunks,
                                                                     int64_t n_chunks, int G,
                                                                     double* __restrict__ partial) {
  constexpr int LPW = 4;  // 8-byte loads per lane and stage: 16 rows a wave, 4 rows per wave-load
  __shared__ __attribute__((aligned(16))) unsigned char sP[2][3 * kWidePlane];
  __shared__ __attribute__((aligned(16))) uint32_t sNeed[2][8][2];  // per wave: any m bit, any l bit of the stage
  const int tp = blockIdx.x, g = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i16 = lane & 15, q = lane >> 4;
  const int2 tile = tile_of(tp, (K + kPT - 1) / kPT);
  const bool diag = tile.x == tile.y;
  const bool stager = !diag || wave < 4;  // a diagonal pair has 64 rows to stage
  const uint16_t* center = reinterpret_cast<const uint16_t*>(center_t);
  const uint16_t* rowp[LPW];
  bool rlive[LPW];
  bool al = (reinterpret_cast<uintptr_t>(center) & 7) == 0;
#pragma unroll
  for (int u = 0; u < LPW; ++u) {
    const int lr = wave * 16 + 4 * u + q;  // plane row
    const int cl = lr < kPT ? tile.x * kPT + lr : tile.y * kPT + (lr - kPT);
    rlive[u] = stager && cl < K;
    rowp[u] = reinterpret_cast<const uint16_t*>(src[rlive[u] ? cl : 0]);  // a row past K reads row 0 and is zeroed
    al = al && (reinterpret_cast<uintptr_t>(rowp[u]) & 7) == 0;
  }
  const bool rows_al = __builtin_amdgcn_ballot_w64(!al) == 0;  // wave-uniform: rows and centre take 8-byte loads
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
  u32x2v v[2][LPW], cen[2];  // raw 16-bit words: columns 4 i16 .. + 3 of the lane's rows and of the centre
  auto fetch = [&](u32x2v (&vv)[LPW], u32x2v& rr) __attribute__((always_inline)) {
    if (c >= n_chunks) return false;
    const int len = int(chunks[2 * c + 1]);
    const int64_t col0 = chunks[2 * c] + s0;
    const int w = len - s0 < kStage ? len - s0 : kStage;
    const int c4 = 4 * i16;
    if (stager) {
      if (w == kStage && rows_al && (col0 & 3) == 0) {
#pragma unroll
        for (int u = 0; u < LPW; ++u) vv[u] = *reinterpret_cast<gu32x2p>(gptr(rowp[u] + col0 + c4));
        rr = *reinterpret_cast<gu32x2p>(gptr(center + col0 + c4));
      } else {  // any start, a partial stage: by element; columns past w read 0 in the rows and the centre: c = 0
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
        const uint16_t* pc = center + col0;
        const uint32_t r0 = c4 < w ? gptr(pc)[c4] : 0u;
        const uint32_t r1 = c4 + 1 < w ? gptr(pc)[c4 + 1] : 0u;
        const uint32_t r2 = c4 + 2 < w ? gptr(pc)[c4 + 2] : 0u;
        const uint32_t r3 = c4 + 3 < w ? gptr(pc)[c4 + 3] : 0u;
        rr = u32x2v{r0 | (r1 << 16), r2 | (r3 << 16)};
      }
    }
    s0 += kStage;
    if (s0 >= len) {
      s0 = 0;
      c += G;
    }
    return true;
  };
  // split the wave's 16 rows of a stage into the planes at P and leave the
  // wave's plane words in sNeed[sb][wave]; a wave that stages nothing leaves
  // zeros there (mbits = lbits = 0), never a stale slot
  auto stage_split = [&](const u32x2v (&vv)[LPW], const u32x2v& rr, int sb, unsigned char* P)
                         __attribute__((always_inline)) {
    uint32_t mbits = 0, lbits = 0;
    if (stager) {
      const f32x4 r = widen4<T>(rr);
#pragma unroll
      for (int u = 0; u < LPW; ++u) {
        f32x4 cc = widen4<T>(vv[u]) - r;
        if (!rlive[u]) cc = f32x4{0.f, 0.f, 0.f, 0.f};  // a row past K: zero planes, no say in the plane count
        const uint32_t h01 = pk_bf16(cc.x, cc.y), h23 = pk_bf16(cc.z, cc.w);
        const float e0 = cc.x - bf16_lo(h01), e1 = cc.y - bf16_hi(h01);
        const float e2 = cc.z - bf16_lo(h23), e3 = cc.w - bf16_hi(h23);
        const uint32_t m01 = pk_bf16(e0, e1), m23 = pk_bf16(e2, e3);
        const uint32_t l01 = pk_bf16(e0 - bf16_lo(m01), e1 - bf16_hi(m01));
        const uint32_t l23 = pk_bf16(e2 - bf16_lo(m23), e3 - bf16_hi(m23));
        mbits |= m01 | m23;
        lbits |= l01 | l23;
        unsigned char* d = P + (wave * 16 + 4 * u + q) * kSplitRB + 8 * i16;
        *reinterpret_cast<u32x2v*>(d) = u32x2v{h01, h23};
        *reinterpret_cast<u32x2v*>(d + kWidePlane) = u32x2v{m01, m23};
        *reinterpret_cast<u32x2v*>(d + 2 * kWidePlane) = u32x2v{l01, l23};
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
  // one stage's tiles with NP planes
  auto tiles = [&](auto np_tag, const unsigned char* P) __attribute__((always_inline)) {
    constexpr int NP = decltype(np_tag)::value;
    if (nt > 0) {
      const unsigned char* fp = P + fo;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8v A[3], B[2][3];
        split_frag<kWidePlane, NP>(fp, ga, ks, A);
        split_frag<kWidePlane, NP>(fp, gb, ks, B[0]);
        split_frag<kWidePlane, NP>(fp, nt > 1 ? gb + 1 : gb, ks, B[1]);
        acc[0] = split_mfma<NP>(A, B[0], acc[0]);
        if (nt > 1) acc[1] = split_mfma<NP>(A, B[1], acc[1]);
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
  // prologue: stages 0 and 1 loaded, stage 0 split
  bool h0 = fetch(v[0], cen[0]);
  bool h1 = h0 && fetch(v[1], cen[1]);
  if (h0) {
    stage_split(v[0], cen[0], 0, sP[0]);
    bool h2 = h1 && fetch(v[0], cen[0]);  // stage 2
    lds_barrier();
    // iteration k (two at a time, so the register sets are static): split
    // stage k + 1 into the free plane buffer and leave its plane words, issue
    // stage k + 3's loads into the freed registers, compute stage k, barrier.
    // sNeed[b] and sP[b] are rewritten only after the barrier that ends the
    // compute that read them.
    auto iter = [&](auto cur_tag, bool& hn, bool& hnn) __attribute__((always_inline)) {
      constexpr int C = decltype(cur_tag)::value;  // k % 2
      // hn: stage k + 1 exists (in v[C ^ 1]); hnn: stage k + 2 (in v[C])
      bool hnnn = false;
      if (hn) {
        stage_split(v[C ^ 1], cen[C ^ 1], C ^ 1, sP[C ^ 1]);
        hnnn = hnn && fetch(v[C ^ 1], cen[C ^ 1]);  // stage k + 3
      }
      compute(sP[C], C);
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

template <class T>
int launch_wide16(const void* const* d_src, int32_t K, const void* d_center, const int64_t* d_chunks,
                  int64_t n_chunks, double* d_out, double* d_work, int64_t work_len, hipStream_t st) {
  const int NT = pair_tiles(K);
  const int64_t per = int64_t(NT) * kPT * kPT;
  const int64_t mat = int64_t(K) * K;
  const int G = grid_groups(wide_group_blocks(NT), n_chunks, work_len - mat, per);
  double* M = d_work + int64_t(G) * per;
  hipLaunchKernelGGL(pairgram_wide16_kernel<T>, dim3(unsigned(NT), unsigned(G)), dim3(kWideBS), 0, st,
                     reinterpret_cast<const T* const*>(d_src), K, static_cast<const T*>(d_center), d_chunks, n_chunks,
                     G, d_work);
  hipLaunchKernelGGL(gram_wide_sum_kernel, dim3(unsigned(per / 64)), dim3(256), 0, st, d_work, G, K, M);
  hipLaunchKernelGGL(gram_dist_kernel, dim3(unsigned((mat + 255) / 256)), dim3(256), 0, st, M, K, d_out);
  return check_launch("fedagg_pairgram2_wide_16");
}

}  // namespace

extern "C" {

int fedagg_pairgram2_wide_16(int32_t dtype, const void* const* d_src, int32_t K, const void* d_center,
                             const int64_t* d_chunks, int64_t n_chunks, double* d_out, double* d_work,
                             int64_t work_len, fedagg_stream_t stream) {
  if (dtype != FEDAGG_DT_BF16 && dtype != FEDAGG_DT_F16)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_wide_16: dtype must be FEDAGG_DT_BF16 or FEDAGG_DT_F16");
  if (K < 1 || K > kWideMax || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_wide_16: K must be in [1, 1024] and n_chunks >= 0");
  if (!d_src || !d_center || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_wide_16: null pointer");
  if (n_chunks > 0 && work_len < int64_t(pair_tiles(K)) * kPT * kPT + int64_t(K) * K)
    return set_error(FEDAGG_EINVAL, "fedagg_pairgram2_wide_16: workspace too small (fedagg_robust_work_len)");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * K * K, st) != hipSuccess)
      return check_launch("fedagg_pairgram2_wide_16");
    return FEDAGG_OK;
  }
  if (dtype == FEDAGG_DT_BF16)
    return launch_wide16<bf16_t>(d_src, K, d_center, d_chunks, n_chunks, d_out, d_work, work_len, st);
  return launch_wide16<f16_t>(d_src, K, d_center, d_chunks, n_chunks, d_out, d_work, work_len, st);
}

}  // extern "C"
