// histgram.h — what the two history-Gram kernels of the "foolsgold_cos" defense
// share: histgram.hip (fp32 client rows, fedagg_histgram_f32) and
// histgram16.hip (bf16 / f16 client rows, fedagg_histgram_16).  The kernel is
// one template on the client rows' element type; histgram.hip's header
// describes the engine (pairgram_split8_kernel's) and the front of a stage,
// histgram16.hip's what 16-bit rows change in that front.  Everything here is
// internal to the including unit.
//
// histgram_kernel follows pairgram_split8_kernel (robust.hip) step for step
// where it can (the tile-run arithmetic, fetch's walk over the chunk groups,
// fold, compute, the prologue / iter pipeline and the partial stores are that
// kernel's): A FIX TO THE PIPELINE OR THE TILE SCHEDULE THERE BELONGS HERE TOO.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/fedagg.h"
#include "host_util.h"
// pairdist.h also holds the exact-difference kernels and the distance finish,
// which the history units do not launch
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "pairdist.h"

namespace {

typedef f32x4 __attribute__((address_space(1))) * gf32x4p;
typedef float __attribute__((address_space(1))) * gf32p;

// A lane's four columns of a client row (or of ref) as they are loaded and
// held until their stage is split: four fp32 values, or two packed pairs of
// raw 16-bit words (half the registers), widened when the stage is consumed.
template <class T>
constexpr bool kHistF32 = std::is_same_v<T, float>;
template <class T>
using hist_elem_t = std::conditional_t<kHistF32<T>, float, uint16_t>;
template <class T>
using hist_piece_t = std::conditional_t<kHistF32<T>, f32x4, u32x2v>;

// four columns at p, one load: 16 bytes of fp32 at any 4-byte alignment, or 8
// bytes of 16-bit words at an 8-byte aligned p
template <class T, bool NT>
__device__ __forceinline__ hist_piece_t<T> hist_ld4(const hist_elem_t<T>* p) {
  if constexpr (kHistF32<T>) {
    return ld4<NT>(p);
  } else {
    const auto q = reinterpret_cast<const u32x2v __attribute__((address_space(1)))*>(gptr(p));
    if constexpr (NT) return __builtin_nontemporal_load(q);
    return *q;
  }
}

// the same four columns c4 .. c4 + 3 of the stage at pp by element: a column
// at or past the stage's width w, and every column of a dead row, reads +0
template <class T>
__device__ __forceinline__ hist_piece_t<T> hist_ld4_elems(const hist_elem_t<T>* pp, int c4, int w, bool ok) {
  if constexpr (kHistF32<T>) {
    f32x4 v;
    v.x = ok && c4 < w ? gptr(pp)[c4] : 0.f;
    v.y = ok && c4 + 1 < w ? gptr(pp)[c4 + 1] : 0.f;
    v.z = ok && c4 + 2 < w ? gptr(pp)[c4 + 2] : 0.f;
    v.w = ok && c4 + 3 < w ? gptr(pp)[c4 + 3] : 0.f;
    return v;
  } else {
    const uint32_t e0 = ok && c4 < w ? gptr(pp)[c4] : 0u;
    const uint32_t e1 = ok && c4 + 1 < w ? gptr(pp)[c4 + 1] : 0u;
    const uint32_t e2 = ok && c4 + 2 < w ? gptr(pp)[c4 + 2] : 0u;
    const uint32_t e3 = ok && c4 + 3 < w ? gptr(pp)[c4 + 3] : 0u;
    return u32x2v{e0 | (e1 << 16), e2 | (e3 << 16)};
  }
}

// a held piece as fp32, exactly
template <class T>
__device__ __forceinline__ f32x4 hist_f32(const hist_piece_t<T>& v) {
  if constexpr (kHistF32<T>) {
    return v;
  } else {
    return widen4<T>(v);
  }
}

// a stage's raw values in flight for one lane: LPW client pieces, their
// history pieces, the ref piece, and where the stage lies (the history store
// needs it after fetch has moved on)
template <class T, int LPW, bool HIST>
struct HistRaw {
  hist_piece_t<T> x[LPW];
  f32x4 h[HIST ? LPW : 1];
  hist_piece_t<T> r;
  int64_t col0;
  int w;
};

// T: float, bf16_t or f16_t, the element type of the client rows and of ref.
// The history rows and everything after the load are fp32 whatever T is.
template <class T, int NB, bool HIST>
__global__ __launch_bounds__(kSplit8BS, 1) void histgram_kernel(const T* const* __restrict__ src, int K,
                                                              const T* __restrict__ ref,
                                                              float* const* __restrict__ hist,
                                                              const int64_t* __restrict__ chunks, int64_t n_chunks,
                                                              int G, double* __restrict__ partial) {
  constexpr int ROWS = NB * 16;
  constexpr int NT = NB * (NB + 1) / 2;
  constexpr int TPW = (NB + 2) / 2;  // ceil((NB + 1) / 2) tiles per wave, at most
  constexpr int RPW = ROWS / 8;      // staged rows per wave
  constexpr int LPW = (RPW + 3) / 4; // loads per lane, stage and operand (4 rows per wave-load)
  constexpr int PLANE = ROWS * kSplitRB;
  using Raw = HistRaw<T, LPW, HIST>;
  using E = hist_elem_t<T>;
  __shared__ __attribute__((aligned(16))) unsigned char sP[2][3 * PLANE];
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i16 = lane & 15, q = lane >> 4;
  const int c4 = 4 * i16;
  const E* const refe = reinterpret_cast<const E*>(ref);
  const E* rowp[LPW];
  float* histp[LPW];
  bool rlive[LPW];
  [[maybe_unused]] bool al = true;
#pragma unroll
  for (int u = 0; u < LPW; ++u) {
    const int lr = 4 * u + q;  // row within the wave's RPW (NB = 1, 2: RPW < 4, lanes past it idle)
    const int cl = wave * RPW + lr;
    rlive[u] = lr < RPW && cl < K;
    rowp[u] = reinterpret_cast<const E*>(src[rlive[u] ? cl : 0]);  // a dead row loads client 0's values and masks them
    histp[u] = HIST ? hist[rlive[u] ? cl : 0] : nullptr;
    if constexpr (!kHistF32<T>) al = al && (reinterpret_cast<uintptr_t>(rowp[u]) & 7) == 0;
  }
  // 16-bit rows, wave-uniform: every row of the wave, and ref, takes 8-byte
  // loads in a full stage whose first column is a multiple of 4
  [[maybe_unused]] bool rows_al = false, ref_al = false;
  if constexpr (!kHistF32<T>) {
    rows_al = __builtin_amdgcn_ballot_w64(!al) == 0;
    ref_al = (reinterpret_cast<uintptr_t>(refe) & 7) == 0;
  }
  // the row pair of this wave and its share of the pair's tiles
  const int p = wave & 3;
  const int pr1 = p, pr2 = NB - 1 - p;
  const int len1 = p < (NB + 1) / 2 ? NB - p : 0;  // row pr1's tiles (b = pr1 .. NB - 1)
  const int len2 = len1 && pr2 > pr1 ? p + 1 : 0;  // row pr2's tiles (b = pr2 .. NB - 1)
  const int half = (len1 + len2 + 1) / 2;
  const int first = wave < 4 ? 0 : half;  // this wave's tiles: pair tiles first .. first + nmine - 1
  const int nmine = wave < 4 ? half : len1 + len2 - half;
  // as (row, first column group, count) runs: at most two
  const int r1 = first < len1 ? pr1 : pr2;
  const int b1 = first < len1 ? pr1 + first : pr2 + (first - len1);
  const int n1 = first < len1 ? (len1 - first < nmine ? len1 - first : nmine) : nmine;
  const int r2 = pr2, b2 = pr2 + (first + n1 - len1 > 0 ? first + n1 - len1 : 0);
  double acc64[TPW][4];
  f32x4v acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    acc[j] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc64[j][r] = 0.0;
  }
  int64_t c = g;
  int s0 = 0;
  Raw v[2];
  auto fetch = [&](Raw& vv) __attribute__((always_inline)) {
    if (c >= n_chunks) return false;
    const int len = int(chunks[2 * c + 1]);
    const int64_t col0 = chunks[2 * c] + s0;
    const int w = len - s0 < kStage ? len - s0 : kStage;
    vv.col0 = col0;
    vv.w = w;
    if constexpr (kHistF32<T>) {
      // fp32 rows: the statements fedagg_histgram_f32's kernel had before it
      // became this template, written out (hist_ld4_elems for its partial
      // stage compiled to other code): the fp32 instantiation's instructions
      // are the ones its tests and profiles were taken on
      if (w == kStage) {
        vv.r = ld4<false>(ref + col0 + c4);
#pragma unroll
        for (int u = 0; u < LPW; ++u) {
          vv.x[u] = ld4<true>(rowp[u] + col0 + c4);
          if constexpr (HIST) vv.h[u] = ld4<true>(histp[u] + col0 + c4);
        }
      } else {
        const float* rr = ref + col0;
        vv.r.x = c4 < w ? gptr(rr)[c4] : 0.f;
        vv.r.y = c4 + 1 < w ? gptr(rr)[c4 + 1] : 0.f;
        vv.r.z = c4 + 2 < w ? gptr(rr)[c4 + 2] : 0.f;
        vv.r.w = c4 + 3 < w ? gptr(rr)[c4 + 3] : 0.f;
#pragma unroll
        for (int u = 0; u < LPW; ++u) {
          const float* pp = rowp[u] + col0;
          const bool ok = rlive[u];
          vv.x[u].x = ok && c4 < w ? gptr(pp)[c4] : 0.f;
          vv.x[u].y = ok && c4 + 1 < w ? gptr(pp)[c4 + 1] : 0.f;
          vv.x[u].z = ok && c4 + 2 < w ? gptr(pp)[c4 + 2] : 0.f;
          vv.x[u].w = ok && c4 + 3 < w ? gptr(pp)[c4 + 3] : 0.f;
          if constexpr (HIST) {
            const float* hh = histp[u] + col0;
            vv.h[u].x = ok && c4 < w ? gptr(hh)[c4] : 0.f;
            vv.h[u].y = ok && c4 + 1 < w ? gptr(hh)[c4 + 1] : 0.f;
            vv.h[u].z = ok && c4 + 2 < w ? gptr(hh)[c4 + 2] : 0.f;
            vv.h[u].w = ok && c4 + 3 < w ? gptr(hh)[c4 + 3] : 0.f;
          }
        }
      }
    } else {
      // The history pieces are fp32 at any 4-byte alignment: one 16-byte load
      // in every full stage, as the fp32 kernel's.  The 16-bit pieces are one
      // 8-byte load where the piece lies on an 8-byte boundary and by element
      // elsewhere; the branches are wave-uniform (scalar conditions), so the
      // loads of a full aligned stage are issued with no per-lane condition
      // and stay in flight until the stage is split.
      const bool full = w == kStage, a4 = (col0 & 3) == 0;
      if (full && ref_al && a4)
        vv.r = hist_ld4<T, false>(refe + col0 + c4);
      else
        vv.r = hist_ld4_elems<T>(refe + col0, c4, w, true);
      if (full && rows_al && a4) {
#pragma unroll
        for (int u = 0; u < LPW; ++u) vv.x[u] = hist_ld4<T, true>(rowp[u] + col0 + c4);
      } else {
#pragma unroll
        for (int u = 0; u < LPW; ++u) vv.x[u] = hist_ld4_elems<T>(rowp[u] + col0, c4, w, rlive[u]);
      }
      if constexpr (HIST) {
        if (full) {
#pragma unroll
          for (int u = 0; u < LPW; ++u) vv.h[u] = ld4<true>(histp[u] + col0 + c4);
        } else {
#pragma unroll
          for (int u = 0; u < LPW; ++u) vv.h[u] = hist_ld4_elems<float>(histp[u] + col0, c4, w, rlive[u]);
        }
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
  // a = fl(fl(x - ref) + h) for the lane's pieces of stage vv: into the
  // history rows (live rows, the stage's columns only) and the three planes
  auto stage_split = [&](const Raw& vv, unsigned char* P) __attribute__((always_inline)) {
    const f32x4 r = hist_f32<T>(vv.r);
#pragma unroll
    for (int u = 0; u < LPW; ++u) {
      if (4 * u + q < RPW) {
        f32x4 a = hist_f32<T>(vv.x[u]) - r;
        if constexpr (HIST) {
          a = a + vv.h[u];
          if (rlive[u]) {
            float* hp = histp[u] + vv.col0 + c4;
            if (vv.w == kStage) {
              __builtin_nontemporal_store(a, (gf32x4p)hp);
            } else {
              if (c4 < vv.w) __builtin_nontemporal_store(a.x, (gf32p)hp);
              if (c4 + 1 < vv.w) __builtin_nontemporal_store(a.y, (gf32p)hp + 1);
              if (c4 + 2 < vv.w) __builtin_nontemporal_store(a.z, (gf32p)hp + 2);
              if (c4 + 3 < vv.w) __builtin_nontemporal_store(a.w, (gf32p)hp + 3);
            }
          }
        }
        split3_store(masked(a, u), P + (wave * RPW + 4 * u + q) * kSplitRB + 8 * i16, PLANE);
      }
    }
  };
  int unfolded = 0;
  auto fold = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      // 16 wait states between the last MFMA writing acc[j] and this VALU
      // read, as pairgram_split8_kernel's fold documents; tools/mfma_hazards.py
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
    if (nmine > 0) {
      const unsigned char* fp = P + fo;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        // one A register set, not the Gram kernel's two: the second run's row
        // is read when the first run ends (n1 >= 1).  The history's register
        // set needs the 12 VGPRs (7 groups spilled with both), and the MFMAs
        // take a tenth of the time the rows take to arrive
        bf16x8v A[3], B[2][3];
        split_frag<PLANE>(fp, r1, ks, A);
        split_frag<PLANE>(fp, b1, ks, B[0]);
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if (j < nmine) {
            if (j == n1) split_frag<PLANE>(fp, r2, ks, A);
            if (j + 1 < nmine)
              split_frag<PLANE>(fp, j + 1 < n1 ? b1 + j + 1 : b2 + (j + 1 - n1), ks, B[(j + 1) & 1]);
            acc[j] = split_mfma6(A, B[j & 1], acc[j]);
          }
        }
      }
    }
    if (++unfolded == kSplitFold) fold();
  };
  // prologue: stages 0 and 1 loaded, stage 0 split and stored, stage 2 on its way
  bool h0 = fetch(v[0]);
  bool h1 = h0 && fetch(v[1]);
  if (h0) {
    stage_split(v[0], sP[0]);
    bool h2 = h1 && fetch(v[0]);  // stage 2
    lds_barrier();
    // iteration k (two at a time, so the register sets are static): split
    // stage k + 1 into the free plane buffer, issue stage k + 3's loads into
    // the freed registers, compute stage k, barrier
    auto iter = [&](auto cur_tag, bool& hn, bool& hnn) __attribute__((always_inline)) {
      constexpr int C = decltype(cur_tag)::value;  // k % 2
      // hn: stage k + 1 exists (in v[C ^ 1]); hnn: stage k + 2 (in v[C])
      bool hnnn = false;
      if (hn) {
        stage_split(v[C ^ 1], sP[C ^ 1]);
        hnnn = hnn && fetch(v[C ^ 1]);  // stage k + 3
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

// gram_sum_kernel for a Gram that is itself the result: M (K x K, fp64) = the
// tiles' partials summed over the chunk groups in the same four fixed-order
// quarters.  A diagonal tile holds both (i, j) and (j, i), whose fp32 chains
// add h_i m_j and m_i h_j in opposite orders and may differ in the last bits:
// only its entries on and above the diagonal are taken and mirrored, so M
// equals its transpose bit for bit.
__global__ __launch_bounds__(256) void gram_sum_sym_kernel(const double* __restrict__ partial, int G, int K,
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
  if (row >= K || col >= K || row > col) return;  // row > col: a diagonal tile's lower half
  M[int64_t(row) * K + col] = v;
  if (row != col) M[int64_t(col) * K + row] = v;
}

// the chunk groups a call runs: pairgram_split8_kernel's (one block per CU)
int histgram_groups(int64_t n_chunks, int64_t work_len, int64_t per) {
  const int G = grid_groups(4096 / (256 * kGramBlocksPerCU), n_chunks, work_len, per);
  return G > kGramMaxGroups ? kGramMaxGroups : G;
}

template <class T, bool HIST>
void launch_histgram(int nb, unsigned G, hipStream_t st, const T* const* d_src, int K, const T* d_ref,
                     float* const* d_hist, const int64_t* d_chunks, int64_t n_chunks, double* d_work) {
  auto kern = histgram_kernel<T, 8, HIST>;
  switch (nb) {
    case 1: kern = histgram_kernel<T, 1, HIST>; break;
    case 2: kern = histgram_kernel<T, 2, HIST>; break;
    case 3: kern = histgram_kernel<T, 3, HIST>; break;
    case 4: kern = histgram_kernel<T, 4, HIST>; break;
    case 5: kern = histgram_kernel<T, 5, HIST>; break;
    case 6: kern = histgram_kernel<T, 6, HIST>; break;
    case 7: kern = histgram_kernel<T, 7, HIST>; break;
    default: break;
  }
  hipLaunchKernelGGL(kern, dim3(G), dim3(kSplit8BS), 0, st, d_src, K, d_ref, d_hist, d_chunks, n_chunks, int(G),
                     d_work);
}

// fedagg_histgram_f32 / fedagg_histgram_16 after the dtype: the argument
// checks (all before any HIP call), the kernel for K and the finish, for
// client rows of element type T
template <class T>
int histgram_call(const char* what, const T* const* d_src, int32_t K, const T* d_ref, float* const* d_hist,
                  const int64_t* d_chunks, int64_t n_chunks, double* d_out, double* d_work, int64_t work_len,
                  fedagg_stream_t stream) {
  if (K < 1 || K > kGramMax || n_chunks < 0)
    return set_error(FEDAGG_EINVAL, std::string(what) + ": K must be in [1, 128] and n_chunks >= 0");
  if (!d_src || !d_ref || !d_out || (n_chunks > 0 && (!d_chunks || !d_work)))
    return set_error(FEDAGG_EINVAL, std::string(what) + ": null pointer");
  const int64_t per = int64_t(gram_tiles(K)) * 256;
  if (n_chunks > 0 && work_len < per)
    return set_error(FEDAGG_EINVAL, std::string(what) + ": workspace too small (fedagg_robust_work_len)");
  auto st = static_cast<hipStream_t>(stream);
  if (n_chunks == 0) {
    if (hipMemsetAsync(d_out, 0, sizeof(double) * K * K, st) != hipSuccess) return check_launch(what);
    return FEDAGG_OK;
  }
  const int G = histgram_groups(n_chunks, work_len, per);
  if (d_hist)
    launch_histgram<T, true>(gram_groups(K), unsigned(G), st, d_src, K, d_ref, d_hist, d_chunks, n_chunks, d_work);
  else
    launch_histgram<T, false>(gram_groups(K), unsigned(G), st, d_src, K, d_ref, d_hist, d_chunks, n_chunks, d_work);
  hipLaunchKernelGGL(gram_sum_sym_kernel, dim3(unsigned((per + 63) / 64)), dim3(256), 0, st, d_work, G, K, d_out);
  return check_launch(what);
}

}  // namespace
