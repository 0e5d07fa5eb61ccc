// sortnet.h — what the one-lane-per-column selection kernels share: the
// compile-time pairwise sorting network, the element types (fp32, bf16, f16
// as fp32 "selection values"), the per-slot row load (load_slot) and, on the
// host, the chunked launch (launch_col_chunks) and the tier ladder (with_tier).
// Included by median.hip, trimmed.hip, trimmed_wide.hip, nearmedian.hip and
// nearmedian_wide.hip (and by lanesort.h, the lane-group sort above 128
// clients); everything is internal to the including translation unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <type_traits>
#include <utility>

#include "host_util.h"

// Loads of the one-lane-per-column kernels (K <= 128; 256 B per wave
// instruction): 1 non-temporal, 0 plain
constexpr int kColsNT = 1;

namespace {

// Client rows arrive through pointer tables, which hipcc cannot prove are
// global memory (see fedagg.hip): the cast keeps the loads global, not FLAT.
template <class T>
__device__ __forceinline__ const T __attribute__((address_space(1)))* as_global(const T* p) {
  return (const T __attribute__((address_space(1)))*)(p);
}

// loads of the one-lane-per-column kernels (kColsNT)
template <class T>
__device__ __forceinline__ T cols_load(const T __attribute__((address_space(1)))* p) {
  if constexpr (kColsNT)
    return __builtin_nontemporal_load(p);
  else
    return *p;
}

__device__ __forceinline__ void cmpx(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// Parberry's pairwise sorting network on N slots, generated at compile time.
// Pruned to the one output slot the median needs, it keeps 2,011 min/max at
// N = 128 where Batcher's odd-even merge sort keeps 2,299 (same 1,471
// comparators before pruning; the pairwise network's last stages feed fewer
// slots).
struct CmpPair {
  int a, b;
};
template <int N>
struct PairwiseNet {
  // emit(a, b) for every comparator in network order; returns the count
  template <class F>
  static constexpr int walk(F emit) {
    int m = 0;
    int a = 1;
    for (; a < N; a *= 2) {
      int b = a, c = 0;
      while (b < N) {
        emit(m++, b - a, b);
        ++b;
        c = (c + 1) % a;
        if (c == 0) b += a;
      }
    }
    a /= 4;
    for (int e = 1; a > 0; a /= 2, e = e * 2 + 1) {
      for (int d = e; d > 0; d /= 2) {
        int b = (d + 1) * a, c = 0;
        while (b < N) {
          emit(m++, b - d * a, b);
          ++b;
          c = (c + 1) % a;
          if (c == 0) b += a;
        }
      }
    }
    return m;
  }
  static constexpr int M = walk([](int, int, int) {});
  struct Table {
    CmpPair p[M > 0 ? M : 1];
  };
  static constexpr Table make() {
    Table t{};
    walk([&t](int m, int x, int y) { t.p[m] = CmpPair{x, y}; });
    return t;
  }
  static constexpr Table table = make();
};

// two 16-bit order keys per register: one v_pk_min_i16 + one v_pk_max_i16
typedef short short2_t __attribute__((ext_vector_type(2)));
typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void cmpx(short2_t& a, short2_t& b) {
  const short2_t lo = __builtin_elementwise_min(a, b), hi = __builtin_elementwise_max(a, b);
  a = lo;
  b = hi;
}

template <int N, int I, class T>
__device__ __forceinline__ void net_cmp(T (&v)[N]) {
  constexpr int A = PairwiseNet<N>::table.p[I].a, B = PairwiseNet<N>::table.p[I].b;
  cmpx(v[A], v[B]);
}
template <int N, class T, int... I>
__device__ __forceinline__ void net_apply(T (&v)[N], std::integer_sequence<int, I...>) {
  (net_cmp<N, I>(v), ...);
}
template <int N, class T>
__device__ __forceinline__ void pairwise_sort(T (&v)[N]) {
  net_apply<N, T>(v, std::make_integer_sequence<int, PairwiseNet<N>::M>{});
}

// Element types of the median kernels.  Every column value becomes an fp32
// "selection value" whose float order is the element's order, the networks
// select on those, and the selected value maps back to the input's bits
// exactly (it is one of the inputs).  fp32 and bf16 widen exactly (bf16 is
// the top half of an fp32).  f16 maps to an order-preserving 16-bit key
// placed in the mantissa of [1, 2): x ^ 0x8000 for positive, ~x for negative
// values, so -inf < -finite < -0 < +0 < +finite < +inf as keys, all normal
// floats, and the ±inf pads stay below / above every key.  (Widening f16 to
// fp32 with v_cvt kept both forms live and took the K = 128 kernel to 256
// VGPRs, occupancy 1.)  nan() tests a selection value for NaN.
struct MedF32 {
  using S = float;
  static __device__ __forceinline__ float widen(S x) { return x; }
  static __device__ __forceinline__ S narrow(float v) { return v; }
  static __device__ __forceinline__ bool nan(float v) { return __builtin_isnan(v); }
  static __device__ __forceinline__ bool raw_nan(S x) { return __builtin_isnan(x); }
  static constexpr bool kReloadNan = false;
  // running "any NaN so far" over the column's selection values
  using NanAcc = bool;
  static __device__ __forceinline__ void nan_add(NanAcc& a, float v) { a |= __builtin_isnan(v); }
  static __device__ __forceinline__ bool nan_any(NanAcc a) { return a; }
  static constexpr uint32_t kNegInf = 0xff800000u, kPosInf = 0x7f800000u;
};
struct IsNanAcc {
  using NanAcc = bool;
  static __device__ __forceinline__ void nan_add(NanAcc& a, float v) { a |= __builtin_isnan(v); }
  static __device__ __forceinline__ bool nan_any(NanAcc a) { return a; }
};
struct MedBF16 : IsNanAcc {
  using S = uint16_t;
  static __device__ __forceinline__ bool raw_nan(S x) { return (x & 0x7fffu) > 0x7f80u; }
  static constexpr bool kReloadNan = true;
  static __device__ __forceinline__ float widen(S x) { return __uint_as_float(uint32_t(x) << 16); }
  static __device__ __forceinline__ S narrow(float v) { return S(__float_as_uint(v) >> 16); }
  static __device__ __forceinline__ bool nan(float v) { return __builtin_isnan(v); }
  static constexpr uint32_t kNegInf = 0xff80u, kPosInf = 0x7f80u;
};
struct MedF16 {
  using S = uint16_t;
  static __device__ __forceinline__ bool raw_nan(S x) { return (x & 0x7fffu) > 0x7c00u; }
  static constexpr bool kReloadNan = true;
  // The value arrives in the high half (as bf16 does: a d16_hi load), its
  // order key is built there (x ^ 0x8000 for positive, ~x for negative values)
  // and shifted down two bits: a positive float below 2.0 whose float order
  // is the key order (normal for every non-NaN key: -inf's key 0x03ff gives
  // 0x00ffc000).
  static __device__ __forceinline__ float widen(S x) {
    const uint32_t u = uint32_t(x) << 16;
    const uint32_t neg = uint32_t(int32_t(u) >> 31);
    return __uint_as_float((u ^ (0x80000000u | (neg & 0x7fff0000u))) >> 2);
  }
  static __device__ __forceinline__ S narrow(float v) {
    const uint32_t k = (__float_as_uint(v) << 2) >> 16;  // the 16-bit key
    const uint32_t neg = ~uint32_t(int32_t(k << 16) >> 31);  // key below 0x8000: a negative value
    return S(k ^ ((neg & 0x7fffu) | 0x8000u));
  }
  static __device__ __forceinline__ uint32_t key(float v) { return (__float_as_uint(v) << 2) >> 16; }
  // NaN keys: +NaN 0x7c01..0x7fff -> 0xfc01..0xffff, -NaN 0xfc01..0xffff -> 0x0000..0x03fe
  static __device__ __forceinline__ bool nan(float v) {
    const uint32_t k = key(v);
    return __float_as_uint(v) < 0x40000000u && (k > 0xfc00u || k < 0x03ffu);
  }
  // rotated key (k - 0x3ff) mod 2^16: NaN keys land above 0xf801, every other
  // key at or below it, so one unsigned compare per value
  using NanAcc = bool;
  static __device__ __forceinline__ void nan_add(NanAcc& a, float v) { a |= ((key(v) - 0x3ffu) & 0xffffu) > 0xf801u; }
  static __device__ __forceinline__ bool nan_any(NanAcc a) { return a; }
  static constexpr uint32_t kNegInf = 0xfc00u, kPosInf = 0x7c00u;
};

// The trimmed mean kernels (trimmed.hip, trimmed_wide.hip):
// what the chain adds for a sorted selection value, and the final rounding
template <class E>
struct TrimVal;
template <>
struct TrimVal<MedF32> {
  static __device__ __forceinline__ float value(float v) { return v; }
  static __device__ __forceinline__ float round(float f) { return f; }
};
template <>
struct TrimVal<MedBF16> {
  static __device__ __forceinline__ float value(float v) { return v; }  // bf16 widened exactly
  static __device__ __forceinline__ uint16_t round(float f) {
    const __bf16 b = static_cast<__bf16>(f);  // v_cvt_pk_bf16_f32: RNE
    return __builtin_bit_cast(uint16_t, b);
  }
};
template <>
struct TrimVal<MedF16> {
  // the selection value is an order key: back to the f16 bits, then v_cvt_f32_f16
  static __device__ __forceinline__ float value(float v) {
    return static_cast<float>(__builtin_bit_cast(_Float16, MedF16::narrow(v)));
  }
  static __device__ __forceinline__ uint16_t round(float f) {
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));  // v_cvt_f16_f32: RNE
  }
};

template <class E>
using raw_bits_t = std::conditional_t<sizeof(typename E::S) == 4, uint32_t, uint16_t>;
template <class E>
constexpr typename E::S trim_pos_inf() {
  return __builtin_bit_cast(typename E::S, static_cast<raw_bits_t<E>>(E::kPosInf));
}

// The nearest-to-median kernels (nearmedian.hip, nearmedian_wide.hip): the
// distance d(x) of a sorted value from the median m.  x - m is NaN only for
// equal infinities, which fmaxf turns into the 0 of x == m; every other
// x == m gives 0 by itself
__device__ __forceinline__ float near_dist(float x, float m) { return fmaxf(__builtin_fabsf(x - m), 0.f); }

// Row base of client row p for a launch starting at column col0 (> 0 only
// past 2^30 columns): an opaque SGPR pair, so the loads keep the
// SGPR-base + 32-bit VGPR-offset form (left visible, the compiler folds col0
// into a per-lane 64-bit address: 2.2x slower at K = 128).
template <class T>
__device__ __forceinline__ const char __attribute__((address_space(1)))* row_base(const T* p, int64_t col0) {
  uint64_t b = reinterpret_cast<uint64_t>(p) + uint64_t(col0) * sizeof(T);
  asm("" : "+s"(b));
  return reinterpret_cast<const char __attribute__((address_space(1)))*>(b);
}

// The raw value of slot c for the lane at byte offset boff of the rows: the
// one load form of median_kernel, trimmed_mean_kernel and
// nearmedian_mean_kernel.  The kernel's unrolled loop over the slots, its
// widening and its NaN handling stay with the kernel, and so does the
//   if (c % 16 == 0 && c) __builtin_amdgcn_sched_barrier(0);
// in front of each call, which keeps at most 16 row pointers live in SGPRs:
// without it the scheduler hoists all KMAX pointer loads to the top and
// spills them.
//   - FULL (K == KMAX): the row pointer is src[c], a scalar load.
//   - Padded tiers read it from tab, the block's LDS table of KMAX slot
//     pointers (pads point at a ±inf constant), at a wave-uniform address and
//     move it to SGPRs.  readfirstlane returns int: each half goes through
//     uint32_t, or a low word with its top bit set sign-extends over the high
//     word.
//   - A padded slot (c >= K) reads the pad constant: its row pointer is the
//     pad and its lane offset is 0, so the load itself yields the pad and
//     nothing per slot waits for a load.
//   - OFF (launches past 2^30 columns): a live row's base is row_base(p, col0),
//     the opaque SGPR pair that keeps the SGPR-base + 32-bit-offset form; a
//     pad is read at its own address.
// src carries no __restrict__ here (the kernels' own parameter does): with it
// the K = 8 full fp32 median kernel allocated its SGPRs differently (26 -> 28);
// without it every kernel's assembly is what the written-out block gave.
template <bool FULL, bool OFF, class S, int NT>
__device__ __forceinline__ S load_slot(const S* const* src, const S* const (&tab)[NT], int c, int K, uint32_t boff,
                                       int64_t col0) {
  const bool live = FULL || c < K;
  const S* p;
  if constexpr (FULL) {
    p = src[c];
  } else {
    const uint64_t t = reinterpret_cast<uint64_t>(tab[c]);
    const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(t >> 32))));
    const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(t))));
    p = reinterpret_cast<const S*>((uint64_t(hi) << 32) | uint64_t(lo));
  }
  const char __attribute__((address_space(1)))* row;
  if constexpr (OFF)
    row = live ? row_base(p, col0) : reinterpret_cast<const char __attribute__((address_space(1)))*>(as_global(p));
  else
    row = reinterpret_cast<const char __attribute__((address_space(1)))*>(as_global(p));
  return cols_load(reinterpret_cast<const S __attribute__((address_space(1)))*>(row + (live ? boff : 0u)));
}

// ---------------------------------------------------------------------------
// Host side of the one-lane-per-column kernels.

// Columns per launch: a lane's byte offset from the (wave-uniform) row base +
// col0 fits in 32 bits.  Even, so the 4-byte column pairs of the packed
// 16-bit kernel stay aligned at every chunk start.
// The environment variable FEDAGG_COLS_CHUNK (cols_chunk below) replaces it
// for a call: it exists for the tests, which run the kernels of the later
// launches on a few hundred columns.
constexpr int64_t kColsChunk = int64_t(1) << 30;

// The columns per launch of this call: kColsChunk, or FEDAGG_COLS_CHUNK where
// it is set and not empty.  Read on every call (as FEDAGG_PACK_SPAWN is in
// fedagg.hip), so one process can switch it.  The whole string must be a
// decimal integer, even (the packed kernel's column pairs) and in
// [2, kColsChunk] (the 32-bit byte offset); anything else is FEDAGG_EINVAL,
// never a silent default.
inline int cols_chunk(const char* what, int64_t& chunk) {
  chunk = kColsChunk;
  const char* s = getenv("FEDAGG_COLS_CHUNK");
  if (!s || !*s) return FEDAGG_OK;
  int64_t v = 0;
  bool ok = true;
  for (const char* p = s; *p && ok; ++p) {
    ok = *p >= '0' && *p <= '9' && v <= kColsChunk;  // v stays far below overflow
    if (ok) v = v * 10 + (*p - '0');
  }
  if (!ok || v < 2 || v > kColsChunk || (v & 1))
    return set_error(FEDAGG_EINVAL, std::string(what) + ": FEDAGG_COLS_CHUNK must be an even decimal integer in [2, " +
                                        std::to_string(kColsChunk) + "] (got \"" + s + "\")");
  chunk = v;
  return FEDAGG_OK;
}

// Columns [0, N) in launches of at most cols_chunk() columns, each thread
// taking `per_thread` adjacent columns: kernel(src, K, n, mid..., out + c0, c0)
// for every chunk start c0.  The first chunk runs `full` when K is the tier's
// KMAX and `padded` otherwise; the later chunks (past 2^30 columns) run
// `padded_off`, the padded kernel (correct for K == KMAX too) with the row
// offset.
template <class Kern, class S, class... Mid>
int launch_col_chunks(const char* what, Kern full, Kern padded, Kern padded_off, bool is_full, int BS, int per_thread,
                      hipStream_t st, const S* const* src, int K, int64_t N, S* out, Mid... mid) {
  int64_t chunk;
  if (int rc = cols_chunk(what, chunk)) return rc;  // before the first launch
  for (int64_t c0 = 0; c0 < N; c0 += chunk) {
    const int64_t n = N - c0 < chunk ? N - c0 : chunk;
    const int64_t grid = ((n + per_thread - 1) / per_thread + BS - 1) / BS;
    const Kern kernel = c0 ? padded_off : is_full ? full : padded;
    hipLaunchKernelGGL(kernel, dim3(unsigned(grid)), dim3(BS), 0, st, src, K, n, mid..., out + c0, c0);
  }
  return check_launch(what);
}

// The tiers of the kernels' KMAX.  with_tier calls f(KMAX, KMIN) as
// std::integral_constant<int, ..> values for the smallest tier holding K
// (the last for anything above it: the callers bound K); KMIN is the smallest
// K the tier is chosen for, the previous tier + 1.
constexpr int kTiers[] = {8, 16, 24, 32, 48, 64, 96, 128};
constexpr int kNumTiers = int(sizeof(kTiers) / sizeof(kTiers[0]));

template <int I = 0, class F>
int with_tier(int K, F f) {
  constexpr int KMAX = kTiers[I], KMIN = I ? kTiers[I ? I - 1 : 0] + 1 : 1;
  // this tier's call stands before the next tier's: the kernels are emitted in ascending tier order
  if (K <= KMAX || I + 1 == kNumTiers)
    return f(std::integral_constant<int, KMAX>{}, std::integral_constant<int, KMIN>{});
  if constexpr (I + 1 < kNumTiers) return with_tier<I + 1>(K, f);
  __builtin_unreachable();
}

}  // namespace
