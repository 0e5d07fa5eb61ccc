// sortnet.h — what the one-lane-per-column selection kernels share: the
// compile-time pairwise sorting network, the element types (fp32, bf16, f16
// as fp32 "selection values") and the row loads.  Included by median.hip and
// trimmed.hip; everything is internal to the including translation unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

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

}  // namespace
