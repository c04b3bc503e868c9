// The two 16-bit element types, said once for every bfloat16 / float16 translation unit: Bf16 / F16 with their exact widening
// and their one rounding, up<T>, pack2<T>, the element scheme Fp32 / Lowp<T> of the units that are one template over fp32 and
// the 16-bit types, the 4-element row pieces load4 / store4, and the host's aligned8 / odd.  Included by the CSR units
// (csr_lowp.hip; csr_reduce.hip and csr_reduce_lowp.hip through csr_reduce_device.h; csr_softmax.hip and csr_attention.hip,
// through csr_softmax_device.h too), by
// mfma_device.h for the five matrix-core units (gemm_lowp.hip, bsr_mm.hip, bsr_linear.hip, block_attention.hip,
// block_attention_decode.hip) and by kv_cache_device.h for the KV-cache family (kv_append.hip, rope_kv_append.hip).  Not
// installed.  Everything here has internal linkage (an anonymous namespace per including unit).
#ifndef MI_LOWP_DEVICE_H_
#define MI_LOWP_DEVICE_H_

#include "mi_common.h"

namespace {

using mi::f32x4;

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// The two element types: exact widening of a stored 16-bit pattern, round-to-nearest-even narrowing at the store
// (gfx950: v_cvt_pk_bf16_f32 / v_cvt_f16_f32; NaN stays NaN, overflow goes to ±inf — DESIGN.md §3.8).
struct Bf16 {
  static __device__ __forceinline__ float lo(unsigned w) { return __uint_as_float(w << 16); }
  static __device__ __forceinline__ float hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
  static __device__ __forceinline__ unsigned short down(float f) { return __builtin_bit_cast(unsigned short, static_cast<__bf16>(f)); }
};
struct F16 {
  static __device__ __forceinline__ float lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
  static __device__ __forceinline__ float hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
  static __device__ __forceinline__ unsigned short down(float f) { return __builtin_bit_cast(unsigned short, static_cast<_Float16>(f)); }
};

template <class T>
__device__ __forceinline__ float up(unsigned short h) { return T::lo(h); }

// The element scheme of the units that cover fp32, bf16 and fp16 with one `template <class E>` (csr_softmax.hip,
// csr_attention.hip, the reductions of csr_reduce_device.h): E::S the stored type, E::up its exact widening, E::down(f) the
// one rounding at the store.
// down(f, z): the stored form of the fp32 result f.  z is a zero the compiler cannot see (the kernels derive it from an
// argument): for fp16 hipcc otherwise fuses the multiply that produces f with the narrowing into ONE mixed-precision fma
// (v_fma_mixlo_f16) — a single rounding of the exact product, and a +0 addend that turns −0 into +0 — which is not
// rne_T(fl32(product)), the contract.  Passing f's bits through `xor z` keeps the two roundings apart.
struct Fp32 {
  typedef float S;
  static __device__ __forceinline__ float up(float v) { return v; }
  static __device__ __forceinline__ float down(float v) { return v; }
  static __device__ __forceinline__ float down(float v, unsigned) { return v; }
};
template <class T>
struct Lowp {
  typedef unsigned short S;
  static __device__ __forceinline__ float up(unsigned short h) { return T::lo(h); }
  static __device__ __forceinline__ unsigned short down(float f) { return T::down(f); }
  static __device__ __forceinline__ unsigned short down(float f, unsigned z) {
    return T::down(__uint_as_float(__float_as_uint(f) ^ z));
  }
};

template <class T>
__device__ __forceinline__ unsigned pack2(float a, float b) { return (unsigned)T::down(a) | ((unsigned)T::down(b) << 16); }

// four consecutive elements: one 8-byte load (VEC: 8-byte aligned, all four inside the row) or four 2-byte loads
// guarded by j < N (zeros beyond: never part of a stored chain)
template <class T, bool VEC>
__device__ __forceinline__ f32x4 load4(const unsigned short* p, int j, int N) {
  if constexpr (VEC) {
    const u32x2 w = *reinterpret_cast<const u32x2*>(p);
    return f32x4{T::lo(w.x), T::hi(w.x), T::lo(w.y), T::hi(w.y)};
  } else {
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (j + 0 < N) r.x = up<T>(p[0]);
    if (j + 1 < N) r.y = up<T>(p[1]);
    if (j + 2 < N) r.z = up<T>(p[2]);
    if (j + 3 < N) r.w = up<T>(p[3]);
    return r;
  }
}

template <class T, bool VEC>
__device__ __forceinline__ void store4(unsigned short* p, int j, int N, f32x4 v) {
  if constexpr (VEC) {
    const u32x2 w = {pack2<T>(v.x, v.y), pack2<T>(v.z, v.w)};
    __builtin_nontemporal_store(w, reinterpret_cast<u32x2*>(p));
  } else {
    if (j + 0 < N) p[0] = T::down(v.x);
    if (j + 1 < N) p[1] = T::down(v.y);
    if (j + 2 < N) p[2] = T::down(v.z);
    if (j + 3 < N) p[3] = T::down(v.w);
  }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool odd(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 1u) != 0; }  // a 2-byte element cannot start there

}  // namespace

#endif  // MI_LOWP_DEVICE_H_
