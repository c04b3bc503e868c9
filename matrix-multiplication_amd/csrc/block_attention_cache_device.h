// What the two units that READ the KV cache on the matrix cores — block_attention_decode.hip (one wave per list entry) and
// block_attention_prefill.hip (workgroup tiles staged in LDS) — say about a walk over it, said once: the cache
// element as a compile-time form (T itself or e4m3fn bytes widened exactly), the three forms of tile addressing and the table
// entries of a tile of a paged cache.  Not installed.  Everything here has internal linkage (an anonymous namespace per
// including unit).
#ifndef MI_BLOCK_ATTENTION_CACHE_DEVICE_H_
#define MI_BLOCK_ATTENTION_CACHE_DEVICE_H_

#include "block_attention_device.h"
#include "kv_cache_device.h"

namespace {

// The cache element as a compile-time form of the walk: Fp8<T> names q's and out's type T over a cache of e4m3fn bytes
template <class T>
struct Fp8 {};
template <class TC>
struct Operand {
  typedef TC type;
  static constexpr bool fp8 = false;
};
template <class T>
struct Operand<Fp8<T>> {
  typedef T type;
  static constexpr bool fp8 = true;
};

// … and what a lane loads for its 8 consecutive elements
template <bool FP8>
struct Cache {
  typedef uint16_t elem;
  typedef uint4 frag;
};
template <>
struct Cache<true> {
  typedef uint8_t elem;
  typedef uint2 frag;
};

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// two e4m3fn (OCP) bytes of w — the low pair, or with HI the high pair — as two T, in their order: exact
template <class T, bool HI>
__device__ __forceinline__ unsigned widen2(unsigned w);
template <>
__device__ __forceinline__ unsigned widen2<Bf16, false>(unsigned w) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ unsigned widen2<Bf16, true>(unsigned w) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true));
}
template <>
__device__ __forceinline__ unsigned widen2<F16, false>(unsigned w) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false));
}
template <>
__device__ __forceinline__ unsigned widen2<F16, true>(unsigned w) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true));
}

// a lane's 8 elements as the 16 bytes of T the MFMA takes: as they are, or 8 e4m3fn bytes widened
template <class T>
__device__ __forceinline__ uint4 widen(uint4 x) { return x; }
template <class T>
__device__ __forceinline__ uint4 widen(uint2 x) {
  return uint4{widen2<T, false>(x.x), widen2<T, true>(x.x), widen2<T, false>(x.y), widen2<T, true>(x.y)};
}

template <class F> __device__ __forceinline__ F zero_frag();
template <> __device__ __forceinline__ uint4 zero_frag<uint4>() { return uint4{0u, 0u, 0u, 0u}; }
template <> __device__ __forceinline__ uint2 zero_frag<uint2>() { return uint2{0u, 0u}; }

// How the walk finds the 64 keys of a list entry: a compile-time form of the kernel, as LENS is in block_attention.hip
constexpr int kContiguous = 0;  // one [Smax][D] run per k / v item behind fixed strides
constexpr int kPaged = 1;       // a pool of pages ≥ 64 keys: the tile lies inside one page — one table entry per tile
constexpr int kPagedSmall = 2;  // pages of 16 or 32 keys: the tile spans 64 / page whole pages — one entry per page

// The table entries of the logical pages of tile J of a paged cache, one per 16-row fragment f of the tile (fragment f lies
// inside logical page (64J + 16f) >> page_shift because 16 divides the page): with pages ≥ 64 keys all four are the tile's
// one page.  J < Smax / 64, so the index stays below Smax / page ≤ table_ld.
template <int FORM>
__device__ __forceinline__ void read_pages(int (&e)[4], const int32_t* trow, int J, int shift) {
  if constexpr (FORM == kPaged) {
    e[0] = e[1] = e[2] = e[3] = trow[(J * kB) >> shift];
  } else {
#pragma unroll
    for (int f = 0; f < 4; ++f) e[f] = trow[(J * kB + 16 * f) >> shift];
  }
}

// bit f: fragment f of the tile lies in a page of the pool; the rows of the others are invisible and never loaded
__device__ __forceinline__ unsigned valid_pages(const int (&e)[4], int pages) {
  unsigned ok = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) ok |= ((unsigned)e[f] < (unsigned)pages ? 1u : 0u) << f;
  return ok;
}

}  // namespace

#endif  // MI_BLOCK_ATTENTION_CACHE_DEVICE_H_
