// What the four units of the KV-cache family — block_attention_decode.hip and block_attention_prefill.hip (the read side),
// kv_append.hip and rope_kv_append.hip (the write side) — and the selection's two, kv_block_bounds.hip and block_select.hip
//  — say about the cache itself, said once: the scales of an fp8 cache,
// the bytes an fp8 cache receives, and what every C entry refuses about the cache operands.  Not installed.  Everything here
// has internal linkage (an anonymous namespace per including unit).
#ifndef MI_KV_CACHE_DEVICE_H_
#define MI_KV_CACHE_DEVICE_H_

#include "lowp_device.h"

namespace {

// ---- the scales of an fp8 cache: null is 1, a count of 1 one scale for all heads, else one per k / v head -------------------
struct Scales {
  const float* k = nullptr;
  int k_count = 1;
  const float* v = nullptr;
  int v_count = 1;
};

__device__ __forceinline__ float head_scale(const float* s, int count, int h) { return s ? s[count == 1 ? 0 : h] : 1.f; }

// ---- the bytes of an fp8 cache (a bit-for-bit contract) ------------------------------------------------------
// The IEEE float32 quotient x / s from r = fl64(1 / s), taken once per thread: float(double(x) · r).  It IS the correctly
// rounded quotient: the double product is within 2⁻⁵² (relative) of x / s, while a quotient of two 24-bit numbers that is not
// itself a float lies at least 2⁻⁴⁹ (relative) from every midpoint of two floats (x − s · m is a non-zero multiple of the last
// place of a 24 × 25-bit product), so the one rounding to float falls where the division's would.  ±0, ±inf and NaN in x or s
// come out as the division gives them (0 · inf = NaN = 0 / 0); a quotient below 2⁻¹²⁶ may differ in its last subnormal bits,
// which is far below 2⁻¹⁰, where every value is the byte ±0.  Three instructions per element where the division takes eleven.
__device__ __forceinline__ float quotient(float x, double r) { return (float)((double)x * r); }

// two floats as two e4m3fn bytes in the low half of the result: quotient, clamp, one rounding; a NaN quotient → 0x7F | sign
__device__ __forceinline__ unsigned fp8x2(float a, float b, double r) {
  const float qa = quotient(a, r), qb = quotient(b, r);
  const float ca = fminf(fmaxf(qa, -448.f), 448.f), cb = fminf(fmaxf(qb, -448.f), 448.f);
  const unsigned w = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(ca, cb, 0, false) & 0xffffu;
  return w | (qa != qa ? 0x7fu : 0u) | (qb != qb ? 0x7f00u : 0u);
}

// the 8 elements of one 16-byte load as 8 bytes
template <class T>
__device__ __forceinline__ uint2 quantise(uint4 x, double s) {
  uint2 r;
  r.x = fp8x2(T::lo(x.x), T::hi(x.x), s) | (fp8x2(T::lo(x.y), T::hi(x.y), s) << 16);
  r.y = fp8x2(T::lo(x.z), T::hi(x.z), s) | (fp8x2(T::lo(x.w), T::hi(x.w), s) << 16);
  return r;
}

// 8 elements of a source row into the cache at element offset `off`: a bit copy, or FP8 the bytes above (s = 1 / scale; T,
// the source's type, is looked at by the fp8 form only)
template <class T, bool FP8>
__device__ __forceinline__ void store_cache(void* base, long off, uint4 x, double s) {
  if constexpr (FP8)
    *reinterpret_cast<uint2*>(static_cast<uint8_t*>(base) + off) = quantise<T>(x, s);
  else
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(base) + off) = x;
}

// ---- what the entries refuse about the cache, ahead of the first HIP call ----------------------------------------------------
bool takes_width(int32_t D) { return D == 32 || D == 64 || D == 96 || D == 128; }

// a stride in elements: a multiple of 16 bytes — 8 two-byte elements, 16 e4m3fn bytes
bool stride_ok(int64_t s, int64_t unit = 8) { return s >= 0 && s % unit == 0; }

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

constexpr long kSpread = 256;  // an append of fewer workgroups of 256 threads than this: workgroups of 64 (the CUs of the chip)

// The cache checks come in two halves, because every entry answers MI_OK for an empty call (items == 0, T == 0) between them:
// the form is refused even then, a pointer is not looked at.
// The form: the scale counts and alignment of an fp8 cache; page == 0 is the contiguous cache, else a pool of `pages` pages
// of `page` rows — a power of two ≥ 16 that divides Smax, the table's logical pages · page.
bool cache_form_ok(bool fp8, const Scales& sc, int32_t heads, int32_t Smax, int32_t pages, int32_t page) {
  if (fp8 && ((sc.k_count != 1 && sc.k_count != heads) || (sc.v_count != 1 && sc.v_count != heads))) return false;
  if (fp8 && (!aligned4(sc.k) || !aligned4(sc.v))) return false;
  return page == 0 || (page >= 16 && (page & (page - 1)) == 0 && pages >= 0 && Smax % page == 0);
}

// The operands: the table of a paged cache with rows, and — where the call `touches` the cache at all, which the reading and
// the writing entries decide differently — k and v: 16-byte aligned, ld ≥ D, every stride a multiple of
// 16 bytes of cache elements.
bool cache_operands_ok(bool fp8, bool touches, int32_t Smax, int32_t D, const void* k, int64_t ldk, int64_t headK, int64_t outerK,
                       const void* v, int64_t ldv, int64_t headV, int64_t outerV, const int32_t* table, int64_t table_ld,
                       int32_t page) {
  const int64_t unit = fp8 ? 16 : 8;  // cache elements in 16 bytes
  if (page != 0 && Smax > 0 && (!table || !aligned4(table) || table_ld < Smax / page)) return false;
  if (!touches) return true;
  if (!k || !mi::aligned16(k) || ldk < D || !stride_ok(ldk, unit) || !stride_ok(headK, unit) || !stride_ok(outerK, unit)) return false;
  return v && mi::aligned16(v) && ldv >= D && stride_ok(ldv, unit) && stride_ok(headV, unit) && stride_ok(outerV, unit);
}

}  // namespace

#endif  // MI_KV_CACHE_DEVICE_H_
