// What the two units that READ the KV cache on the matrix cores — block_attention_decode.hip (one wave per list entry) and
// block_attention_prefill.hip (workgroup tiles staged in LDS) — say about a walk over it, said once: the cache
// element as a compile-time form (T itself or e4m3fn bytes widened exactly), the three forms of tile addressing and the table
// entries of a tile of a paged cache — and, in its host section, what their two entry functions say alike about a reading call
// (§3.31): its sizes, its operands, the fields their Args share, the head-size and the cache-form dispatch.  Not installed.
// Everything here has internal linkage (an anonymous namespace per including unit).
#ifndef MI_BLOCK_ATTENTION_CACHE_DEVICE_H_
#define MI_BLOCK_ATTENTION_CACHE_DEVICE_H_

#include <type_traits>

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

// ---- the host side: what decode_entry and prefill_entry say alike about a reading call ----------------------
// What every reading entry takes, in the header's words.  page == 0: the contiguous cache, `outerK` / `outerV` its batch
// strides and no table; page > 0: a pool of `pages` pages of `page` keys, `outerK` / `outerV` its page strides, Smax = the
// table's logical pages · page.  `scales`: looked at by the fp8 entries only (k and v are e4m3fn bytes, their strides multiples
// of 16).  q, new_lens, chunk / split and the workspace are each entry's own.
struct ReadCall {
  const int32_t *rowptr, *col;
  int64_t nnz;
  int32_t layouts, items, heads, T, Smax, D;
  const void* k;
  int64_t ldk, headK, outerK;
  const void* v;
  int64_t ldv, headV, outerV;
  const int32_t* k_lens;
  int32_t lens_count, group;
  float scale;
  uint16_t* out;
  int64_t ldo, strideO;
  float* lse;
  const int32_t* table = nullptr;
  int64_t table_ld = 0;
  int32_t pages = 0, page = 0;
  Scales scales = Scales();
};

// … as an entry gathers it from its parameters, which the header names alike for all 32 (the four list entries over an fp8
// cache, §3.32, included): the list (a layout's, or the caller's lists: §3.29), then what the paged entries add (MI_READ_PAGED) and the scales of the fp8 ones (MI_READ_FP8).  (k, batchK and v,
// batchV stand for k_pages, pageK and v_pages, pageV of the header.)
#define MI_READ_CALL(ROWPTR, COL, NNZ, LAYOUTS, ...)                                                                         \
  ReadCall{ROWPTR, COL, NNZ, LAYOUTS, items, heads, T, Smax, D, k, ldk, headK, batchK, v, ldv, headV, batchV, k_lens, lens_count, \
           group, scale, out, ldo, strideO, lse, __VA_ARGS__}
#define MI_READ_PAGED block_table, table_ld, pages, page
#define MI_READ_FP8 Scales{k_scale, k_scale_count, v_scale, v_scale_count}
// … and by token, for the entry tables of the decode and the prefill unit, whose lines say FLAT or PAGED and FP8 false or true:
// what MI_READ_CALL takes behind the list, the cache's element type, and the paged entries' guard — a page of 0 keys would
// name the contiguous form, so it is refused here like every page that is no power of two ≥ 16.
#define MI_READ_TABLE_FLAT nullptr, 0, 0, 0
#define MI_READ_TABLE_PAGED MI_READ_PAGED
#define MI_READ_GUARD_FLAT
#define MI_READ_GUARD_PAGED page < 16 ? MI_EINVAL:
#define MI_READ_SCALES_false Scales()
#define MI_READ_SCALES_true MI_READ_FP8
#define MI_READ_CACHE_false uint16_t
#define MI_READ_CACHE_true uint8_t

// The checks come in two halves, as the cache's own do, because every entry answers MI_OK for an empty call between them —
// and refuses sizes of its own (the decode grid's items and T) there.  The sizes: MI_EINVAL, MI_ERANGE for a layout beyond
// int32 indices, or MI_OK to go on.
int read_sizes_status(bool fp8, const ReadCall& r) {
  if (!cache_form_ok(fp8, r.scales, r.heads, r.Smax, r.pages, r.page)) return MI_EINVAL;
  if (r.group < 1 || !takes_width(r.D)) return MI_EINVAL;
  if (r.nnz < 0 || r.layouts < 0 || r.items < 0 || r.heads < 0 || r.T < 0 || r.Smax < 0 || r.Smax % kB != 0) return MI_EINVAL;
  return r.nnz > 0x7fffffffLL ? MI_ERANGE : MI_OK;
}

bool read_is_empty(const ReadCall& r) { return r.items == 0 || r.T == 0; }

// The operands of a call that is not empty; `listed`: the caller's lists stand in col and there is no rowptr (§3.29).  A cache
// that no list entry can reach — no entry, no row, an empty pool: every entry of the table is invalid — is not looked at.
bool read_operands_ok(bool fp8, const ReadCall& r, bool listed = false) {
  if (r.layouts == 0 || r.heads == 0 || r.items % r.heads != 0 || r.lens_count < 1 || r.items % r.lens_count != 0) return false;
  if ((!listed && !r.rowptr) || (r.nnz > 0 && !r.col) || !r.k_lens || !aligned4(r.k_lens)) return false;
  if (!r.lse || !aligned4(r.lse)) return false;
  if (!r.out || !mi::aligned16(r.out) || r.ldo < r.D || !stride_ok(r.ldo) || !stride_ok(r.strideO)) return false;
  const bool reads = r.nnz > 0 && r.Smax > 0 && (r.page == 0 || r.pages > 0);
  return cache_operands_ok(fp8, reads, r.Smax, r.D, r.k, r.ldk, r.headK, r.outerK, r.v, r.ldv, r.headV, r.outerV, r.table, r.table_ld,
                           r.page);
}

// the fields that the two units' Args name alike, into a zeroed A: the 2-byte entries leave k_scale / v_scale null, which the
// kernels read as 1
template <class A>
void fill_read_args(A& a, bool fp8, const ReadCall& r) {
  a.rowptr = r.rowptr, a.col = r.col, a.nnz = r.nnz, a.layouts = r.layouts, a.blocks = r.Smax / kB, a.heads = r.heads;
  a.group = r.group, a.T = r.T, a.smax = r.Smax;
  a.k = r.k, a.ldk = r.ldk, a.headK = r.headK, a.v = r.v, a.ldv = r.ldv, a.headV = r.headV;
  if (r.page != 0 && r.Smax > 0) {  // (Smax == 0: no list has an entry, the contiguous form stores the zero rows)
    a.table = r.table, a.table_ld = r.table_ld, a.pages = r.pages, a.page_shift = __builtin_ctz((unsigned)r.page);
    a.pageK = r.outerK, a.pageV = r.outerV;
  } else {
    a.batchK = r.outerK, a.batchV = r.outerV;
  }
  a.k_lens = r.k_lens, a.lens_div = r.items / r.lens_count, a.scale = r.scale;
  a.out = r.out, a.ldo = r.ldo, a.strideO = r.strideO, a.lse = r.lse;
  if (fp8) a.k_scale = r.scales.k, a.k_scale_count = r.scales.k_count, a.v_scale = r.scales.v, a.v_scale_count = r.scales.v_count;
}

// f(std::integral_constant<int, D>()) for the head size (takes_width(D) holds) …
template <class F>
int with_width(int32_t D, F&& f) {
  switch (D) {
    case 32: return f(std::integral_constant<int, 32>());
    case 64: return f(std::integral_constant<int, 64>());
    case 96: return f(std::integral_constant<int, 96>());
    default: return f(std::integral_constant<int, 128>());
  }
}

// … and f(std::integral_constant<int, FORM>()) for the tile addressing of filled Args
template <class A, class F>
int with_form(const A& a, F&& f) {
  if (!a.table) return f(std::integral_constant<int, kContiguous>());
  if (a.page_shift >= 6) return f(std::integral_constant<int, kPaged>());
  return f(std::integral_constant<int, kPagedSmall>());
}

}  // namespace

#endif  // MI_BLOCK_ATTENTION_CACHE_DEVICE_H_
