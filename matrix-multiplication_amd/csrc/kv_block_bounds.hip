// Per-block key bounds of a key cache: for every 64-key block of every k / v item the elementwise minimum and maximum of the
// keys it holds — what block_select.hip scores a query against.  The cache is the one of
// block_attention_decode.hip, contiguous or paged, in its two 2-byte forms or — the *_fp8 entries, DESIGN.md §3.32 — of e4m3fn
// bytes, whose bounds are kept in bfloat16 or float16.
//
// What it writes (contract of include/mi_spmm.h, mi_kv_block_bounds{,_paged}{,_fp8}_{bf16,f16}):
//  * bounds [items][Smax / 64][2][D] in the cache's type (fp8: the entry's): bounds[c][J][0][d] = min, bounds[c][J][1][d] = max
//    of k[c][j][d] over the SEEN keys j of block J: 64J ≤ j < min(64J + 64, k_len), and, paged, the table entry of j's logical
//    page in [0, pages).  k_len is clamped to [0, Smax].  A block with no seen key is NOT WRITTEN; neither is anything else.
//  * last = 0 refreshes every block with a seen key; last = T ≥ 1 only the blocks that hold a position of
//    [k_len − T, k_len) — the refresh after an append of T tokens.
//  * min and max are exact and a function of the seen keys alone: the 16-bit patterns are compared as ordered integers (sign
//    and magnitude turned into one unsigned order, in which −0 < +0), so neither the order of the rows, nor the launch, nor
//    the form of the cache can show in the bits, and no widening is needed: ONE kernel serves bfloat16 and float16.  A NaN
//    pattern sorts beyond ±inf on its sign's side: the result with NaN keys is unspecified, and nothing faults.
//  * An fp8 cache: the BYTES are compared in their own total order (the same turn of sign and magnitude on 8 bits) and only the
//    D minima and D maxima are widened, at the store, to the bounds' type — exact: every finite e4m3fn code is a bfloat16 and a
//    float16, and the widening is strictly monotone from the one order into the other, −0 < +0 kept, so minimum and maximum
//    commute with it: the bits of the 2-byte kernel on the widened cache.  The scales of the cache are not looked at: positive
//    per-head factors change neither a minimum nor the ranking inside a head.  NaN codes (0x7f, 0xff): unspecified, no fault.
//  * Nothing outside is read: rows at or beyond k_len, the gaps between the rows of a strided cache and the pages behind an
//    out-of-range table entry are never loaded.
//
// Kernel: grid (blocks refreshed, items), 256 threads; a thread owns 8 consecutive elements of the rows r, r + 256 / (D/8), …
// of its block — one 16-byte global load per row, 8 bytes of an fp8 cache —, the partial minima and maxima of the threads of
// one column group meet in LDS and thread d < D folds column d over them.  No atomics, no read-back: graph-capturable.
#include "block_attention_cache_device.h"  // kB, the keys of a block: the decode walk's tile; widen2: e4m3fn bytes as T, exact

namespace {

struct Args {
  int heads, blocks, last;  // k / v item c is head c % heads of batch item c / heads; blocks = Smax / 64; last: 0 = all
  long smax;
  const void* k;  // key j of item c: k + (c / heads) · outerK + (c % heads) · headK + j · ldk; paged:
                  // k + table[(c / heads) · table_ld + (j >> page_shift)] · outerK + (c % heads) · headK + (j & (page − 1)) · ldk
  long ldk, headK, outerK;  // (in cache elements: 2-byte patterns, or e4m3fn bytes)
  const int32_t* k_lens;  // [items / lens_div], clamped to [0, Smax] where read
  int lens_div;
  const int32_t* table;  // [items / heads][table_ld]; an entry outside [0, pages) hides the keys of its logical page
  long table_ld;
  int pages, page_shift;
  uint16_t* bounds;  // [items][blocks][2][D]
};

// a 16-bit floating-point pattern as an unsigned integer of the same order (−max … −0 < +0 … +max), and back
__device__ __forceinline__ unsigned ordered(unsigned h) { return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u); }
__device__ __forceinline__ unsigned pattern(unsigned o) { return (o & 0x8000u) ? (o & 0x7fffu) : (~o & 0xffffu); }

// … of e4m3fn bytes: the same turn on 8 bits
__device__ __forceinline__ unsigned ordered8(unsigned b) { return (b & 0x80u) ? (~b & 0xffu) : (b | 0x80u); }
__device__ __forceinline__ unsigned pattern8(unsigned o) { return (o & 0x80u) ? (o & 0x7fu) : (~o & 0xffu); }

// the block J this workgroup refreshes for its item blockIdx.y and the keys of it below k_len; false: no key, nothing is written
__device__ __forceinline__ bool own_block(const Args& a, int& J, int& rows) {
  int klen = a.k_lens[blockIdx.y / a.lens_div];
  klen = klen < 0 ? 0 : klen > a.smax ? (int)a.smax : klen;
  // the first block of the refresh: the one of position k_len − last (0: the whole cache)
  const int from = a.last > 0 && klen > a.last ? (klen - a.last) / kB : 0;
  J = from + (int)blockIdx.x;
  rows = klen - J * kB < kB ? klen - J * kB : kB;
  return J < a.blocks && rows > 0;
}

// row j of k / v head h of batch item b in a cache of elements E; null: an invisible key, behind a table entry outside the pool
template <bool PAGED, class E>
__device__ __forceinline__ const E* key_row(const Args& a, int b, int h, long j) {
  const E* k = static_cast<const E*>(a.k);
  if constexpr (PAGED) {
    const int e = a.table[(long)b * a.table_ld + (j >> a.page_shift)];
    if ((unsigned)e >= (unsigned)a.pages) return nullptr;
    return k + (long)e * a.outerK + (long)h * a.headK + (j & ((1L << a.page_shift) - 1)) * a.ldk;
  } else {
    return k + (long)b * a.outerK + (long)h * a.headK + j * a.ldk;
  }
}

template <int D, bool PAGED>
__global__ __launch_bounds__(256) void kv_block_bounds_kernel(Args a) {
  constexpr int DV = D / 8;      // threads of a row
  constexpr int RP = 256 / DV;   // rows of a pass (D = 96: 21, and 4 threads idle)
  __shared__ unsigned short lo_s[RP][D], hi_s[RP][D];
  const int tid = threadIdx.x, c = blockIdx.y;
  const int b = c / a.heads, h = c - b * a.heads;
  // (own_block and key_row, written out: with the calls these eight kernels' register counts moved by one to two)
  int klen = a.k_lens[c / a.lens_div];
  klen = klen < 0 ? 0 : klen > a.smax ? (int)a.smax : klen;
  // the first block of the refresh: the one of position k_len − last (0: the whole cache)
  const int from = a.last > 0 && klen > a.last ? (klen - a.last) / kB : 0;
  const int J = from + (int)blockIdx.x;
  const int rows = klen - J * kB < kB ? klen - J * kB : kB;  // keys of this block below k_len
  if (J >= a.blocks || rows <= 0) return;  // no key: not written
  const int r0 = tid / DV, g = tid - r0 * DV;
  unsigned mn[8], mx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mn[e] = 0xffffu, mx[e] = 0u;
  if (r0 < RP) {
    for (int r = r0; r < rows; r += RP) {
      const long j = (long)J * kB + r;
      const uint16_t* row;
      if constexpr (PAGED) {
        const int e = a.table[(long)b * a.table_ld + (j >> a.page_shift)];
        if ((unsigned)e >= (unsigned)a.pages) continue;  // an invisible key
        row = static_cast<const uint16_t*>(a.k) + (long)e * a.outerK + (long)h * a.headK + (j & ((1L << a.page_shift) - 1)) * a.ldk;
      } else {
        row = static_cast<const uint16_t*>(a.k) + (long)b * a.outerK + (long)h * a.headK + j * a.ldk;
      }
      const uint4 x = *reinterpret_cast<const uint4*>(row + 8 * g);
      const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned p = ordered(w[i] & 0xffffu), q = ordered(w[i] >> 16);
        mn[2 * i] = p < mn[2 * i] ? p : mn[2 * i], mx[2 * i] = p > mx[2 * i] ? p : mx[2 * i];
        mn[2 * i + 1] = q < mn[2 * i + 1] ? q : mn[2 * i + 1], mx[2 * i + 1] = q > mx[2 * i + 1] ? q : mx[2 * i + 1];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) lo_s[r0][8 * g + e] = (unsigned short)mn[e], hi_s[r0][8 * g + e] = (unsigned short)mx[e];
  }
  __syncthreads();
  if (tid < D) {
    unsigned m = 0xffffu, M = 0u;
#pragma unroll 4
    for (int r = 0; r < RP; ++r) {
      const unsigned p = lo_s[r][tid], q = hi_s[r][tid];
      m = p < m ? p : m, M = q > M ? q : M;
    }
    if (m <= M) {  // (a block whose every page is out of range saw no key: not written)
      uint16_t* out = a.bounds + ((long)c * a.blocks + J) * 2 * D;
      out[tid] = (uint16_t)pattern(m);
      out[D + tid] = (uint16_t)pattern(M);
    }
  }
}

// The same kernel over a cache of e4m3fn bytes with bounds of T: a thread loads the 8 bytes of its 8 elements with one load,
// minima and maxima are taken and folded on ordered bytes, and thread d widens the two results of column d at the store.
template <class T, int D, bool PAGED>
__global__ __launch_bounds__(256) void kv_block_bounds_fp8_kernel(Args a) {
  constexpr int DV = D / 8;
  constexpr int RP = 256 / DV;
  __shared__ __attribute__((aligned(8))) unsigned char lo_s[RP][D], hi_s[RP][D];
  const int tid = threadIdx.x, c = blockIdx.y;
  const int b = c / a.heads, h = c - b * a.heads;
  int J, rows;
  if (!own_block(a, J, rows)) return;
  const int r0 = tid / DV, g = tid - r0 * DV;
  unsigned mn[8], mx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mn[e] = 0xffu, mx[e] = 0u;
  if (r0 < RP) {
    for (int r = r0; r < rows; r += RP) {
      const uint8_t* row = key_row<PAGED, uint8_t>(a, b, h, (long)J * kB + r);
      if (!row) continue;
      const uint2 x = *reinterpret_cast<const uint2*>(row + 8 * g);
      const unsigned w[2] = {x.x, x.y};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned p = ordered8((w[e >> 2] >> (8 * (e & 3))) & 0xffu);
        mn[e] = p < mn[e] ? p : mn[e], mx[e] = p > mx[e] ? p : mx[e];
      }
    }
    uint2 lo, hi;
    lo.x = mn[0] | (mn[1] << 8) | (mn[2] << 16) | (mn[3] << 24), lo.y = mn[4] | (mn[5] << 8) | (mn[6] << 16) | (mn[7] << 24);
    hi.x = mx[0] | (mx[1] << 8) | (mx[2] << 16) | (mx[3] << 24), hi.y = mx[4] | (mx[5] << 8) | (mx[6] << 16) | (mx[7] << 24);
    *reinterpret_cast<uint2*>(&lo_s[r0][8 * g]) = lo;
    *reinterpret_cast<uint2*>(&hi_s[r0][8 * g]) = hi;
  }
  __syncthreads();
  if (tid < D) {
    unsigned m = 0xffu, M = 0u;
#pragma unroll 4
    for (int r = 0; r < RP; ++r) {
      const unsigned p = lo_s[r][tid], q = hi_s[r][tid];
      m = p < m ? p : m, M = q > M ? q : M;
    }
    if (m <= M) {
      // the code as the 16-bit pattern of T (block_attention_cache_device.h's widening); −0 is written out: 0x8000
      auto wide = [](unsigned code) { return code == 0x80u ? 0x8000u : widen2<T, false>(code) & 0xffffu; };
      uint16_t* out = a.bounds + ((long)c * a.blocks + J) * 2 * D;
      out[tid] = (uint16_t)wide(pattern8(m));
      out[D + tid] = (uint16_t)wide(pattern8(M));
    }
  }
}

// which kernel: the 2-byte one, or the fp8 one with bounds of bfloat16 / float16
enum Form { k2Byte, kFp8Bf16, kFp8F16 };

template <int D, bool PAGED>
void launch_form(const Args& a, Form form, dim3 grid, hipStream_t s) {
  if (form == k2Byte)
    hipLaunchKernelGGL((kv_block_bounds_kernel<D, PAGED>), grid, dim3(256), 0, s, a);
  else if (form == kFp8Bf16)
    hipLaunchKernelGGL((kv_block_bounds_fp8_kernel<Bf16, D, PAGED>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((kv_block_bounds_fp8_kernel<F16, D, PAGED>), grid, dim3(256), 0, s, a);
}

template <int D>
int launch(const Args& a, Form form, int items, int grid_x, hipStream_t s) {
  const dim3 grid((unsigned)grid_x, (unsigned)items);
  if (a.table)
    launch_form<D, true>(a, form, grid, s);
  else
    launch_form<D, false>(a, form, grid, s);
  return mi::check_launch();
}

// Every check comes before the first HIP call.  page == 0: the contiguous cache, outerK its batch stride and no table;
// page > 0: a pool of `pages` pages of `page` keys, outerK its page stride, Smax = the table's logical pages · page.  `form`:
// the cache's element — with an fp8 cache the strides are counted, and checked, in bytes.
int bounds_entry(Form form, int32_t items, int32_t heads, int32_t Smax, int32_t D, const void* k, int64_t ldk, int64_t headK, int64_t outerK,
                 const int32_t* k_lens, int32_t lens_count, int32_t last, uint16_t* bounds, hipStream_t s,
                 const int32_t* table = nullptr, int64_t table_ld = 0, int32_t pages = 0, int32_t page = 0) {
  const bool fp8 = form != k2Byte;  // (its scales are not this call's: none to check)
  if (!cache_form_ok(false, Scales(), heads, Smax, pages, page) || !takes_width(D)) return MI_EINVAL;
  const bool paged = page != 0;
  if (items < 0 || heads < 0 || Smax < 0 || Smax % kB != 0 || last < 0) return MI_EINVAL;
  if (items > 65535) return MI_EINVAL;  // the grid's y, as in the decode calls
  if (items == 0 || Smax == 0) return MI_OK;
  if (heads == 0 || items % heads != 0 || lens_count < 1 || items % lens_count != 0) return MI_EINVAL;
  if (!k_lens || !aligned4(k_lens) || !bounds || !mi::aligned16(bounds)) return MI_EINVAL;
  const bool reads = !paged || pages > 0;  // (an empty pool: every key is invisible, nothing is read or written)
  if (!cache_operands_ok(fp8, reads, Smax, D, k, ldk, headK, outerK, k, ldk, headK, outerK, table, table_ld, page)) return MI_EINVAL;
  if (!reads) return MI_OK;
  Args a = {};
  a.heads = heads, a.blocks = Smax / kB, a.last = last, a.smax = Smax;
  a.k = k, a.ldk = ldk, a.headK = headK, a.outerK = outerK;
  a.k_lens = k_lens, a.lens_div = items / lens_count;
  if (paged) a.table = table, a.table_ld = table_ld, a.pages = pages, a.page_shift = __builtin_ctz((unsigned)page);
  a.bounds = bounds;
  // `last` positions touch at most ⌈(last − 1) / 64⌉ + 1 blocks
  const long span = last > 0 ? ((long)last + 62) / kB + 1 : a.blocks;
  const int grid_x = (int)(span < a.blocks ? span : a.blocks);
  switch (D) {
    case 32: return launch<32>(a, form, items, grid_x, s);
    case 64: return launch<64>(a, form, items, grid_x, s);
    case 96: return launch<96>(a, form, items, grid_x, s);
    default: return launch<128>(a, form, items, grid_x, s);
  }
}

}  // namespace

extern "C" {

#define MI_BOUNDS_ARGS(CT)                                                                                                 \
  int32_t D, const CT *k, int64_t ldk, int64_t headK, int64_t batchK, const int32_t *k_lens, int32_t lens_count, \
      int32_t last, uint16_t *bounds, mi_stream_t stream
#define MI_BOUNDS_PASS(FORM) FORM, items, heads, Smax, D, k, ldk, headK, batchK, k_lens, lens_count, last, bounds, static_cast<hipStream_t>(stream)

// (the two types share one kernel: minima and maxima are taken on the ordered bit patterns)
int mi_kv_block_bounds_bf16(int32_t items, int32_t heads, int32_t Smax, MI_BOUNDS_ARGS(uint16_t)) { return bounds_entry(MI_BOUNDS_PASS(k2Byte)); }
int mi_kv_block_bounds_f16(int32_t items, int32_t heads, int32_t Smax, MI_BOUNDS_ARGS(uint16_t)) { return bounds_entry(MI_BOUNDS_PASS(k2Byte)); }
// (k and batchK stand for k_pages and pageK of the header)  A page of 0 keys would name the contiguous form: refused here.
int mi_kv_block_bounds_paged_bf16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                  int32_t pages, int32_t page, MI_BOUNDS_ARGS(uint16_t)) {
  return page < 16 ? MI_EINVAL : bounds_entry(MI_BOUNDS_PASS(k2Byte), block_table, table_ld, pages, page);
}
int mi_kv_block_bounds_paged_f16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                 int32_t pages, int32_t page, MI_BOUNDS_ARGS(uint16_t)) {
  return page < 16 ? MI_EINVAL : bounds_entry(MI_BOUNDS_PASS(k2Byte), block_table, table_ld, pages, page);
}

// an fp8 cache: the same lists with a cache of e4m3fn bytes and strides in bytes; the suffix is the bounds' type
#define MI_BOUNDS_PAGED_ARGS int32_t items, int32_t heads, int32_t Smax, const int32_t *block_table, int64_t table_ld, int32_t pages, int32_t page
int mi_kv_block_bounds_fp8_bf16(int32_t items, int32_t heads, int32_t Smax, MI_BOUNDS_ARGS(uint8_t)) {
  return bounds_entry(MI_BOUNDS_PASS(kFp8Bf16));
}
int mi_kv_block_bounds_fp8_f16(int32_t items, int32_t heads, int32_t Smax, MI_BOUNDS_ARGS(uint8_t)) {
  return bounds_entry(MI_BOUNDS_PASS(kFp8F16));
}
int mi_kv_block_bounds_paged_fp8_bf16(MI_BOUNDS_PAGED_ARGS, MI_BOUNDS_ARGS(uint8_t)) {
  return page < 16 ? MI_EINVAL : bounds_entry(MI_BOUNDS_PASS(kFp8Bf16), block_table, table_ld, pages, page);
}
int mi_kv_block_bounds_paged_fp8_f16(MI_BOUNDS_PAGED_ARGS, MI_BOUNDS_ARGS(uint8_t)) {
  return page < 16 ? MI_EINVAL : bounds_entry(MI_BOUNDS_PASS(kFp8F16), block_table, table_ld, pages, page);
}

}  // extern "C"
