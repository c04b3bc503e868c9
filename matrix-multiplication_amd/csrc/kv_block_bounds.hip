// Per-block key bounds of a key cache: for every 64-key block of every k / v item the elementwise minimum and maximum of the
// keys it holds — what block_select.hip scores a query against.  The cache is the one of
// block_attention_decode.hip in its two 2-byte forms, contiguous or paged.
//
// What it writes (contract of include/mi_spmm.h, mi_kv_block_bounds{,_paged}_{bf16,f16}):
//  * bounds [items][Smax / 64][2][D] in the cache's type: bounds[c][J][0][d] = min, bounds[c][J][1][d] = max of k[c][j][d] over
//    the SEEN keys j of block J: 64J ≤ j < min(64J + 64, k_len), and, paged, the table entry of j's logical page in [0, pages).
//    k_len is clamped to [0, Smax].  A block with no seen key is NOT WRITTEN; neither is anything else.
//  * last = 0 refreshes every block with a seen key; last = T ≥ 1 only the blocks that hold a position of
//    [k_len − T, k_len) — the refresh after an append of T tokens.
//  * min and max are exact and a function of the seen keys alone: the 16-bit patterns are compared as ordered integers (sign
//    and magnitude turned into one unsigned order, in which −0 < +0), so neither the order of the rows, nor the launch, nor
//    the form of the cache can show in the bits, and no widening is needed: ONE kernel serves bfloat16 and float16.  A NaN
//    pattern sorts beyond ±inf on its sign's side: the result with NaN keys is unspecified, and nothing faults.
//  * Nothing outside is read: rows at or beyond k_len, the gaps between the rows of a strided cache and the pages behind an
//    out-of-range table entry are never loaded.
//
// Kernel: grid (blocks refreshed, items), 256 threads; a thread owns 8 consecutive elements of the rows r, r + 256 / (D/8), …
// of its block — one 16-byte global load per row —, the partial minima and maxima of the threads of one column group meet in
// LDS and thread d < D folds column d over them.  No atomics, no read-back: graph-capturable.
#include "kv_cache_device.h"

namespace {

constexpr int kB = 64;  // keys of a block: the decode walk's tile

struct Args {
  int heads, blocks, last;  // k / v item c is head c % heads of batch item c / heads; blocks = Smax / 64; last: 0 = all
  long smax;
  const uint16_t* k;  // key j of item c: k + (c / heads) · outerK + (c % heads) · headK + j · ldk; paged:
                      // k + table[(c / heads) · table_ld + (j >> page_shift)] · outerK + (c % heads) · headK + (j & (page − 1)) · ldk
  long ldk, headK, outerK;
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

template <int D, bool PAGED>
__global__ __launch_bounds__(256) void kv_block_bounds_kernel(Args a) {
  constexpr int DV = D / 8;      // threads of a row
  constexpr int RP = 256 / DV;   // rows of a pass (D = 96: 21, and 4 threads idle)
  __shared__ unsigned short lo_s[RP][D], hi_s[RP][D];
  const int tid = threadIdx.x, c = blockIdx.y;
  const int b = c / a.heads, h = c - b * a.heads;
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
        row = a.k + (long)e * a.outerK + (long)h * a.headK + (j & ((1L << a.page_shift) - 1)) * a.ldk;
      } else {
        row = a.k + (long)b * a.outerK + (long)h * a.headK + j * a.ldk;
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

template <int D>
int launch(const Args& a, int items, int grid_x, hipStream_t s) {
  const dim3 grid((unsigned)grid_x, (unsigned)items);
  if (a.table)
    hipLaunchKernelGGL((kv_block_bounds_kernel<D, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((kv_block_bounds_kernel<D, false>), grid, dim3(256), 0, s, a);
  return mi::check_launch();
}

// Every check comes before the first HIP call.  page == 0: the contiguous cache, outerK its batch stride and no table;
// page > 0: a pool of `pages` pages of `page` keys, outerK its page stride, Smax = the table's logical pages · page.
int bounds_entry(int32_t items, int32_t heads, int32_t Smax, int32_t D, const uint16_t* k, int64_t ldk, int64_t headK, int64_t outerK,
                 const int32_t* k_lens, int32_t lens_count, int32_t last, uint16_t* bounds, hipStream_t s,
                 const int32_t* table = nullptr, int64_t table_ld = 0, int32_t pages = 0, int32_t page = 0) {
  if (!cache_form_ok(false, Scales(), heads, Smax, pages, page) || !takes_width(D)) return MI_EINVAL;
  const bool paged = page != 0;
  if (items < 0 || heads < 0 || Smax < 0 || Smax % kB != 0 || last < 0) return MI_EINVAL;
  if (items > 65535) return MI_EINVAL;  // the grid's y, as in the decode calls
  if (items == 0 || Smax == 0) return MI_OK;
  if (heads == 0 || items % heads != 0 || lens_count < 1 || items % lens_count != 0) return MI_EINVAL;
  if (!k_lens || !aligned4(k_lens) || !bounds || !mi::aligned16(bounds)) return MI_EINVAL;
  const bool reads = !paged || pages > 0;  // (an empty pool: every key is invisible, nothing is read or written)
  if (!cache_operands_ok(false, reads, Smax, D, k, ldk, headK, outerK, k, ldk, headK, outerK, table, table_ld, page)) return MI_EINVAL;
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
    case 32: return launch<32>(a, items, grid_x, s);
    case 64: return launch<64>(a, items, grid_x, s);
    case 96: return launch<96>(a, items, grid_x, s);
    default: return launch<128>(a, items, grid_x, s);
  }
}

}  // namespace

extern "C" {

#define MI_BOUNDS_ARGS                                                                                                     \
  int32_t D, const uint16_t *k, int64_t ldk, int64_t headK, int64_t batchK, const int32_t *k_lens, int32_t lens_count, \
      int32_t last, uint16_t *bounds, mi_stream_t stream
#define MI_BOUNDS_PASS items, heads, Smax, D, k, ldk, headK, batchK, k_lens, lens_count, last, bounds, static_cast<hipStream_t>(stream)

// (the two types share one kernel: minima and maxima are taken on the ordered bit patterns)
int mi_kv_block_bounds_bf16(int32_t items, int32_t heads, int32_t Smax, MI_BOUNDS_ARGS) { return bounds_entry(MI_BOUNDS_PASS); }
int mi_kv_block_bounds_f16(int32_t items, int32_t heads, int32_t Smax, MI_BOUNDS_ARGS) { return bounds_entry(MI_BOUNDS_PASS); }
// (k and batchK stand for k_pages and pageK of the header)  A page of 0 keys would name the contiguous form: refused here.
int mi_kv_block_bounds_paged_bf16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                  int32_t pages, int32_t page, MI_BOUNDS_ARGS) {
  return page < 16 ? MI_EINVAL : bounds_entry(MI_BOUNDS_PASS, block_table, table_ld, pages, page);
}
int mi_kv_block_bounds_paged_f16(int32_t items, int32_t heads, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                                 int32_t pages, int32_t page, MI_BOUNDS_ARGS) {
  return page < 16 ? MI_EINVAL : bounds_entry(MI_BOUNDS_PASS, block_table, table_ld, pages, page);
}

}  // extern "C"
