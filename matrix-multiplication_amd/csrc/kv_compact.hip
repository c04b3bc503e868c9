// After a speculative step: the accepted path's key / value rows moved to the front of the window of the T drafted slots, in
// place and in one launch for k and v — over the cache of block_attention_decode.hip in its four forms: contiguous or paged,
// 2-byte or e4m3fn bytes.  Rows are bit copies, so ONE kernel over row bytes serves every cache element.
//
// What it writes (contract of include/mi_spmm.h, mi_kv_compact{,_paged} — DESIGN.md §3.34):
//  * k_lens still counts the T drafted slots: the window of k / v item c (head c % heads of batch item b = c / heads) is the rows
//    [base, base + T), base = k_len − T (k_len is not clamped, as in kv_append.hip: a row outside [0, Smax) is not touched).
//    With n = clamp(accept_counts[b], 0, T), for i < n row base + i becomes the OLD row base + accept[b · T + i].
//  * Gather semantics: every source row of an (item, head, tensor) is read before any is written — one workgroup owns them all,
//    holds the rows in its threads' private pieces (T ≤ 64 rows of at most 256 bytes: four 16-byte pieces a thread, which the
//    compiler places in LDS: 16 KiB a workgroup) and crosses one workgroup barrier between its loads and its stores.  So the path [1, 2, 3] moves rows 1, 2, 3 to 0, 1, 2, whatever the order.
//  * Row i is left unwritten when its offset lies outside [0, T), its source or destination row outside [0, Smax), or — paged —
//    the table entry of either outside [0, pages).  Rows at or beyond n, and everything else, keep their bytes.  k_lens is not
//    written: the caller shrinks it on the device.
//
// Kernel: grid (items, 2): blockIdx.y = 0 moves k, 1 moves v; 256 threads; piece u = tid + 256 s of the n · (row bytes / 16)
// pieces is piece u % units of path entry u / units.  No atomics, no read-back, plain vector accesses: graph-capturable.
#include "kv_cache_device.h"

namespace {

constexpr int kMaxWindow = 64;  // T: the drafted slots of a step — the tree calls' limit
constexpr int kPieces = 4;      // 16-byte pieces a thread holds: 64 rows · 16 pieces / 256 threads

struct Args {
  int heads, T;
  long smax;
  unsigned char *k, *v;  // row j of item c: k + (c / heads) · outerK + (c % heads) · headK + j · ldk, IN BYTES; paged:
                         // k + table[(c / heads) · table_ld + (j >> page_shift)] · outerK + (c % heads) · headK + (j & (page − 1)) · ldk
  long ldk, headK, outerK, ldv, headV, outerV;
  const int32_t* k_lens;  // [items / lens_div], the lengths that still count the T drafted slots; not clamped
  int lens_div;
  const int32_t* accept;  // [items / heads][T]: offsets into the window
  const int32_t* counts;  // [items / heads]
  const int32_t* table;   // [items / heads][table_ld]; a row behind an entry outside [0, pages) is neither read nor written
  long table_ld;
  int pages, page_shift;
  int units;              // 16-byte pieces of a row: D · element bytes / 16
};

template <bool PAGED>
__global__ __launch_bounds__(256) void kv_compact_kernel(Args a) {
  const int c = blockIdx.x, b = c / a.heads, h = c - b * a.heads, tid = threadIdx.x;
  const bool values = blockIdx.y != 0;
  unsigned char* const cache = values ? a.v : a.k;
  const long ld = values ? a.ldv : a.ldk, head = values ? a.headV : a.headK, outer = values ? a.outerV : a.outerK;
  const long base = (long)a.k_lens[c / a.lens_div] - a.T;
  int n = a.counts[b];
  n = n < 0 ? 0 : n > a.T ? a.T : n;
  const int total = n * a.units;
  auto row = [&](long j) -> unsigned char* {  // row j of this (item, head, tensor), or null: it is not touched
    if (j < 0 || j >= a.smax) return nullptr;
    if constexpr (PAGED) {
      const int e = a.table[(long)b * a.table_ld + (j >> a.page_shift)];
      if ((unsigned)e >= (unsigned)a.pages) return nullptr;
      return cache + (long)e * outer + (long)h * head + (j & ((1L << a.page_shift) - 1)) * ld;
    } else {
      return cache + (long)b * outer + (long)h * head + j * ld;
    }
  };
  uint4 piece[kPieces];
  unsigned char* to[kPieces];
#pragma unroll
  for (int s = 0; s < kPieces; ++s) {
    to[s] = nullptr;
    const int u = tid + 256 * s;
    if (u >= total) continue;
    const int i = u / a.units, part = u - i * a.units;
    const int off = a.accept[(long)b * a.T + i];
    if ((unsigned)off >= (unsigned)a.T) continue;
    const unsigned char* from = row(base + off);
    unsigned char* dst = row(base + i);
    if (!from || !dst) continue;
    piece[s] = *reinterpret_cast<const uint4*>(from + 16 * part);
    to[s] = dst + 16 * part;
  }
  __syncthreads();  // every source row of this (item, head, tensor) is in registers
#pragma unroll
  for (int s = 0; s < kPieces; ++s)
    if (to[s]) *reinterpret_cast<uint4*>(to[s]) = piece[s];
}

// Every check comes before the first HIP call.  page == 0: the contiguous cache; page > 0: a pool, as in append_entry
// (kv_append.hip).  elem_bytes: 2 (bfloat16 / float16) or 1 (e4m3fn) — the strides count elements.
int compact_entry(int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, int32_t elem_bytes, void* k, int64_t ldk,
                  int64_t headK, int64_t outerK, void* v, int64_t ldv, int64_t headV, int64_t outerV, const int32_t* k_lens,
                  int32_t lens_count, const int32_t* accept, const int32_t* accept_counts, hipStream_t s,
                  const int32_t* table = nullptr, int64_t table_ld = 0, int32_t pages = 0, int32_t page = 0) {
  if (elem_bytes != 1 && elem_bytes != 2) return MI_EINVAL;
  const bool bytes = elem_bytes == 1;
  if (!cache_form_ok(bytes, Scales(), heads, Smax, pages, page) || !takes_width(D)) return MI_EINVAL;
  const bool paged = page != 0;
  if (items < 0 || heads < 0 || T < 0 || Smax < 0 || T > kMaxWindow) return MI_EINVAL;
  if (items > 65535) return MI_EINVAL;  // the grid's x; the decode calls' limit
  if (items == 0 || T == 0) return MI_OK;
  if (heads == 0 || items % heads != 0 || lens_count < 1 || items % lens_count != 0) return MI_EINVAL;
  if (!k_lens || !aligned4(k_lens) || !accept || !aligned4(accept) || !accept_counts || !aligned4(accept_counts)) return MI_EINVAL;
  const bool touched = Smax > 0 && (!paged || pages > 0);  // (an empty cache or pool: no row is touched, nothing is read)
  if (!cache_operands_ok(bytes, touched, Smax, D, k, ldk, headK, outerK, v, ldv, headV, outerV, table, table_ld, page)) return MI_EINVAL;
  if (!touched) return MI_OK;
  Args a = {};
  a.heads = heads, a.T = T, a.smax = Smax;
  a.k = static_cast<unsigned char*>(k), a.v = static_cast<unsigned char*>(v);
  a.ldk = ldk * elem_bytes, a.headK = headK * elem_bytes, a.outerK = outerK * elem_bytes;
  a.ldv = ldv * elem_bytes, a.headV = headV * elem_bytes, a.outerV = outerV * elem_bytes;
  a.k_lens = k_lens, a.lens_div = items / lens_count, a.accept = accept, a.counts = accept_counts;
  if (paged) a.table = table, a.table_ld = table_ld, a.pages = pages, a.page_shift = __builtin_ctz((unsigned)page);
  a.units = D * elem_bytes / 16;
  static_assert(kMaxWindow * (128 * 2 / 16) <= 256 * kPieces, "a thread's pieces hold the widest window");
  const dim3 grid((unsigned)items, 2);
  if (paged)
    hipLaunchKernelGGL((kv_compact_kernel<true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((kv_compact_kernel<false>), grid, dim3(256), 0, s, a);
  return mi::check_launch();
}

}  // namespace

extern "C" {

#define MI_COMPACT_ARGS                                                                                                        \
  int32_t D, int32_t elem_bytes, void *k, int64_t ldk, int64_t headK, int64_t batchK, void *v, int64_t ldv, int64_t headV,     \
      int64_t batchV, const int32_t *k_lens, int32_t lens_count, const int32_t *accept, const int32_t *accept_counts, mi_stream_t stream
#define MI_COMPACT_PASS                                                                                                       \
  items, heads, T, Smax, D, elem_bytes, k, ldk, headK, batchK, v, ldv, headV, batchV, k_lens, lens_count, accept, accept_counts, \
      static_cast<hipStream_t>(stream)

int mi_kv_compact(int32_t items, int32_t heads, int32_t T, int32_t Smax, MI_COMPACT_ARGS) { return compact_entry(MI_COMPACT_PASS); }
// (k, batchK and v, batchV stand for k_pages, pageK and v_pages, pageV of the header; a page of 0 rows would name the contiguous form)
int mi_kv_compact_paged(int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t* block_table, int64_t table_ld,
                        int32_t pages, int32_t page, MI_COMPACT_ARGS) {
  return page < 16 ? MI_EINVAL : compact_entry(MI_COMPACT_PASS, block_table, table_ld, pages, page);
}

}  // extern "C"
