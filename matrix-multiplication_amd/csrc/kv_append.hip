// The write side of decoding: the keys and values of the T newest tokens of every item appended to a key / value cache in ONE
// launch — the cache of block_attention_decode.hip in its four forms: contiguous or paged, 2-byte (bfloat16 / float16) or OCP
// e4m3fn bytes with a float32 scale per k / v head.
//
// What it writes (contract of include/mi_spmm.h, mi_kv_append_* — DESIGN.md §3.21):
//  * k_lens is the length AFTER the append — the tensor the decode call takes next.  Token t of k / v item c (head c % heads of
//    batch item c / heads) goes to pos = k_len − T + t; it is written iff 0 ≤ pos < Smax and, paged, the table entry of logical
//    page pos / page lies in [0, pages).  Otherwise it is DROPPED: nothing is stored for it anywhere.  k_len is not clamped: a
//    length beyond Smax drops what does not fit and moves nothing.
//  * The 2-byte forms copy bits (NaN payloads, −0).  The fp8 forms store, per element, the byte of torch's CPU expression
//    (float32(x) / scale[h]).clamp(−448, 448).to(float8_e4m3fn): the IEEE float32 quotient (taken through a double
//    reciprocal: `quotient` in kv_cache_device.h, which owns this rule — DESIGN.md §3.23), the clamp, ONE
//    round-to-nearest-even into e4m3fn (v_cvt_pk_fp8_f32, the OCP encoding on gfx950).  v_med3_f32 — what the clamp compiles
//    to — turns a NaN into ±448, so a NaN quotient is given its own path: its byte is ORed with 0x7F, a NaN code.
//  * Everything else keeps its bytes: other rows, the gap between the rows of a padded cache, unreferenced pages.
//
// Kernel: one thread moves 8 consecutive elements of one k row and the same 8 of the matching v row — two 16-byte global
// loads, two 16-byte stores (copy) or two 8-byte stores (fp8).  pos, the table entry — read as the decode walk reads it:
// table[(c / heads) · table_ld + (pos >> shift)] — and the two scales are taken once per thread, i.e. per 8 + 8 elements of
// one row.  The threads of all rows are numbered in one flat index (item, token, 8-element group): the grid is one-dimensional,
// ⌈items · T · D/8 / 256⌉ workgroups of 256 threads — or of 64 while that would be fewer workgroups than the chip has CUs, so
// that a decode step (T = 1) still spreads.  No LDS, no barrier, no atomics, plain vector stores: graph-capturable, and which
// write lands when two (item, token) pairs are mapped to one pool row is unspecified.
#include "kv_cache_device.h"

namespace {

// The cache element as a compile-time form, as in block_attention_decode.hip: B16 — a 2-byte cache of the source's own type,
// a bit copy — or Fp8<T>: a source of T over a cache of e4m3fn bytes
struct B16 {};
template <class T>
struct Fp8 {};

struct Args {
  int n;              // threads with work: items · T · D/8
  int heads, T;       // k / v item c is head c % heads of batch item c / heads
  long smax;          // rows of an item's cache: Smax, or paged the table's logical pages · page
  const uint16_t *k_new, *v_new;  // token t of item c: k_new + (c / heads) · batchKn + (c % heads) · headKn + t · ldkn
  long ldkn, headKn, batchKn, ldvn, headVn, batchVn;
  void *k, *v;        // row j of item c: k + (c / heads) · batchK + (c % heads) · headK + j · ldk (in cache elements); paged:
                      // k + table[(c / heads) · table_ld + (j >> page_shift)] · pageK + (c % heads) · headK + (j & (page − 1)) · ldk
  long ldk, headK, outerK, ldv, headV, outerV;
  const int32_t* k_lens;  // [items / lens_div], the lengths AFTER the append; not clamped
  int lens_div;
  const int32_t* table;   // [items / heads][table_ld]; an entry outside [0, pages) drops its tokens
  long table_ld;
  int pages, page_shift;
  const float *k_scale, *v_scale;  // the fp8 forms: null is 1, a count of 1 one scale for all heads, else one per k / v head
  int k_scale_count, v_scale_count;
};

// what store_cache (kv_cache_device.h) takes for a form: the source's type, which only the fp8 form looks at
template <class TC>
struct Form {
  typedef void type;
  static constexpr bool fp8 = false;
};
template <class T>
struct Form<Fp8<T>> {
  typedef T type;
  static constexpr bool fp8 = true;
};

template <class TC, int D, bool PAGED>
__global__ __launch_bounds__(256) void kv_append_kernel(Args a) {
  constexpr int DV = D / 8;  // threads of a row
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;  // (n < 2³¹: no wrap)
  if (idx >= (unsigned)a.n) return;
  const unsigned row = idx / DV;
  const int d = (int)(idx - row * DV) * 8;
  const int c = (int)(row / (unsigned)a.T), t = (int)(row - (unsigned)c * (unsigned)a.T);
  const int b = c / a.heads, h = c - b * a.heads;
  const long pos = (long)a.k_lens[c / a.lens_div] - a.T + t;
  if (pos < 0 || pos >= a.smax) return;  // dropped: the token does not exist, or does not fit
  long ko, vo;
  if constexpr (PAGED) {
    const int e = a.table[(long)b * a.table_ld + (pos >> a.page_shift)];
    if ((unsigned)e >= (unsigned)a.pages) return;  // dropped: no page
    const long r = pos & ((1L << a.page_shift) - 1);
    ko = (long)e * a.outerK + (long)h * a.headK + r * a.ldk + d;
    vo = (long)e * a.outerV + (long)h * a.headV + r * a.ldv + d;
  } else {
    ko = (long)b * a.outerK + (long)h * a.headK + pos * a.ldk + d;
    vo = (long)b * a.outerV + (long)h * a.headV + pos * a.ldv + d;
  }
  const uint4 kx = *reinterpret_cast<const uint4*>(a.k_new + (long)b * a.batchKn + (long)h * a.headKn + (long)t * a.ldkn + d);
  const uint4 vx = *reinterpret_cast<const uint4*>(a.v_new + (long)b * a.batchVn + (long)h * a.headVn + (long)t * a.ldvn + d);
  double ks = 1.0, vs = 1.0;  // the fp8 forms: 1 / scale[h] in double, one division per thread and tensor
  if constexpr (Form<TC>::fp8) {
    ks = 1.0 / (double)head_scale(a.k_scale, a.k_scale_count, h);
    vs = 1.0 / (double)head_scale(a.v_scale, a.v_scale_count, h);
  }
  store_cache<typename Form<TC>::type, Form<TC>::fp8>(a.k, ko, kx, ks);
  store_cache<typename Form<TC>::type, Form<TC>::fp8>(a.v, vo, vx, vs);
}

template <class TC, int D>
int launch(const Args& a, hipStream_t s) {
  const unsigned threads = a.n < kSpread * 256 ? 64u : 256u;
  const dim3 grid((unsigned)((a.n + threads - 1) / threads));
  if (a.table)
    hipLaunchKernelGGL((kv_append_kernel<TC, D, true>), grid, dim3(threads), 0, s, a);
  else
    hipLaunchKernelGGL((kv_append_kernel<TC, D, false>), grid, dim3(threads), 0, s, a);
  return mi::check_launch();
}

// Every check comes before the first HIP call.  page == 0: the contiguous cache, `outerK` / `outerV` its batch strides and no
// table; page > 0: a pool of `pages` pages of `page` rows, `outerK` / `outerV` its page strides, Smax = the table's logical
// pages · page.
template <class TC>
int append_entry(int32_t items, int32_t heads, int32_t T_, int32_t Smax, int32_t D, const uint16_t* k_new, int64_t ldkn,
                 int64_t headKn, int64_t batchKn, const uint16_t* v_new, int64_t ldvn, int64_t headVn, int64_t batchVn, void* k,
                 int64_t ldk, int64_t headK, int64_t outerK, void* v, int64_t ldv, int64_t headV, int64_t outerV,
                 const int32_t* k_lens, int32_t lens_count, hipStream_t s, const int32_t* table = nullptr, int64_t table_ld = 0,
                 int32_t pages = 0, int32_t page = 0, const Scales& scales = Scales()) {
  constexpr bool FP8 = Form<TC>::fp8;
  if (!cache_form_ok(FP8, scales, heads, Smax, pages, page) || !takes_width(D)) return MI_EINVAL;
  const bool paged = page != 0;
  if (items < 0 || heads < 0 || T_ < 0 || Smax < 0) return MI_EINVAL;
  if (items > 65535) return MI_EINVAL;  // the decode calls' limit: their grid's y
  if (items == 0 || T_ == 0) return MI_OK;
  if (heads == 0 || items % heads != 0 || lens_count < 1 || items % lens_count != 0) return MI_EINVAL;
  if (!k_lens || !aligned4(k_lens)) return MI_EINVAL;
  if (!k_new || !mi::aligned16(k_new) || !stride_ok(ldkn) || !stride_ok(headKn) || !stride_ok(batchKn)) return MI_EINVAL;
  if (!v_new || !mi::aligned16(v_new) || !stride_ok(ldvn) || !stride_ok(headVn) || !stride_ok(batchVn)) return MI_EINVAL;
  const bool written = Smax > 0 && (!paged || pages > 0);  // (an empty cache or pool: every token is dropped, nothing is read)
  if (!cache_operands_ok(FP8, written, Smax, D, k, ldk, headK, outerK, v, ldv, headV, outerV, table, table_ld, page)) return MI_EINVAL;
  const long n = (long)items * T_ * (D / 8);
  if (n > 0x7fffffffL) return MI_ERANGE;
  if (!written) return MI_OK;
  Args a = {};
  a.n = (int)n, a.heads = heads, a.T = T_, a.smax = Smax;
  a.k_new = k_new, a.ldkn = ldkn, a.headKn = headKn, a.batchKn = batchKn;
  a.v_new = v_new, a.ldvn = ldvn, a.headVn = headVn, a.batchVn = batchVn;
  a.k = k, a.ldk = ldk, a.headK = headK, a.outerK = outerK, a.v = v, a.ldv = ldv, a.headV = headV, a.outerV = outerV;
  a.k_lens = k_lens, a.lens_div = items / lens_count;
  if (paged) a.table = table, a.table_ld = table_ld, a.pages = pages, a.page_shift = __builtin_ctz((unsigned)page);
  if (FP8) a.k_scale = scales.k, a.k_scale_count = scales.k_count, a.v_scale = scales.v, a.v_scale_count = scales.v_count;
  switch (D) {
    case 32: return launch<TC, 32>(a, s);
    case 64: return launch<TC, 64>(a, s);
    case 96: return launch<TC, 96>(a, s);
    default: return launch<TC, 128>(a, s);
  }
}

}  // namespace

extern "C" {

#define MI_APPEND_ARGS(CT)                                                                                                       \
  const uint16_t *k_new, int64_t ldkn, int64_t headKn, int64_t batchKn, const uint16_t *v_new, int64_t ldvn, int64_t headVn,     \
      int64_t batchVn, CT *k, int64_t ldk, int64_t headK, int64_t batchK, CT *v, int64_t ldv, int64_t headV, int64_t batchV,      \
      const int32_t *k_lens, int32_t lens_count
#define MI_APPEND_PASS                                                                                                         \
  items, heads, T, Smax, D, k_new, ldkn, headKn, batchKn, v_new, ldvn, headVn, batchVn, k, ldk, headK, batchK, v, ldv, headV, \
      batchV, k_lens, lens_count, static_cast<hipStream_t>(stream)
#define MI_APPEND_SIZES int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D
// (k, batchK and v, batchV stand for k_pages, pageK and v_pages, pageV of the header)  A page of 0 rows would name the
// contiguous form: it is refused here like every page that is no power of two ≥ 16.
#define MI_APPEND_PAGED_SIZES \
  int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t *block_table, int64_t table_ld, int32_t pages, int32_t page, int32_t D
#define MI_APPEND_SCALE_ARGS const float *k_scale, int32_t k_scale_count, const float *v_scale, int32_t v_scale_count
#define MI_APPEND_SCALES Scales{k_scale, k_scale_count, v_scale, v_scale_count}

int mi_kv_append_b16(MI_APPEND_SIZES, MI_APPEND_ARGS(uint16_t), mi_stream_t stream) { return append_entry<B16>(MI_APPEND_PASS); }
int mi_kv_append_paged_b16(MI_APPEND_PAGED_SIZES, MI_APPEND_ARGS(uint16_t), mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : append_entry<B16>(MI_APPEND_PASS, block_table, table_ld, pages, page);
}
int mi_kv_append_fp8_bf16(MI_APPEND_SIZES, MI_APPEND_ARGS(uint8_t), MI_APPEND_SCALE_ARGS, mi_stream_t stream) {
  return append_entry<Fp8<Bf16>>(MI_APPEND_PASS, nullptr, 0, 0, 0, MI_APPEND_SCALES);
}
int mi_kv_append_fp8_f16(MI_APPEND_SIZES, MI_APPEND_ARGS(uint8_t), MI_APPEND_SCALE_ARGS, mi_stream_t stream) {
  return append_entry<Fp8<F16>>(MI_APPEND_PASS, nullptr, 0, 0, 0, MI_APPEND_SCALES);
}
int mi_kv_append_paged_fp8_bf16(MI_APPEND_PAGED_SIZES, MI_APPEND_ARGS(uint8_t), MI_APPEND_SCALE_ARGS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : append_entry<Fp8<Bf16>>(MI_APPEND_PASS, block_table, table_ld, pages, page, MI_APPEND_SCALES);
}
int mi_kv_append_paged_fp8_f16(MI_APPEND_PAGED_SIZES, MI_APPEND_ARGS(uint8_t), MI_APPEND_SCALE_ARGS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : append_entry<Fp8<F16>>(MI_APPEND_PASS, block_table, table_ld, pages, page, MI_APPEND_SCALES);
}

}  // extern "C"
