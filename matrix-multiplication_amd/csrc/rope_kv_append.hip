// The step in front of the append, fused into it: q and the keys of the T newest tokens of every item are ROTATED by position
// (rotary embedding, RoPE) with the caller's cos / sin tables, the rotated keys and the values are written into the key / value
// cache of block_attention_decode.hip — its four forms: contiguous or paged, 2-byte or e4m3fn bytes — and the rotated q into
// q_out, all in ONE launch.
//
// The rule (contract of include/mi_spmm.h, mi_rope_kv_append_* — DESIGN.md §3.22):
//  * pos = k_len − T + t in 64 bits, k_len the length AFTER the append, not clamped — the position of kv_append.hip.  With
//    n = T (no new_lens) or clamp(new_lens[b], 0, T), slot t HOLDS A TOKEN iff t ≥ T − n and 0 ≤ pos < table_rows.
//  * No token: the slot's rows of q_out, and of k_out if given, are zeros; nothing is stored into the cache.
//  * A token: its q rows and its k row are rotated by table row pos; q goes to q_out, k to k_out if given; k and v go into the
//    cache iff 0 ≤ pos < Smax and, paged, the table entry lies in [0, pages) — kv_append.hip's condition — and are dropped
//    otherwise.  Everything the rule does not write keeps its bytes.
//  * Explicit positions (mi_rope_pos_kv_append_* — DESIGN.md §3.34): with `positions` int32 [B][T] the ROTATION of slot t takes table
//    row positions[b][t] in the place of pos — a tree node is rotated by prefix length + depth while it is stored in slot t —,
//    and the slot holds a token iff the conditions above hold AND 0 ≤ positions[b][t] < table_rows.  Where the rows go — q_out's
//    and k_out's row t, the cache row pos — does not change; positions[b][t] = pos is the call without them, bit for bit.
//  * Bits: for pair index i < R/2 the pair (a, b) is (x[i], x[i + R/2]) — the NeoX halves — or, interleaved, (x[2i], x[2i + 1]);
//    with c = cos[pos, i], s = sin[pos, i] and the elements widened exactly:
//        a' = fl32(fl32(a·c) − fl32(b·s))      b' = fl32(fl32(b·c) + fl32(a·s))
//    — two products and one sum, each rounded to float32, NOT contracted into an fma, float32 subnormals kept — and one
//    round-to-nearest-even to the source type.  Elements d ≥ R of q and k and all of v are bit copies.  An fp8 cache receives
//    kv_append.hip's bytes of the rotated k AFTER that rounding: the cache is what mi_kv_append_* leaves for the rounded k.
//
// Kernel: one flat index over (item, token, head of q | k | v, 8-element group), one-dimensional grid, no LDS, no barrier, no
// atomics, plain vector stores, as kv_append_kernel.  A thread owns whole pairs, so q_out == q and k_out == k_new are safe:
// NeoX — the thread of the group at d < R/2 also takes the partner group at d + R/2 (two 16-byte loads of each of cos and
// sin), the thread of the partner group has nothing to do; interleaved — the four pairs of its own group (one 16-byte load of
// each table).  pos, the slot test, the table entry and the scales are taken once per thread.
// (in front of the pragma: the header's fp8 pieces hold a product, a clamp and a conversion, no multiply-add pair that
// contraction could fuse, so their bits do not depend on it; the pragma covers `rotate` below, which does)
#include "kv_cache_device.h"

#pragma clang fp contract(off)

namespace {

struct Src {  // a source-like operand: token t of head h of batch item b at p + b · batch + h · head + t · ld
  const uint16_t* p;
  long ld, head, batch;
};
struct Dst {
  uint16_t* p;
  long ld, head, batch;
};

struct Args {
  int n;                   // threads with work: B · (Hq + 2·Hkv) · T · D/8
  int Hq, Hkv, T, DV, R;   // DV = D/8 groups of a row; R = rotary_dim
  long smax;               // rows of an item's cache: Smax, or paged the table's logical pages · page
  long table_rows;         // rows of cos / sin
  Src q, k_new, v_new;
  Dst q_out, k_out;        // k_out.p null: the rotated k goes to the cache only
  const float *cos, *sin;  // [table_rows][ld], R/2 entries of a row used
  long ld;
  void *k, *v;             // as in kv_append.hip: row j of head h of batch item b (paged: of pool page e)
  long ldk, headK, outerK, ldv, headV, outerV;
  const int32_t* k_lens;   // [1] or [B], the lengths AFTER the append; not clamped
  int lens_each;           // 1: one entry per batch item; 0: one for all
  const int32_t* new_lens; // null, or [B]: clamped to [0, T] here
  const int32_t* table;    // [B][table_ld]; an entry outside [0, pages) drops its tokens
  long table_ld;
  int pages, page_shift;
  const float *k_scale, *v_scale;  // the fp8 forms: null is 1, a count of 1 one scale for all heads, else one per k / v head
  int k_scale_count, v_scale_count;
  const int32_t* positions;  // null, or [B][T]: the table row slot t is rotated by, in the place of pos
};

// ---- the rotation -------------------------------------------------------------------------------------------------------------
// one pair: two products and one sum each, every one rounded to float32.  Plain operators under the pragma above, NOT
// __fmul_rn / __fadd_rn: those are defined in a header, in front of the pragma, so their operations carry the `contract` flag
// of the default -ffp-contract=fast-honor-pragmas into this function when they are inlined, and the backend then fuses them
// (v_pk_fma_f32 — seen in this unit's assembly; tests/test_gpu_rope_kv_cache_append.py, test 2, tells the difference).
__device__ __forceinline__ void rotate(float a, float b, float c, float s, float& ra, float& rb) {
  const float ac = a * c, bs = b * s, bc = b * c, as = a * s;
  ra = ac - bs;
  rb = bc + as;
}

// NeoX: the pairs (xa[e], xb[e]) of two 8-element groups with cos / sin entries c[e], s[e]
template <class T>
__device__ __forceinline__ void rotate_halves(uint4& xa, uint4& xb, const float4 (&c)[2], const float4 (&s)[2]) {
  const unsigned wa[4] = {xa.x, xa.y, xa.z, xa.w}, wb[4] = {xb.x, xb.y, xb.z, xb.w};
  const float cc[8] = {c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w};
  const float ss[8] = {s[0].x, s[0].y, s[0].z, s[0].w, s[1].x, s[1].y, s[1].z, s[1].w};
  unsigned ya[4], yb[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float a0, b0, a1, b1;
    rotate(T::lo(wa[w]), T::lo(wb[w]), cc[2 * w], ss[2 * w], a0, b0);
    rotate(T::hi(wa[w]), T::hi(wb[w]), cc[2 * w + 1], ss[2 * w + 1], a1, b1);
    ya[w] = pack2<T>(a0, a1), yb[w] = pack2<T>(b0, b1);
  }
  xa = make_uint4(ya[0], ya[1], ya[2], ya[3]), xb = make_uint4(yb[0], yb[1], yb[2], yb[3]);
}

// interleaved: the four pairs (x[2m], x[2m + 1]) of one group with c[m], s[m]
template <class T>
__device__ __forceinline__ void rotate_pairs(uint4& x, float4 c, float4 s) {
  const unsigned w[4] = {x.x, x.y, x.z, x.w};
  const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {s.x, s.y, s.z, s.w};
  unsigned y[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    float a, b;
    rotate(T::lo(w[m]), T::hi(w[m]), cc[m], ss[m], a, b);
    y[m] = pack2<T>(a, b);
  }
  x = make_uint4(y[0], y[1], y[2], y[3]);
}

template <class T, bool FP8, bool PAGED, bool INTER>
__global__ __launch_bounds__(256) void rope_kv_append_kernel(Args a) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;  // (n < 2³¹: no wrap)
  if (idx >= (unsigned)a.n) return;
  const unsigned heads = (unsigned)(a.Hq + 2 * a.Hkv);
  const unsigned row = idx / (unsigned)a.DV;
  const int d = (int)(idx - row * (unsigned)a.DV) * 8;
  const unsigned slot = row / heads;
  const int j = (int)(row - slot * heads);  // head of q | k | v
  const int b = (int)(slot / (unsigned)a.T), t = (int)(slot - (unsigned)b * (unsigned)a.T);
  const int half = a.R >> 1;
  const bool v_head = j >= a.Hq + a.Hkv;
  // the groups this thread owns: its own at d, and — a rotated NeoX group of q or k — the partner at d + R/2
  const bool rotated = !v_head && d < a.R;
  const bool two = !INTER && rotated;
  if (two && d >= half) return;  // the partner group: its owner sits at d − R/2
  const long pos = (long)a.k_lens[a.lens_each ? b : 0] - a.T + t;
  int n_new = a.T;
  if (a.new_lens) n_new = min(max(a.new_lens[b], 0), a.T);
  bool token = t >= a.T - n_new && pos >= 0 && pos < a.table_rows;
  long turn = pos;  // the table row of the rotation
  if (a.positions) {
    turn = a.positions[(long)b * a.T + t];
    token = token && turn >= 0 && turn < a.table_rows;
  }

  if (!token) {  // zeros into q_out and k_out; nothing into the cache
    if (v_head) return;
    const bool is_q = j < a.Hq;
    const Dst& o = is_q ? a.q_out : a.k_out;
    if (!o.p) return;
    uint16_t* p = o.p + (long)b * o.batch + (long)(is_q ? j : j - a.Hq) * o.head + (long)t * o.ld + d;
    *reinterpret_cast<uint4*>(p) = make_uint4(0u, 0u, 0u, 0u);
    if (two) *reinterpret_cast<uint4*>(p + half) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }

  const int kind = j < a.Hq ? 0 : (v_head ? 2 : 1);
  const int h = kind == 0 ? j : (kind == 1 ? j - a.Hq : j - a.Hq - a.Hkv);
  // k and v: where the row goes in the cache, or nowhere (kv_append.hip's condition)
  bool cached = kind != 0 && pos < a.smax;
  long co = 0;
  if (cached) {
    const long ld = kind == 1 ? a.ldk : a.ldv, head = kind == 1 ? a.headK : a.headV, outer = kind == 1 ? a.outerK : a.outerV;
    if constexpr (PAGED) {
      const int e = a.table[(long)b * a.table_ld + (pos >> a.page_shift)];
      cached = (unsigned)e < (unsigned)a.pages;  // else dropped: no page
      co = (long)e * outer + (long)h * head + (pos & ((1L << a.page_shift) - 1)) * ld + d;
    } else {
      co = (long)b * outer + (long)h * head + pos * ld + d;
    }
  }
  if (kind == 2 && !cached) return;
  const Src& src = kind == 0 ? a.q : (kind == 1 ? a.k_new : a.v_new);
  const uint16_t* sp = src.p + (long)b * src.batch + (long)h * src.head + (long)t * src.ld + d;
  uint4 x = *reinterpret_cast<const uint4*>(sp), y = make_uint4(0u, 0u, 0u, 0u);
  if (rotated) {
    if constexpr (INTER) {
      const long at = turn * a.ld + (d >> 1);
      rotate_pairs<T>(x, *reinterpret_cast<const float4*>(a.cos + at), *reinterpret_cast<const float4*>(a.sin + at));
    } else {
      y = *reinterpret_cast<const uint4*>(sp + half);
      const long at = turn * a.ld + d;
      const float4 c[2] = {*reinterpret_cast<const float4*>(a.cos + at), *reinterpret_cast<const float4*>(a.cos + at + 4)};
      const float4 s[2] = {*reinterpret_cast<const float4*>(a.sin + at), *reinterpret_cast<const float4*>(a.sin + at + 4)};
      rotate_halves<T>(x, y, c, s);
    }
  }
  if (kind != 2) {
    const Dst& o = kind == 0 ? a.q_out : a.k_out;
    if (o.p) {
      uint16_t* p = o.p + (long)b * o.batch + (long)h * o.head + (long)t * o.ld + d;
      *reinterpret_cast<uint4*>(p) = x;
      if (two) *reinterpret_cast<uint4*>(p + half) = y;
    }
  }
  if (!cached) return;
  double r = 1.0;  // the fp8 forms: 1 / scale[h] in double, one division per thread
  if constexpr (FP8)
    r = 1.0 / (double)(kind == 1 ? head_scale(a.k_scale, a.k_scale_count, h) : head_scale(a.v_scale, a.v_scale_count, h));
  void* base = kind == 1 ? a.k : a.v;
  store_cache<T, FP8>(base, co, x, r);
  if (two) store_cache<T, FP8>(base, co + half, y, r);
}

bool operand_ok(const void* p, int64_t ld, int64_t head, int64_t batch) {
  return p && mi::aligned16(p) && stride_ok(ld) && stride_ok(head) && stride_ok(batch);
}

template <class T, bool FP8>
int launch(const Args& a, bool inter, hipStream_t s) {
  const unsigned threads = a.n < kSpread * 256 ? 64u : 256u;
  const dim3 grid((unsigned)((a.n + threads - 1) / threads));
  if (a.table) {
    if (inter)
      hipLaunchKernelGGL((rope_kv_append_kernel<T, FP8, true, true>), grid, dim3(threads), 0, s, a);
    else
      hipLaunchKernelGGL((rope_kv_append_kernel<T, FP8, true, false>), grid, dim3(threads), 0, s, a);
  } else {
    if (inter)
      hipLaunchKernelGGL((rope_kv_append_kernel<T, FP8, false, true>), grid, dim3(threads), 0, s, a);
    else
      hipLaunchKernelGGL((rope_kv_append_kernel<T, FP8, false, false>), grid, dim3(threads), 0, s, a);
  }
  return mi::check_launch();
}

struct Rope {  // what the entries take beyond the append's arguments
  int32_t q_heads;
  Src q;
  Dst q_out, k_out;
  const float *cos, *sin;
  int32_t table_rows;
  int64_t ld;
  int32_t rotary_dim, interleaved;
  const int32_t* new_lens;
  const int32_t* positions = nullptr;  // the *_pos entries: [B][T], and …
  bool with_positions = false;         // … that the entry takes them: a null pointer is refused there
};

// Every check comes before the first HIP call.  page == 0: the contiguous cache; page > 0: a pool, as in kv_append.hip.
template <class T, bool FP8>
int rope_entry(int32_t items, int32_t heads, int32_t T_, int32_t Smax, int32_t D, const Rope& ro, Src k_new, Src v_new, void* k,
               int64_t ldk, int64_t headK, int64_t outerK, void* v, int64_t ldv, int64_t headV, int64_t outerV, const int32_t* k_lens,
               int32_t lens_count, hipStream_t s, const int32_t* table = nullptr, int64_t table_ld = 0, int32_t pages = 0,
               int32_t page = 0, const Scales& scales = Scales()) {
  if (!cache_form_ok(FP8, scales, heads, Smax, pages, page) || !takes_width(D)) return MI_EINVAL;
  const int32_t R = ro.rotary_dim;
  if (R < 16 || R > D || R % 16 != 0) return MI_EINVAL;
  const bool paged = page != 0;
  if (items < 0 || heads < 0 || T_ < 0 || Smax < 0 || ro.q_heads < 0 || ro.table_rows < 0) return MI_EINVAL;
  if (items > 65535) return MI_EINVAL;  // the decode calls' limit: their grid's y
  if (items == 0 || T_ == 0) return MI_OK;
  if (heads == 0 || items % heads != 0 || ro.q_heads == 0) return MI_EINVAL;
  const int32_t B = items / heads;
  if (lens_count != 1 && lens_count != B) return MI_EINVAL;  // (q has no k / v head: one length per batch item, or one for all)
  if (!k_lens || !aligned4(k_lens) || !aligned4(ro.new_lens)) return MI_EINVAL;
  if (ro.with_positions && (!ro.positions || !aligned4(ro.positions))) return MI_EINVAL;
  if (!operand_ok(ro.q.p, ro.q.ld, ro.q.head, ro.q.batch) || !operand_ok(ro.q_out.p, ro.q_out.ld, ro.q_out.head, ro.q_out.batch))
    return MI_EINVAL;
  if (!operand_ok(k_new.p, k_new.ld, k_new.head, k_new.batch) || !operand_ok(v_new.p, v_new.ld, v_new.head, v_new.batch)) return MI_EINVAL;
  if (ro.k_out.p && !operand_ok(ro.k_out.p, ro.k_out.ld, ro.k_out.head, ro.k_out.batch)) return MI_EINVAL;
  if (ro.ld < R / 2 || ro.ld % 4 != 0) return MI_EINVAL;
  if (ro.table_rows > 0 && (!ro.cos || !ro.sin || !mi::aligned16(ro.cos) || !mi::aligned16(ro.sin))) return MI_EINVAL;
  const bool written = Smax > 0 && (!paged || pages > 0);  // (an empty cache or pool: every k / v row is dropped; q is still rotated)
  if (!cache_operands_ok(FP8, written, Smax, D, k, ldk, headK, outerK, v, ldv, headV, outerV, table, table_ld, page)) return MI_EINVAL;
  const long n = (long)B * ((long)ro.q_heads + 2L * heads) * T_ * (D / 8);
  if (n > 0x7fffffffL) return MI_ERANGE;
  Args a = {};
  a.n = (int)n, a.Hq = ro.q_heads, a.Hkv = heads, a.T = T_, a.DV = D / 8, a.R = R;
  a.smax = written ? Smax : 0, a.table_rows = ro.table_rows;
  a.q = ro.q, a.k_new = k_new, a.v_new = v_new, a.q_out = ro.q_out, a.k_out = ro.k_out;
  a.cos = ro.cos, a.sin = ro.sin, a.ld = ro.ld;
  a.k = k, a.ldk = ldk, a.headK = headK, a.outerK = outerK, a.v = v, a.ldv = ldv, a.headV = headV, a.outerV = outerV;
  a.k_lens = k_lens, a.lens_each = lens_count == 1 ? 0 : 1, a.new_lens = ro.new_lens, a.positions = ro.positions;
  if (paged && written) a.table = table, a.table_ld = table_ld, a.pages = pages, a.page_shift = __builtin_ctz((unsigned)page);
  if (FP8) a.k_scale = scales.k, a.k_scale_count = scales.k_count, a.v_scale = scales.v, a.v_scale_count = scales.v_count;
  return launch<T, FP8>(a, ro.interleaved != 0, s);
}

}  // namespace

extern "C" {

#define MI_ROPE_ARGS(CT)                                                                                                         \
  int32_t q_heads, const uint16_t *q, int64_t ldq, int64_t headQ, int64_t batchQ, uint16_t *q_out, int64_t ldqo, int64_t headQo, \
      int64_t batchQo, const uint16_t *k_new, int64_t ldkn, int64_t headKn, int64_t batchKn, const uint16_t *v_new, int64_t ldvn, \
      int64_t headVn, int64_t batchVn, uint16_t *k_out, int64_t ldko, int64_t headKo, int64_t batchKo, const float *cos,          \
      const float *sin, int32_t table_rows, int64_t ld, int32_t rotary_dim, int32_t interleaved, CT *k, int64_t ldk,              \
      int64_t headK, int64_t batchK, CT *v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t *k_lens, int32_t lens_count, \
      const int32_t *new_lens
// (the variadic tail: what the *_pos entries add to the Rope record)
#define MI_ROPE_PASS_WITH(...)                                                                                                   \
  items, heads, T, Smax, D,                                                                                                     \
      Rope{q_heads,   Src{q, ldq, headQ, batchQ}, Dst{q_out, ldqo, headQo, batchQo}, Dst{k_out, ldko, headKo, batchKo}, cos, sin, \
           table_rows, ld, rotary_dim, interleaved, new_lens __VA_ARGS__},                                                       \
      Src{k_new, ldkn, headKn, batchKn}, Src{v_new, ldvn, headVn, batchVn}, k, ldk, headK, batchK, v, ldv, headV, batchV, k_lens, \
      lens_count, static_cast<hipStream_t>(stream)
#define MI_ROPE_PASS MI_ROPE_PASS_WITH()
#define MI_ROPE_POS_PASS MI_ROPE_PASS_WITH(, positions, true)
#define MI_ROPE_SIZES int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D
// (k, batchK and v, batchV stand for k_pages, pageK and v_pages, pageV of the header)  A page of 0 rows would name the
// contiguous form: it is refused here like every page that is no power of two ≥ 16.
#define MI_ROPE_PAGED_SIZES \
  int32_t items, int32_t heads, int32_t T, int32_t Smax, const int32_t *block_table, int64_t table_ld, int32_t pages, int32_t page, int32_t D
#define MI_ROPE_SCALE_ARGS const float *k_scale, int32_t k_scale_count, const float *v_scale, int32_t v_scale_count
#define MI_ROPE_SCALES Scales{k_scale, k_scale_count, v_scale, v_scale_count}
#define MI_ROPE_TABLE block_table, table_ld, pages, page

int mi_rope_kv_append_bf16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint16_t), mi_stream_t stream) { return rope_entry<Bf16, false>(MI_ROPE_PASS); }
int mi_rope_kv_append_f16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint16_t), mi_stream_t stream) { return rope_entry<F16, false>(MI_ROPE_PASS); }
int mi_rope_kv_append_paged_bf16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint16_t), mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<Bf16, false>(MI_ROPE_PASS, MI_ROPE_TABLE);
}
int mi_rope_kv_append_paged_f16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint16_t), mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<F16, false>(MI_ROPE_PASS, MI_ROPE_TABLE);
}
int mi_rope_kv_append_fp8_bf16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return rope_entry<Bf16, true>(MI_ROPE_PASS, nullptr, 0, 0, 0, MI_ROPE_SCALES);
}
int mi_rope_kv_append_fp8_f16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return rope_entry<F16, true>(MI_ROPE_PASS, nullptr, 0, 0, 0, MI_ROPE_SCALES);
}
int mi_rope_kv_append_paged_fp8_bf16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<Bf16, true>(MI_ROPE_PASS, MI_ROPE_TABLE, MI_ROPE_SCALES);
}
int mi_rope_kv_append_paged_fp8_f16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<F16, true>(MI_ROPE_PASS, MI_ROPE_TABLE, MI_ROPE_SCALES);
}

// … with explicit positions: the eight entries above with `positions` int32 [B][T] after new_lens.  (`pos`
// stands before `kv_append` in the name: the entries `mi_rope_kv_append…` are a closed family.)
#define MI_ROPE_POS const int32_t *positions
int mi_rope_pos_kv_append_bf16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint16_t), MI_ROPE_POS, mi_stream_t stream) {
  return rope_entry<Bf16, false>(MI_ROPE_POS_PASS);
}
int mi_rope_pos_kv_append_f16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint16_t), MI_ROPE_POS, mi_stream_t stream) {
  return rope_entry<F16, false>(MI_ROPE_POS_PASS);
}
int mi_rope_pos_kv_append_paged_bf16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint16_t), MI_ROPE_POS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<Bf16, false>(MI_ROPE_POS_PASS, MI_ROPE_TABLE);
}
int mi_rope_pos_kv_append_paged_f16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint16_t), MI_ROPE_POS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<F16, false>(MI_ROPE_POS_PASS, MI_ROPE_TABLE);
}
int mi_rope_pos_kv_append_fp8_bf16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_POS, MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return rope_entry<Bf16, true>(MI_ROPE_POS_PASS, nullptr, 0, 0, 0, MI_ROPE_SCALES);
}
int mi_rope_pos_kv_append_fp8_f16(MI_ROPE_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_POS, MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return rope_entry<F16, true>(MI_ROPE_POS_PASS, nullptr, 0, 0, 0, MI_ROPE_SCALES);
}
int mi_rope_pos_kv_append_paged_fp8_bf16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_POS, MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<Bf16, true>(MI_ROPE_POS_PASS, MI_ROPE_TABLE, MI_ROPE_SCALES);
}
int mi_rope_pos_kv_append_paged_fp8_f16(MI_ROPE_PAGED_SIZES, MI_ROPE_ARGS(uint8_t), MI_ROPE_POS, MI_ROPE_SCALE_ARGS, mi_stream_t stream) {
  return page < 16 ? MI_EINVAL : rope_entry<F16, true>(MI_ROPE_POS_PASS, MI_ROPE_TABLE, MI_ROPE_SCALES);
}

}  // extern "C"
