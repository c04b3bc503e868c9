// Block-sparse prefill attention over the KV cache in bfloat16 and float16 on the matrix cores: the T newest tokens of every
// item — a whole prompt, or one chunk of it behind a prefix that is already cached — against a key / value cache in any of
// its four forms, out = softmax(scale · q·kᵀ + mask) · v.  Token t of an item of length k_len stands at pos = k_len − T + t and
// sees key j iff j ≤ pos and the CSR block layout lists 64-block (pos / 64, j / 64): the decode call's rule, word for word.
// Forward only.  q and out are of one type T ∈ {bf16, fp16} (2-byte bit patterns at the C-ABI); the cache holds T or e4m3fn.
//
// What it computes (contract of include/mi_spmm.h, mi_block_attention_prefill_* — DESIGN.md §3.27):
//  * The training forward, placed in the cache.  A workgroup owns one POSITION TILE of one query head: the positions
//    [64r, 64r + 64) of layout row r that fall inside the item's [k_len − T, k_len).  Own row i of the tile is position
//    64r + i, that is q row t = 64r + i − (k_len − T); k_len − T need not be a multiple of 64, so the first and the last tile
//    of an item are partial.  The tile walks the list of layout row r in list order, skips listed blocks J > r, masks the
//    diagonal block by position and the keys ≥ k_len as LENS masks them — block_attention_fwd_kernel<T, D, true, true>
//    (block_attention.hip) statement for statement: the score MFMAs from the LDS row image, the online softmax, pack_tile,
//    accumulate, group_max / group_sum, one accumulator per element, one rounding at the store.  For a cache whose seen
//    table entries are in range, out and lse rows of existing tokens have the bits of that kernel with q_lens = k_lens on
//    the gathered (widened) cache and q scattered to its positions.  The bits of a row depend on its item's operands, its
//    list and pos: never on T, new_lens, B, the neighbours or the launch.
//  * Slot t holds a token iff t ≥ T − clamp(new_lens[b], 0, T) and pos ≥ 0.  A slot without a token is a zero fragment, never
//    an MFMA operand; its out row is zero and its lse −inf, as for a token that sees nothing; no walk is spent on a tile
//    without a token.  Every row of out is written exactly once by the launch: slot t belongs to tile
//    ⌊pos / 64⌋ − ⌊(k_len − T) / 64⌋ ∈ [0, ⌈T / 64⌉], so ⌈T / 64⌉ + 1 tiles per item from the shape alone.
//  * Nothing outside is read: the cache through its own strides, q through its own; a block outside the list, a block above
//    the diagonal, rows at or beyond k_len (staged as zeros), the gaps between rows and pages whose table entry lies outside
//    [0, P) are never loaded.  Such an entry hides its page's keys (§3.19).  Offsets are clamped to nnz, a column outside
//    the grid is skipped.
//  * fp8 (§3.20): a lane loads the 8 bytes of its 8 elements and widens them on the way into LDS (exact); both images hold
//    T.  A score is multiplied by scale · k_scale[h], one fp32 product taken once per workgroup; with a v_scale the stored
//    element is T::down((O · inv) · v_scale[h]), the product an fp32 value of its own before it is narrowed (§3.20's guard).
//    Without a v_scale the store is the training kernel's statement, so an fp8 call without scales has the bits of the
//    2-byte call on the widened cache.
//
// Kernel: a 1-d grid over (k / v item, tile, query head of the group), 256 threads, an item loop beyond the grid.  The G
// heads of one (item, k / v head, tile) walk the same tiles; they stand 8 workgroups apart (work unit u = 8G·a + 8g + s is
// head g of slot 8a + s, a slot one (item, tile)), where the guide observes — and does not promise — a shared L2.
// Staging is the training kernel's double-buffered tile into Ks and Vt, its rows addressed through the cache form
// (block_attention_cache_device.h: contiguous / pages ≥ 64 / pages of 16, 32 keys — there a lane's four rows lie in one
// page, 4 divides 16); the table is read one list entry ahead.  Tile, store_own and next_block are copies of
// block_attention.hip's private pieces with the cache form added; kB, the images' strides, score, pack_tile, accumulate,
// group_max / group_sum are block_attention_device.h's; mfma<T>, half_of, store_rc mfma_device.h's.  Host side: what a reading
// entry checks and fills alike here and in block_attention_decode.hip is block_attention_cache_device.h's (§3.31); prefill_entry
// keeps split, new_lens, q's strides, the workspace of the parts and the tiles' counts.
//
// Split walks (mi_block_attention_prefill_split_* — DESIGN.md §3.28), for a short chunk behind a long cache: the list of a
// tile's layout row is cut by list position into parts of `split` entries.  There is ONE walk, prefill_walk<…, SPLIT>:
// block_attention_prefill_kernel and block_attention_prefill_split_kernel are shells around it.  SPLIT gives every (work unit,
// part) a workgroup over the part's entries, which leaves a tile without a token to the combine launch and stores the partial
// (o, m, l) of its 64 rows where the unsplit walk normalises and stores out and lse.  block_attention_prefill_combine_kernel
// merges the parts in ascending order and makes the unsplit store (store_row).  What the three kernels must agree on — the
// tile's geometry (Geom), the clamped list range, the part count of a list — is said once, above the walk.
//
// Lists in the place of a layout (mi_block_attention_lists_prefill{,_paged}{,_fp8}_* — DESIGN.md §3.33): the list of tile x of
// k / v item c is the first clamp(block_counts[c·X + x], 0, K) entries of row c·X + x of block_ids [items][X][K], X = ⌈T / 64⌉ + 1 —
// the output of block_select_tiles.hip, or anyone's.  prefill_walk<…, LISTS> is the same walk: listed_range() stands where
// list_range() stands, every statement after the two bounds of the list is shared, so a list has the bits of the layout row that
// lists the same blocks in the same order.  block_attention_prefill_lists_kernel is the third shell; what it adds to Args
// travels beside it (ListArgs).  Unsplit only: a list has K entries.
//
// Sliding windows and sink keys (mi_block_attention_window_prefill{,_lists}{,_paged}{,_fp8}_* — DESIGN.md §3.35): with a window W ≥ 1 and
// S ≥ 0 sink keys the own row at pos sees key j iff the rule above holds and (j > pos − W or j < S).  prefill_walk<…, WINDOW> is the same
// walk with two additions: a test per element behind the diagonal's — the rows of a tile have different edges; under a uniform branch,
// in the blocks that reach behind the window of the tile's last position — and next_block_window,
// which skips a listed block that lies wholly in [S, 64 r − W], hidden from every position the tile can hold: never loaded.
// block_attention_prefill_window_kernel<…, LISTS> is the fourth shell, over either list source, reading new_lens at run time as the
// lists kernel does (so NEWLENS does not double it); what it adds to Args travels beside it (WindowArgs).  Unsplit only.  The walks
// without a window keep their statements — next_block is untouched — and with them their registers.
#include <type_traits>

#include "block_attention_cache_device.h"

namespace {

constexpr int kSpreadHeads = 8;      // workgroups between two heads of a group on one (item, tile)
constexpr long kMaxGrid = 1L << 16;  // workgroups of a launch: work units beyond are served by the item loop

struct Args {
  const int32_t* rowptr;  // [layouts][blocks + 1], with the layouts' bases
  const int32_t* col;     // [nnz], layout-local block columns
  long nnz;
  int layouts, blocks;  // blocks = Smax / 64
  int heads;            // k / v heads per batch item: k / v item c is head c % heads of batch item c / heads
  int group, T, tiles;  // tiles = ⌈T / 64⌉ + 1 position tiles per item
  long smax;
  long slots, units;  // slots = items · tiles; units = ⌈slots / 8⌉ · 8 · group
  const uint16_t* q;  // query head g of k / v item c, token t: q + (c / heads) · batchQ + ((c % heads) · group + g) · headQ + t · ldq
  long ldq, headQ, batchQ;
  const void *k, *v;  // the cache, as in block_attention_decode.hip
  long ldk, headK, batchK, ldv, headV, batchV;
  const int32_t* k_lens;  // [items / lens_div], clamped to [0, Smax] where read
  int lens_div;
  const int32_t* new_lens;  // [B] or [1], clamped to [0, T] where read; null (NEWLENS false): T
  int new_lens_one;         // one entry for all batch items
  float scale;
  uint16_t* out;  // query item c · group + g, token t: out + (c · group + g) · strideO + t · ldo
  long ldo, strideO;
  float* lse;  // [items · group][T]
  const int32_t* table;
  long table_ld;
  int pages, page_shift;
  long pageK, pageV;
  const float *k_scale, *v_scale;
  int k_scale_count, v_scale_count;
};

// One 64 × D block of the cache in registers: unit u = tid < 2D holds rows 4(u & 15) … + 3, columns 8(u >> 4) … + 7 — 16 bytes
// of T or 8 e4m3fn bytes a row.  Rows at or beyond `limit` (the part of the block beyond the item's length) and the rows of a
// page outside the pool are zero rows, whatever memory holds.
template <int D, class F, class E, int FORM>
struct Tile {
  F v[4];
  // `src`: the cache or pool at the item's head; J: the block; e, ok: its table entries and their validity (paged forms)
  __device__ __forceinline__ void load(const E* src, long ld, long pageStride, int J, const int (&e)[4], unsigned ok, int in_page,
                                       int tid, int limit) {
    if (tid < 2 * D) {
      const int row = 4 * (tid & 15);
      const E* p;
      bool valid = true;
      if constexpr (FORM == kContiguous) {
        p = src + ((long)J * kB + row) * ld + 8 * (tid >> 4);
      } else if constexpr (FORM == kPaged) {
        p = src + (long)e[0] * pageStride + (long)(((J * kB) & in_page) + row) * ld + 8 * (tid >> 4);
        valid = ok != 0;
      } else {  // the lane's four rows lie in fragment row / 16, so in one page
        const int f = (tid & 15) >> 2;
        const int mine = f == 0 ? e[0] : f == 1 ? e[1] : f == 2 ? e[2] : e[3];
        p = src + (long)mine * pageStride + (long)(row & in_page) * ld + 8 * (tid >> 4);
        valid = (ok >> f) & 1u;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (valid && row + i < limit)
          v[i] = *reinterpret_cast<const F*>(p + i * ld);
        else
          v[i] = zero_frag<F>();
      }
    }
  }
  // the row image [64][D + 8], in T
  template <class T>
  __device__ __forceinline__ void store_rows(unsigned short* R, int tid) const {
    if (tid < 2 * D) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(R + (4 * (tid & 15) + i) * (D + 8) + 8 * (tid >> 4)) = widen<T>(v[i]);
    }
  }
  // the transposed image [D][64 + 8], in T: the unit is store_rc's, the walk rows its k
  template <class T>
  __device__ __forceinline__ void store_transposed(unsigned short* Tt, int tid) const {
    if (tid < 2 * D) {
      const uint4 x[4] = {widen<T>(v[0]), widen<T>(v[1]), widen<T>(v[2]), widen<T>(v[3])};
      store_rc(Tt, x, tid);
    }
  }
};

// The stored element of the training kernel's statement T::down(x · mul), AS ITS KERNELS HOLD IT.  For float16 the compiler
// makes the product and the narrowing of block_attention_fwd_kernel ONE v_fma_mixlo_f16 — a single rounding of the exact
// product, in all D / 4 stores of a lane (read from that unit's assembly; §3.20 met the same fold in the decode walk).  Left
// to the compiler here, the 2-byte kernels were folded likewise but the fp8 kernels only in part (30 of 32 stores at D = 128),
// which broke "an fp8 call without scales has the bits of the 2-byte call" in float16.  So the instruction is written out:
// the bits do not depend on the compiler's choice in this unit.  bfloat16 has no such instruction and is never folded.
template <class T>
__device__ __forceinline__ unsigned down_product(float x, float mul) { return T::down(x * mul); }
template <>
__device__ __forceinline__ unsigned down_product<F16>(float x, float mul) {
  unsigned r;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(r) : "v"(x), "v"(mul));  // (writes the low half only)
  return r & 0xffffu;
}

// rows [d][own row] → the lane's own row `row`, columns 16fd + 4lg … + 3, each value times `mul`, rounded once
template <class T, int D>
__device__ __forceinline__ void store_own(const f32x4 (&acc)[D / 16], float mul, uint16_t* row, int lg) {
#pragma unroll
  for (int fd = 0; fd < D / 16; ++fd) {
    const f32x4 x = acc[fd];
    *reinterpret_cast<uint2*>(row + 16 * fd + 4 * lg) =
        uint2{down_product<T>(x[0], mul) | (down_product<T>(x[1], mul) << 16), down_product<T>(x[2], mul) | (down_product<T>(x[3], mul) << 16)};
  }
}

// … times `vs`, an fp8 cache's v_scale: the last product is an fp32 value of its own before it is narrowed (DESIGN.md §3.20:
// left alone, the product and the narrowing to float16 become one v_fma_mixlo_f16, which rounds the exact product once)
template <class T, int D>
__device__ __forceinline__ void store_own_scaled(const f32x4 (&acc)[D / 16], float mul, float vs, uint16_t* row, int lg) {
#pragma unroll
  for (int fd = 0; fd < D / 16; ++fd) {
    f32x4 x = acc[fd];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float y = (x[r] * mul) * vs;
      asm("" : "+v"(y));  // (no instruction)
      x[r] = y;
    }
    *reinterpret_cast<uint2*>(row + 16 * fd + 4 * lg) = uint2{pack2<T>(x[0], x[1]), pack2<T>(x[2], x[3])};
  }
}

// the next listed block at or after p that is computed: inside the grid cut to the item's length, not above the diagonal
__device__ __forceinline__ int next_block(const int32_t* col, int p, int end, int own_block, int walk_blocks) {
  for (; p < end; ++p) {
    const int j = col[p];
    if ((unsigned)j >= (unsigned)walk_blocks) continue;
    if (j > own_block) continue;
    break;
  }
  return p;
}
// … under a window: nor wholly behind the window of every position the tile can hold — the keys
// [64j, 64j + 64) ⊂ [sink, edge), edge = 64 · own_block − window + 1 the first key that the window of the tile's first position
// shows.  (A function of its own: the walks without a window keep their statements, and with them their registers.)
__device__ __forceinline__ int next_block_window(const int32_t* col, int p, int end, int own_block, int walk_blocks, int edge, int sink) {
  for (; p < end; ++p) {
    const int j = col[p];
    if ((unsigned)j >= (unsigned)walk_blocks) continue;
    if (j > own_block) continue;
    if ((long)j * kB >= sink && (long)j * kB + kB <= edge) continue;
    break;
  }
  return p;
}

// What the split launches add to Args.  The unsplit kernel's argument stays as it was.
struct SplitArgs {
  Args a;
  int split, parts;  // list entries of a part; parts = ⌈blocks / split⌉ > 1, the parts of a full list
  float* ws;         // [items · group][tiles][parts] partials of 64 · (D + 2) floats: o [64][D], then m [64], then l [64]
};

// Position tile x of k / v item c (of batch item bi) as thread (w, li) on own row 16w + li sees it: what the walks and the
// combine launch must agree on, said once.
struct Geom {
  int klen;      // the item's length, clamped to [0, Smax]
  int start;     // the position of slot 0 (negative: slots without a token)
  int first;     // the existing tokens stand at [first, klen)
  int r;         // the tile's layout row: ⌊start / 64⌋ + x
  int pos;       // the own row's position …
  long t;        // … and its slot
  bool slot_ok;  // the row is a row of q and out
  bool token;    // … that holds a token (pos < k_len follows from t < T)
  bool any;      // the tile holds a token; then 0 ≤ r < blocks: 64r + 63 ≥ first ≥ 0 and 64r < k_len ≤ Smax
};

// `newlens`: a.new_lens is read (the walks' NEWLENS, a compile-time constant there); without it every slot ≥ −start has a token
__device__ __forceinline__ Geom geometry(const Args& a, bool newlens, int c, int bi, int x, int w, int li) {
  Geom g;
  const int klen = a.k_lens[c / a.lens_div];
  g.klen = klen < 0 ? 0 : klen > a.smax ? (int)a.smax : klen;
  int n = a.T;  // the item's new tokens: they stand in the last n of the T slots
  if (newlens) {
    n = a.new_lens[a.new_lens_one ? 0 : bi];
    n = n < 0 ? 0 : n > a.T ? a.T : n;
  }
  g.start = g.klen - a.T;
  g.first = g.klen - n < 0 ? 0 : g.klen - n;
  g.r = (g.start >> 6) + x;
  g.pos = g.r * kB + 16 * w + li;
  g.t = (long)g.pos - g.start;
  g.slot_ok = g.t >= 0 && g.t < a.T;
  g.token = g.slot_ok && g.pos >= g.first;
  g.any = g.first < g.klen && g.r * kB + kB > g.first && g.r * kB < g.klen;
  return g;
}

// the list of layout row r of k / v item c as positions [beg, end) of col, clamped to [0, nnz]
struct ListRange {
  long beg, end;
};
__device__ __forceinline__ ListRange list_range(const Args& a, int c, int r) {
  const int32_t* rp = a.rowptr + (long)(c % a.layouts) * (a.blocks + 1);
  const long beg = rp[r], end = rp[r + 1];
  return {beg < 0 ? 0 : beg, end > a.nnz ? a.nnz : end};
}

// What the list entries add to Args: the caller's lists in the place of the layout.  a.col is block_ids
// [items][tiles][list_k], a.nnz its entries, a.rowptr null.  The unsplit kernel's argument stays as it was.
struct ListArgs {
  Args a;
  const int32_t* counts;  // block_counts [items][tiles]
  int list_k;             // K, the entries of a row of block_ids
};

// … and the list of tile x of k / v item c there: the first clamp(counts, 0, K) entries of row c · tiles + x, so inside col
// whatever counts holds
__device__ __forceinline__ ListRange listed_range(const Args& a, const int32_t* counts, int list_k, int c, int x) {
  const long row = (long)c * a.tiles + x;
  int n = counts[row];
  n = n < 0 ? 0 : n > list_k ? list_k : n;
  return {row * list_k, row * list_k + n};
}

// The parts of a list cut every `split` entries — part i holds the positions [beg + i · split, min(end, beg + (i + 1) · split))
// — of which the first `parts` have a place in the workspace (a malformed rowptr cannot index past it).  A walk workgroup
// whose part is not below this count leaves before any load, barrier or store; the combine launch merges exactly these.
__device__ __forceinline__ int list_parts(const ListRange& ls, int split, int parts) {
  if (ls.end <= ls.beg) return 0;
  const unsigned np = (unsigned)(ls.end - ls.beg - 1) / (unsigned)split + 1u;  // (0 < end − beg ≤ nnz < 2³¹, split ≥ 1)
  return np < (unsigned)parts ? (int)np : parts;
}

// The unsplit store of own row gm.t of query item `item` (head h of its k / v item) from the sums (o, m, l) of its walk, made
// by the unsplit walk and by the combine launch: normalised, with `scaled` through an fp8 cache's v_scale; lse beside it.
template <class T, int D>
__device__ __forceinline__ void store_row(const Args& a, const Geom& gm, long item, int h, bool scaled, const f32x4 (&o)[D / 16],
                                          float m, float l, int lg) {
  const float inv = l == 0.f ? 0.f : 1.f / l;
  if (gm.slot_ok) {
    uint16_t* orow = a.out + item * a.strideO + gm.t * a.ldo;
    if (scaled)
      store_own_scaled<T, D>(o, inv, head_scale(a.v_scale, a.v_scale_count, h), orow, lg);
    else
      store_own<T, D>(o, inv, orow, lg);
    if (lg == 0) a.lse[item * a.T + gm.t] = l == 0.f ? -INFINITY : m + __logf(l);
  }
}

// The walk of both launches.  Without SPLIT a work unit u is one (item, tile, head) and walks its whole list; its epilogue is
// store_row, and a tile without a token stores the zero rows of the slots it owns.  With SPLIT a work unit is (u, part) and
// walks the list positions of its part; a tile without a token, and a part beyond the list's count, leave at once — the
// combine launch writes those rows —, and the epilogue stores the partial (o, m, l) of the 64 own rows into `ws`.
// LISTS (unsplit only): the list is the caller's, row (c, x) of block_ids, where the layout gives row r of its CSR lists —
// the two bounds of the list are all that differs; a.new_lens is looked at when it is there, whatever NEWLENS says.
// WINDOW (unsplit only): the own row at pos sees key j iff the rule above holds and (j > pos − window or
// j < sink) — a test per element beside the diagonal's, the rows of a tile having different edges —, and a listed block that
// no position of the tile can see is skipped by next_block and never loaded.  new_lens is looked at as LISTS looks at it.
template <class TC, int D, int FORM, bool NEWLENS, bool SPLIT, bool LISTS = false, bool WINDOW = false>
__device__ __forceinline__ void prefill_walk(const Args& a, int split, int parts, float* ws, const int32_t* counts = nullptr,
                                             int list_k = 0, [[maybe_unused]] int window = 0x7fffffff, [[maybe_unused]] int sink = 0) {
  static_assert(!(WINDOW && SPLIT), "a windowed row's list is short: no split walks");
  typedef typename Operand<TC>::type T;
  constexpr bool FP8 = Operand<TC>::fp8;
  typedef typename Cache<FP8>::elem E;
  typedef typename Cache<FP8>::frag F;
  __shared__ __attribute__((aligned(16))) unsigned short Ks[kB * (D + 8)];
  __shared__ __attribute__((aligned(16))) unsigned short Vt[D * kTStr];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int G = a.group;
  const int in_page = FORM == kContiguous ? 0 : (1 << a.page_shift) - 1;
  const long total = SPLIT ? a.units * parts : a.units;
  for (long uu = blockIdx.x; uu < total; uu += gridDim.x) {
    // the parts of a work unit stand `units` workgroups apart, so the heads of a group keep their distance of 8
    const long u = SPLIT ? uu % a.units : uu;
    const int part = SPLIT ? (int)(uu / a.units) : 0;
    // the G heads of a slot stand 8 work units apart
    const long slot = u / ((long)kSpreadHeads * G) * kSpreadHeads + (u & (kSpreadHeads - 1));
    if (slot >= a.slots) continue;  // (the padding of the last eight)
    const int g = (int)((u / kSpreadHeads) % G);
    const int c = (int)(slot / a.tiles), x = (int)(slot - (long)c * a.tiles);
    const int bi = c / a.heads, h = c - bi * a.heads;
    const Geom gm = geometry(a, LISTS || WINDOW ? a.new_lens != nullptr : NEWLENS, c, bi, x, w, li);
    const int klen = gm.klen, r = gm.r;
    const long item = (long)c * G + g;
    if (!gm.any) {  // nothing to walk: the zero rows of the slots it owns, if any
      if (!SPLIT && gm.slot_ok) {
        uint16_t* orow = a.out + item * a.strideO + gm.t * a.ldo;
#pragma unroll
        for (int fd = 0; fd < D / 16; ++fd) *reinterpret_cast<uint2*>(orow + 16 * fd + 4 * lg) = uint2{0u, 0u};
        if (lg == 0) a.lse[item * a.T + gm.t] = -INFINITY;
      }
      continue;
    }
    // (a pool has no batch stride: the item's pages come from its table row)
    const E* K = static_cast<const E*>(a.k) + (FORM == kContiguous ? (long)bi * a.batchK : 0L) + (long)h * a.headK;
    const E* V = static_cast<const E*>(a.v) + (FORM == kContiguous ? (long)bi * a.batchV : 0L) + (long)h * a.headV;
    const int32_t* trow = FORM == kContiguous ? nullptr : a.table + (long)bi * a.table_ld;
    // what multiplies a score: scale, or in the fp8 forms scale · k_scale[h] — one fp32 product per workgroup
    const float sc = FP8 ? a.scale * head_scale(a.k_scale, a.k_scale_count, h) : a.scale;
    const int kblocks = (klen + kB - 1) / kB;
    ListRange ls;
    if constexpr (LISTS)
      ls = listed_range(a, counts, list_k, c, x);
    else
      ls = list_range(a, c, r);
    if (SPLIT) {  // the part's entries, cut by list position
      if (part >= list_parts(ls, split, parts)) continue;
      ls.beg += (long)part * split;
      ls.end = ls.end - ls.beg > split ? ls.beg + split : ls.end;
    }
    const int pend = (int)ls.end;

    uint4 qf[D / 32];  // the wave's 16 own rows as B fragments: lane (li, lg) holds columns 32s + 8lg … + 7 of row li
#pragma unroll
    for (int s = 0; s < D / 32; ++s) qf[s] = uint4{0u, 0u, 0u, 0u};
    if (gm.token) {
      const uint16_t* qrow = a.q + (long)bi * a.batchQ + ((long)h * G + g) * a.headQ + gm.t * a.ldq;
#pragma unroll
      for (int s = 0; s < D / 32; ++s) qf[s] = *reinterpret_cast<const uint4*>(qrow + 32 * s + 8 * lg);
    }
    f32x4 o[D / 16];
#pragma unroll
    for (int fd = 0; fd < D / 16; ++fd) o[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // The tile whose loads are in flight (J, its table entries e, their validity ok) and the entry after it (pn, Jn, en): the
    // column and the table entries of an entry are read ONE ENTRY AHEAD, right after the loads of the entry before it were
    // issued, so the chain col[p] → table → tile never stands in front of a tile's loads.
    Tile<D, F, E, FORM> tk, tv;
    int J = 0, Jn = 0, pn = pend, e[4] = {0, 0, 0, 0}, en[4] = {0, 0, 0, 0};
    unsigned ok = 0xfu;
    auto issue = [&]() {
      tk.load(K, a.ldk, a.pageK, J, e, ok, in_page, tid, klen - J * kB);
      tv.load(V, a.ldv, a.pageV, J, e, ok, in_page, tid, klen - J * kB);
    };
    auto look_ahead = [&](int from) {
      if constexpr (WINDOW)  // (the tile skips the blocks inside [sink, 64r − window]; r ≥ 0, window ≥ 1: an int32)
        pn = next_block_window(a.col, from, pend, r, kblocks, r * kB - window + 1, sink);
      else
        pn = next_block(a.col, from, pend, r, kblocks);
      if (pn < pend) {
        Jn = a.col[pn];
        if constexpr (FORM != kContiguous) read_pages<FORM>(en, trow, Jn, a.page_shift);
      }
    };
    int p;
    if constexpr (WINDOW)
      p = next_block_window(a.col, (int)ls.beg, pend, r, kblocks, r * kB - window + 1, sink);
    else
      p = next_block(a.col, (int)ls.beg, pend, r, kblocks);
    if (p < pend) {
      J = a.col[p];
      if constexpr (FORM != kContiguous) {
        read_pages<FORM>(e, trow, J, a.page_shift);
        ok = valid_pages(e, a.pages);
      }
      issue();
      look_ahead(p + 1);
    }
    while (p < pend) {
      const int Jc = J;           // the block computed in this turn …
      const unsigned seen = ok;   // … and the fragments of it that lie in a page (paged forms)
      __syncthreads();  // the previous block's reads are done
      tk.template store_rows<T>(Ks, tid);
      tv.template store_transposed<T>(Vt, tid);
      __syncthreads();
      p = pn;
      if (p < pend) {  // the next block's loads are in flight while this one is computed
        J = Jn;
        if constexpr (FORM != kContiguous) {
#pragma unroll
          for (int f = 0; f < 4; ++f) e[f] = en[f];
          ok = valid_pages(e, a.pages);
        }
        issue();
        look_ahead(p + 1);
      }
      const int kleft = klen - Jc * kB;  // keys of this block that exist
      f32x4 s[4];
      score<T, D>(s, Ks, qf, li, lg);
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          float x = s[f][rr] * sc;
          if (Jc == r && 16 * f + 4 * lg + rr > 16 * w + li) x = -INFINITY;
          if (16 * f + 4 * lg + rr >= kleft) x = -INFINITY;
          s[f][rr] = x;
        }
      if constexpr (WINDOW) {
        // keys behind the own row's window that are no sink keys: j ≥ sink and j ≤ pos − window (pos ≥ 0, window ≥ 1: int32s).  A
        // uniform branch: only a block that reaches behind the window of the tile's LAST position, and is not all sink keys, holds
        // one — of a banded list the oldest block or two
        if (Jc * kB <= r * kB + (kB - 1) - window && Jc * kB + (kB - 1) >= sink) {
#pragma unroll
          for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const int j = Jc * kB + 16 * f + 4 * lg + rr;
              if (j >= sink && j <= gm.pos - window) s[f][rr] = -INFINITY;
            }
        }
      }
      if (FORM != kContiguous && seen != 0xfu) {  // keys of a page outside the pool (a uniform branch: tables are in range as a rule)
#pragma unroll
        for (int f = 0; f < 4; ++f)
          if (!((seen >> f) & 1u)) s[f] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
      float mt = -INFINITY;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) mt = fmaxf(mt, s[f][rr]);
      const float mn = fmaxf(m, group_max(mt));
      const float alpha = m == mn ? 1.f : __expf(m - mn);  // (−inf stays: nothing seen yet)
      float sum = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float ex = s[f][rr] == -INFINITY ? 0.f : __expf(s[f][rr] - mn);
          s[f][rr] = ex;
          sum += ex;
        }
      l = l * alpha + sum;  // this lane's share of the row sum; the four shares meet after the walk
      m = mn;
#pragma unroll
      for (int fd = 0; fd < D / 16; ++fd)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) o[fd][rr] *= alpha;
      uint4 pb[2];
      pack_tile<T>(pb, s);
      accumulate<T, D>(o, Vt, pb, li, lg);
    }
    l = group_sum(l);
    if (!gm.token) {
      l = 0.f;
#pragma unroll
      for (int fd = 0; fd < D / 16; ++fd) o[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (SPLIT) {
      // the partial of the own row: an empty one is (−inf, 0) with a zero accumulator (o is zero wherever m is −inf)
      float* wp = ws + (((item * a.tiles + x) * parts + part) * (long)(kB * (D + 2)));
      const int row = 16 * w + li;
#pragma unroll
      for (int fd = 0; fd < D / 16; ++fd) *reinterpret_cast<f32x4*>(wp + row * D + 16 * fd + 4 * lg) = o[fd];
      if (lg == 0) {
        wp[kB * D + row] = l == 0.f ? -INFINITY : m;
        wp[kB * D + kB + row] = l;
      }
    } else {
      store_row<T, D>(a, gm, item, h, FP8 && a.v_scale != nullptr, o, m, l, lg);
    }
    __syncthreads();  // the next work unit restages
  }
}

template <class TC, int D, int FORM, bool NEWLENS>
__global__ __launch_bounds__(256) void block_attention_prefill_kernel(Args a) {
  prefill_walk<TC, D, FORM, NEWLENS, false>(a, 0, 1, nullptr);
}
template <class TC, int D, int FORM, bool NEWLENS>
__global__ __launch_bounds__(256) void block_attention_prefill_split_kernel(SplitArgs sa) {
  prefill_walk<TC, D, FORM, NEWLENS, true>(sa.a, sa.split, sa.parts, sa.ws);
}

template <class TC, int D, int FORM>
__global__ __launch_bounds__(256) void block_attention_prefill_lists_kernel(ListArgs la) {
  prefill_walk<TC, D, FORM, true, false, true>(la.a, 0, 1, nullptr, la.counts, la.list_k);
}

// What the window entries add to Args, for either list source: counts null — the layout —, or the caller's lists
// as in ListArgs.  The other kernels' arguments stay as they were.
struct WindowArgs {
  Args a;
  const int32_t* counts;
  int list_k;
  int window, sink;
};
template <class TC, int D, int FORM, bool LISTS>
__global__ __launch_bounds__(256) void block_attention_prefill_window_kernel(WindowArgs wa) {
  prefill_walk<TC, D, FORM, true, false, LISTS, true>(wa.a, 0, 1, nullptr, wa.counts, wa.list_k, wa.window, wa.sink);
}

// the window of the window_prefill entries
struct Window {
  bool on = false;
  int32_t window = 0x7fffffff, sink = 0;
};

// The second launch of a split call: one workgroup per (query item, tile), thread (w, li, lg) on own row 16w + li as in the
// walk.  The tile's rows, its list and its number of parts are recomputed as the walk computes them; the partials of parts
// [0, n) — exactly those a walk workgroup wrote — are merged in ascending order: M = max mᵢ, wᵢ = 1 if mᵢ == M else exp(mᵢ − M)
// (the walk's alpha statement), L = Σ lᵢ·wᵢ, O = Σ oᵢ·wᵢ, the first part setting the sums (so one part is the walk's values,
// bit for bit).  M and the weights are taken once per row, by the lane with lg == 0, and handed to the row's other three lanes.
// The store is the unsplit kernel's; every out and lse row of the tile's slots is written here and nowhere else.
template <class T, int D>
__global__ __launch_bounds__(256) void block_attention_prefill_combine_kernel(SplitArgs sa) {
  const Args& a = sa.a;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int G = a.group;
  const long total = a.slots * G;
  for (long uu = blockIdx.x; uu < total; uu += gridDim.x) {
    const long item = uu / a.tiles;
    const int x = (int)(uu - item * a.tiles);
    const int c = (int)(item / G);
    const int bi = c / a.heads, h = c - bi * a.heads;
    const Geom gm = geometry(a, a.new_lens != nullptr, c, bi, x, w, li);
    // the parts of the tile's list: those whose workgroup wrote a partial
    const int parts = gm.any ? list_parts(list_range(a, c, gm.r), sa.split, sa.parts) : 0;
    const float* wp = sa.ws + (item * a.tiles + x) * sa.parts * (long)(kB * (D + 2));
    const long pstride = (long)kB * (D + 2);
    const int row = 16 * w + li;
    float M = -INFINITY;
    if (lg == 0)
      for (int i = 0; i < parts; ++i) M = fmaxf(M, wp[i * pstride + kB * D + row]);
    M = __shfl(M, li);
    f32x4 o[D / 16];
#pragma unroll
    for (int fd = 0; fd < D / 16; ++fd) o[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int i = 0; i < parts; ++i) {
      const float* pp = wp + i * pstride;
      float wt = 0.f, lw = 0.f;
      if (lg == 0) {
        const float mi = pp[kB * D + row];
        wt = mi == M ? 1.f : __expf(mi - M);
        lw = pp[kB * D + kB + row] * wt;
      }
      wt = __shfl(wt, li);
      lw = __shfl(lw, li);
      if (i == 0) {
        l = lw;
#pragma unroll
        for (int fd = 0; fd < D / 16; ++fd) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(pp + row * D + 16 * fd + 4 * lg);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) o[fd][rr] = v[rr] * wt;
        }
      } else {
        l += lw;
#pragma unroll
        for (int fd = 0; fd < D / 16; ++fd) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(pp + row * D + 16 * fd + 4 * lg);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) o[fd][rr] += v[rr] * wt;
        }
      }
    }
    if (!gm.token) {  // (its partials are empty: l is 0 already)
      l = 0.f;
#pragma unroll
      for (int fd = 0; fd < D / 16; ++fd) o[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    store_row<T, D>(a, gm, item, h, a.v_scale != nullptr, o, M, l, lg);
  }
}

template <class TC, int D, int FORM>
int launch_form(const Args& a, const SplitArgs& sp, const ListArgs& li, const Window& win, hipStream_t s) {
  if (win.on) {  // a window: one launch over either list source, never split
    const WindowArgs wa = {a, li.counts, li.list_k, win.window, win.sink};
    const dim3 grid((unsigned)(a.units < kMaxGrid ? a.units : kMaxGrid));
    if (li.counts)
      hipLaunchKernelGGL((block_attention_prefill_window_kernel<TC, D, FORM, true>), grid, dim3(256), 0, s, wa);
    else
      hipLaunchKernelGGL((block_attention_prefill_window_kernel<TC, D, FORM, false>), grid, dim3(256), 0, s, wa);
    return mi::check_launch();
  }
  if (li.counts) {  // the list source: one launch, never split
    const ListArgs la = {a, li.counts, li.list_k};
    hipLaunchKernelGGL((block_attention_prefill_lists_kernel<TC, D, FORM>), dim3((unsigned)(a.units < kMaxGrid ? a.units : kMaxGrid)),
                       dim3(256), 0, s, la);
    return mi::check_launch();
  }
  if (sp.parts > 1) {  // the split walk, then the combine: two launches on the one stream, the kernel boundary the hand-over
    typedef typename Operand<TC>::type T;
    const SplitArgs sa = {a, sp.split, sp.parts, sp.ws};
    const long walks = a.units * sp.parts, tiles = a.slots * a.group;
    const dim3 grid((unsigned)(walks < kMaxGrid ? walks : kMaxGrid));
    if (a.new_lens)
      hipLaunchKernelGGL((block_attention_prefill_split_kernel<TC, D, FORM, true>), grid, dim3(256), 0, s, sa);
    else
      hipLaunchKernelGGL((block_attention_prefill_split_kernel<TC, D, FORM, false>), grid, dim3(256), 0, s, sa);
    if (const int st = mi::check_launch()) return st;
    hipLaunchKernelGGL((block_attention_prefill_combine_kernel<T, D>), dim3((unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid)), dim3(256),
                       0, s, sa);
    return mi::check_launch();
  }
  const dim3 grid((unsigned)(a.units < kMaxGrid ? a.units : kMaxGrid));
  if (a.new_lens)
    hipLaunchKernelGGL((block_attention_prefill_kernel<TC, D, FORM, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((block_attention_prefill_kernel<TC, D, FORM, false>), grid, dim3(256), 0, s, a);
  return mi::check_launch();
}

template <class T, int D, bool FP8>
int launch(const Args& a, const SplitArgs& sp, const ListArgs& li, const Window& win, hipStream_t s) {
  typedef std::conditional_t<FP8, Fp8<T>, T> TC;  // the cache element type is part of the kernel's first parameter
  return with_form(a, [&](auto form) { return launch_form<TC, D, decltype(form)::value>(a, sp, li, win, s); });
}

// What the split entries add: the list entries of a part, and the workspace of the partials.
struct Split {
  bool on = false;
  int32_t entries = 0;
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
};

// the caller's lists of the *_lists entries: block_counts [items][tiles] and K, the entries of a row of block_ids
struct Lists {
  const int32_t* counts = nullptr;
  int32_t K = 0;
};

// the parts of a full list of Smax / 64 entries cut every `split`
inline int parts_of(int32_t Smax, int32_t split) { return (int)(((long)Smax / kB + split - 1) / split); }

// Every check comes before the first HIP call.  `r`: what every reading entry takes (block_attention_cache_device.h), FP8 its
// cache type; q, new_lens and `split` — the split entries' cut and workspace; with one part the call is the unsplit launch —
// are this entry's own, and `lists`: the list source (never with split) — `col` is block_ids, nnz its items · tiles · K entries;
// `win`: the window of the window_prefill entries (never with split), over either list source.
template <class T, bool FP8 = false>
int prefill_entry(const ReadCall& r, const uint16_t* q, int64_t ldq, int64_t headQ, int64_t batchQ, const int32_t* new_lens,
                  int32_t new_lens_count, hipStream_t s, const Split& split = Split(), const Lists& lists = Lists(),
                  const Window& win = Window()) {
  if (win.on && (win.window < 1 || win.sink < 0 || split.on)) return MI_EINVAL;
  const bool listed = lists.K != 0 || lists.counts;
  if (listed && (split.on || lists.K < 1 || !lists.counts || !aligned4(lists.counts) || !aligned4(r.col))) return MI_EINVAL;
  if (split.on && split.entries < 1) return MI_EINVAL;
  if (const int st = read_sizes_status(FP8, r)) return st;
  if (read_is_empty(r)) return MI_OK;
  if (!read_operands_ok(FP8, r, listed)) return MI_EINVAL;
  if (new_lens && (!aligned4(new_lens) || (new_lens_count != 1 && new_lens_count != r.items / r.heads))) return MI_EINVAL;
  if (!q || !mi::aligned16(q) || !stride_ok(ldq) || !stride_ok(headQ) || !stride_ok(batchQ) || (r.T > 1 && ldq < r.D)) return MI_EINVAL;
  const int parts = split.on ? parts_of(r.Smax, split.entries) : 1;
  if (parts > 1) {  // (one part: the unsplit launch, no workspace)
    if (!split.workspace || !mi::aligned16(split.workspace)) return MI_EINVAL;
    const int64_t need = mi_block_attention_prefill_split_workspace_bytes(r.items, r.group, r.T, r.D, r.Smax, split.entries);
    if (need < 0) return (int)need;
    if (split.workspace_bytes < (uint64_t)need) return MI_ENOMEM;
  }
  Args a = {};
  SplitArgs sp = {};
  ListArgs li = {};
  if (listed) li.counts = lists.counts, li.list_k = lists.K;
  if (parts > 1) sp.split = split.entries, sp.parts = parts, sp.ws = static_cast<float*>(split.workspace);
  fill_read_args(a, FP8, r);
  a.tiles = (int)(((long)r.T + kB - 1) / kB + 1);
  a.slots = (long)r.items * a.tiles;
  a.units = (a.slots + kSpreadHeads - 1) / kSpreadHeads * kSpreadHeads * r.group;
  a.q = q, a.ldq = ldq, a.headQ = headQ, a.batchQ = batchQ;
  a.new_lens = new_lens, a.new_lens_one = new_lens_count == 1;
  return with_width(r.D, [&](auto d) { return launch<T, decltype(d)::value, FP8>(a, sp, li, win, s); });
}

}  // namespace

extern "C" {

int64_t mi_block_attention_prefill_split_workspace_bytes(int32_t items, int32_t group, int32_t T, int32_t D, int32_t Smax,
                                                         int32_t split) {
  if (items < 0 || group < 1 || T < 0 || !takes_width(D) || Smax < 0 || Smax % kB != 0 || split < 1) return MI_EINVAL;
  const int parts = parts_of(Smax, split);
  if (items == 0 || T == 0 || parts <= 1) return 0;  // (one part: the walk stores out itself)
  int64_t n = (int64_t)items * group;                // < 2^62
  if (__builtin_mul_overflow(n, ((int64_t)T + kB - 1) / kB + 1, &n) || __builtin_mul_overflow(n, (int64_t)parts, &n) ||
      __builtin_mul_overflow(n, (int64_t)kB * (D + 2) * (int64_t)sizeof(float), &n))
    return MI_ERANGE;
  return n;
}

// The 48 entries of the header, two per line of the table below (bf16, f16).  Their parameter lists are the header's pieces:
// the list with the sizes — a LAYOUT's, or the caller's LISTS —, [the table] of a PAGED entry, D, the operands,
// [the scales] of an fp8 entry, and the tail of the entry's form.  What an entry passes on: the reading call, then its own.  The
// list source hands block_ids over as col, its items · (⌈T / 64⌉ + 1) · K entries as nnz, no rowptr and one layout.  (A K that
// is no positive int32 is refused inside, before the product is looked at; T < 0 likewise by the sizes' check.)
#define MI_PREFILL_HEAD_LAYOUT MI_BLOCK_ATTENTION_PREFILL_LIST
#define MI_PREFILL_HEAD_LISTS MI_BLOCK_ATTENTION_PREFILL_LISTS_HEAD
#define MI_PREFILL_TABLE_FLAT
#define MI_PREFILL_TABLE_PAGED MI_BLOCK_ATTENTION_PREFILL_TABLE,
#define MI_PREFILL_SCALES_false
#define MI_PREFILL_SCALES_true MI_BLOCK_ATTENTION_PREFILL_SCALES,
#define MI_PREFILL_CALL_LAYOUT(...) MI_READ_CALL(rowptr, col, nnz, layouts, __VA_ARGS__)
#define MI_PREFILL_CALL_LISTS(...) \
  MI_READ_CALL(nullptr, block_ids, (K < 1 || T < 0) ? 0 : (int64_t)items * (((int64_t)T + kB - 1) / kB + 1) * K, 1, __VA_ARGS__)
#define MI_PREFILL_LISTS_LAYOUT Lists()
#define MI_PREFILL_LISTS_LISTS Lists{block_counts, K < 1 ? -1 : K}
#define MI_PREFILL_OWN q, ldq, headQ, batchQ, new_lens, new_lens_count, static_cast<hipStream_t>(stream)
// The forms, by the token a line ends in — the tail of the parameter list, and what is passed behind the entry's own (LISTS: the
// entry's Lists): PLAIN; SPLIT (§3.28): the cut and the workspace, behind the outputs; WINDOW (§3.35): window ≥ 1 and sink ≥ 0,
// ahead of them.  prefill_entry refuses a split over lists or beside a window.
#define MI_PREFILL_TAIL_PLAIN MI_BLOCK_ATTENTION_PREFILL_OUT
#define MI_PREFILL_TAIL_SPLIT MI_BLOCK_ATTENTION_PREFILL_SPLIT_OUT
#define MI_PREFILL_TAIL_WINDOW int32_t window, int32_t sink, MI_BLOCK_ATTENTION_PREFILL_OUT
#define MI_PREFILL_PASS_PLAIN(LISTS) Split(), LISTS
#define MI_PREFILL_PASS_SPLIT(LISTS) Split{true, split, workspace, workspace_bytes}, LISTS
#define MI_PREFILL_PASS_WINDOW(LISTS) Split(), LISTS, Window{true, window, sink}

#define MI_PREFILL_ENTRY(STEM, TYPE, SUFFIX, HEAD, PAGED, FP8, FORM)                                                            \
  int mi_block_attention_##STEM##SUFFIX(MI_PREFILL_HEAD_##HEAD, MI_PREFILL_TABLE_##PAGED int32_t D,                             \
                                        MI_BLOCK_ATTENTION_PREFILL_OPERANDS(MI_READ_CACHE_##FP8),                               \
                                        MI_PREFILL_SCALES_##FP8 MI_PREFILL_TAIL_##FORM) {                                       \
    return MI_READ_GUARD_##PAGED prefill_entry<TYPE, FP8>(MI_PREFILL_CALL_##HEAD(MI_READ_TABLE_##PAGED, MI_READ_SCALES_##FP8),  \
                                                          MI_PREFILL_OWN, MI_PREFILL_PASS_##FORM(MI_PREFILL_LISTS_##HEAD));     \
  }
// one line of the table: the entry's name stem as the header spells it, the list, the cache's storage, FP8, the form
#define MI_PREFILL_ENTRIES(STEM, HEAD, PAGED, FP8, FORM)       \
  MI_PREFILL_ENTRY(STEM, Bf16, _bf16, HEAD, PAGED, FP8, FORM)  \
  MI_PREFILL_ENTRY(STEM, F16, _f16, HEAD, PAGED, FP8, FORM)

// clang-format off
MI_PREFILL_ENTRIES(prefill,                          LAYOUT, FLAT,  false, PLAIN)
MI_PREFILL_ENTRIES(prefill_paged,                    LAYOUT, PAGED, false, PLAIN)
MI_PREFILL_ENTRIES(prefill_fp8,                      LAYOUT, FLAT,  true,  PLAIN)
MI_PREFILL_ENTRIES(prefill_paged_fp8,                LAYOUT, PAGED, true,  PLAIN)
MI_PREFILL_ENTRIES(prefill_split,                    LAYOUT, FLAT,  false, SPLIT)
MI_PREFILL_ENTRIES(prefill_split_paged,              LAYOUT, PAGED, false, SPLIT)
MI_PREFILL_ENTRIES(prefill_split_fp8,                LAYOUT, FLAT,  true,  SPLIT)
MI_PREFILL_ENTRIES(prefill_split_paged_fp8,          LAYOUT, PAGED, true,  SPLIT)
// (the names put `lists` first: `mi_block_attention_prefill…` was a closed family when these came)
MI_PREFILL_ENTRIES(lists_prefill,                    LISTS,  FLAT,  false, PLAIN)
MI_PREFILL_ENTRIES(lists_prefill_paged,              LISTS,  PAGED, false, PLAIN)
MI_PREFILL_ENTRIES(lists_prefill_fp8,                LISTS,  FLAT,  true,  PLAIN)
MI_PREFILL_ENTRIES(lists_prefill_paged_fp8,          LISTS,  PAGED, true,  PLAIN)
MI_PREFILL_ENTRIES(window_prefill,                   LAYOUT, FLAT,  false, WINDOW)
MI_PREFILL_ENTRIES(window_prefill_paged,             LAYOUT, PAGED, false, WINDOW)
MI_PREFILL_ENTRIES(window_prefill_fp8,               LAYOUT, FLAT,  true,  WINDOW)
MI_PREFILL_ENTRIES(window_prefill_paged_fp8,         LAYOUT, PAGED, true,  WINDOW)
MI_PREFILL_ENTRIES(window_prefill_lists,             LISTS,  FLAT,  false, WINDOW)
MI_PREFILL_ENTRIES(window_prefill_lists_paged,       LISTS,  PAGED, false, WINDOW)
MI_PREFILL_ENTRIES(window_prefill_lists_fp8,         LISTS,  FLAT,  true,  WINDOW)
MI_PREFILL_ENTRIES(window_prefill_lists_paged_fp8,   LISTS,  PAGED, true,  WINDOW)
// clang-format on

}  // extern "C"
