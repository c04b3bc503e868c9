// Block-sparse attention for decoding in bfloat16 and float16 on the matrix cores: the T newest tokens of every item
// against a key / value cache, out = softmax(scale · q·kᵀ + mask) · v, where token t of an item of length k_len stands at
// pos = k_len − T + t and sees key j iff j ≤ pos and the CSR block layout lists 64-block (pos / 64, j / 64).  Forward
// only.  q, k, v and out are of one type T ∈ {bf16, fp16} (2-byte bit patterns at the C-ABI).
//
// What it computes (contract of include/mi_spmm.h, mi_block_attention_decode_{bf16,f16} — DESIGN.md §3.18):
//  * The arithmetic of block_attention_fwd_kernel (block_attention.hip): v_mfma_f32_16x16x32_{bf16,f16} with fp32
//    accumulators, scores, maxima and sums in fp32 as lane scalars, P narrowed to T only as the operand of P·V, out rounded
//    once at the final store.  The own rows of a workgroup are the `group` query heads of one (item, k / v head, token) in
//    ONE 16-row tile (rows ≥ group are zero fragments and never stored): a k / v tile is read once for the whole group.
//  * The order of summation: the list of layout row pos / 64 is cut into chunks of `chunk` consecutive entries BY LIST
//    POSITION (entry p belongs to chunk (p − beg) / chunk; an entry outside the grid or wholly beyond pos is skipped inside
//    its chunk and does not move the cut).  A workgroup owns one chunk; wave w walks its entries w, w + 4, … in order, and
//    the four waves' partials (running maximum m, sum l, unnormalised fp32 accumulator) are merged in ascending wave order:
//    M = max m_i, l = Σ l_i·exp(m_i − M), o likewise; an empty partial is (−inf, 0, 0).  The chunks' partials are merged the
//    same way in ascending chunk order by block_attention_decode_combine_kernel — or, with one chunk, stored at once by
//    the first kernel with the same arithmetic.  The bits of an output row depend on its own item's operands, its list,
//    pos and chunk only: never on the batch, the neighbours or the launch.  No atomics, no read-back: graph-capturable.
//  * Nothing outside is read: the cache is read through its own row, head and batch strides; a block outside the list, a
//    key beyond pos (so every key at or beyond k_len) and everything between the rows are never loaded; the rows of a
//    straddling block beyond pos are staged as zeros, their scores masked to −inf.  Offsets are clamped to nnz, a column
//    outside the grid is skipped: a malformed layout reads nothing outside the operands.
//
//  * Paged caches (mi_block_attention_decode_paged_{bf16,f16}): k and v are one pool of pages of 2^s ≥ 16 keys
//    and a block table per batch item names the pool page of each logical page; the walk's tile addressing is a compile-time
//    form of the kernel (contiguous / pages ≥ 64 keys / pages of 16 or 32 keys), everything else is shared.  A table entry
//    outside the pool hides its page's keys: nothing is loaded for them, zeros are staged, their scores are −inf.
//
//  * fp8 caches (mi_block_attention_decode{,_paged}_fp8_{bf16,f16}): k and v (or the pool) hold OCP e4m3fn
//    bytes and a float32 scale per k / v head (or one for all).  The cache element type is a compile-time form of the walk:
//    a lane loads the 8 bytes of its 8 elements where the 2-byte walk loads 16, and widens them to T in registers
//    (v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1: exact, every finite e4m3fn code is a T) — k right before the score
//    MFMAs, v on its way into the transposed image, which holds T as before.  From there the statements are the same, but
//    for two: a score is multiplied by scale · k_scale[h] (ONE fp32 product, taken once per workgroup) and the stored
//    element is T::down((O · inv) · v_scale[h]).  So without scales the call has the bits of the 2-byte call on the widened
//    cache.  The scales are read from device memory by the kernels: never read back, graph-capturable.
//
//  * Lists in the place of a layout (mi_block_attention_decode_lists{,_paged}_{bf16,f16}, DESIGN.md §3.29, and over an fp8 cache
//    mi_block_attention_lists_decode{,_paged}_fp8_{bf16,f16}, §3.32): the list of token t of
//    k / v item c is the first clamp(block_counts[c · T + t], 0, K) entries of row c · T + t of the caller's block_ids — what
//    block_select.hip writes —, the chunks are counted over the K list positions, and everything after the list's two bounds is
//    the same statements: the bits of the layout row that lists the same blocks in the same order.
//
//  * Tree masks (mi_block_attention_tree_decode{,_lists}{,_paged}{,_fp8}_{bf16,f16}): the T new tokens are the nodes
//    of a drafted tree in the window [base, base + T), base = clamp(k_len, 0, Smax) − T; token t sees key j iff the rule above
//    holds and (j < base, or j == pos, or bit j − base of its int64 word tree_mask[b][t] is set).  A compile-time form of the
//    kernel's first parameter — Tree<…> around either list source: a hidden key is treated like a key beyond pos (never loaded,
//    staged as zeros, its score −inf), everything else is the same statements, so the word (2 << t) − 1 gives the plain call's bits.
//
//  * Sliding windows and sink keys (mi_block_attention_window_decode{,_lists}{,_paged}{,_fp8}_{bf16,f16}): with a window
//    W ≥ 1 and S ≥ 0 sink keys the token at pos sees key j iff the rule above holds and (j > pos − W or j < S) — W counts the token
//    itself.  The hide word's second source: in tile J the bits [max(S − 64 J, 0), min(pos − W + 1 − 64 J, 64)), made in scalar
//    registers, are OR-ed to the tree word, so a hidden key is again never loaded, staged as zeros, its score −inf; a listed block
//    that lies wholly in [S, pos − W] is skipped by next_entry like a block beyond pos and keeps its list position.  The entries run
//    on the Tree<…> kernels with a null mask ("no tree": H = 0, T not bound to 64); the tree entries pass W = 2³¹ − 1, S = 0, whose
//    range is empty.  No new instantiation.
//
// Kernel: grid (chunks, items, T), 256 threads.  No workgroup barrier inside the walk.  A wave loads the k tile of an
// entry as 16-byte global loads straight into MFMA A fragments (lane (li, lg): row 16f + li, columns 32s + 8lg … + 7), the v
// tile into registers and from there into a wave-private transposed LDS image [D][64 + 8] (a wave-level fence between its
// writes and reads); the next entry's loads are issued before this one's softmax and P·V.  kB, the image's stride,
// pack_tile, accumulate and group_max / group_sum are block_attention_device.h's, which block_attention.hip shares (the walk
// rows are the keys here); mfma<T> and half_of are mfma_device.h's; what is said about the cache is
// kv_cache_device.h's (§3.23), what is said about a walk over it — Fp8 / Operand / Cache, widen, the forms, read_pages,
// valid_pages — block_attention_cache_device.h's, which block_attention_prefill.hip shares (§3.27).  `score` is this unit's
// own: its k fragments come from registers.  Host side: what a reading entry checks and fills alike in both units — ReadCall,
// read_sizes_status, read_operands_ok, fill_read_args, with_width, with_form — is that header's too (§3.31); decode_entry keeps
// the lists' rules, group ≤ 16, chunk, the grid's bounds, q and the workspace.
#include <type_traits>

#include "block_attention_cache_device.h"

namespace {

constexpr int kWaves = 4;      // waves of a workgroup: wave w walks entries w, w + 4, … of the chunk
constexpr int kMaxGroup = 16;  // own rows of the one MFMA tile

// the list source as a form of the kernel's first parameter: TC itself — a CSR layout over a cache of TC — or Listed<TC>
template <class TC>
struct Listed {};
template <class TS>
struct Source {
  typedef TS cache;
  static constexpr bool lists = false;
  static constexpr bool tree = false;
};
template <class TC>
struct Source<Listed<TC>> {
  typedef TC cache;
  static constexpr bool lists = true;
  static constexpr bool tree = false;
};
// … and the tree form wraps either: Tree<TC> or Tree<Listed<TC>> — the kernels of the tree_decode entries, whose
// new tokens see the draft keys that their word of tree_mask names; the names of the plain kernels stay as they were
template <class TS>
struct Tree {};
template <class TS>
struct Source<Tree<TS>> {
  typedef typename Source<TS>::cache cache;
  static constexpr bool lists = Source<TS>::lists;
  static constexpr bool tree = true;
};

struct Args {
  const int32_t* rowptr;  // [layouts][blocks + 1], with the layouts' bases
  const int32_t* col;     // [nnz], layout-local block columns
  long nnz;
  int layouts, blocks;    // blocks = Smax / 64
  int heads;              // k / v heads per batch item: k / v item c is head c % heads of batch item c / heads
  int group, T, chunk, chunks;
  long smax;
  const uint16_t* q;      // query item c · group + g, token t: q + (c · group + g) · strideQ + t · ldq
  long ldq, strideQ;
  const void *k, *v;      // key j of k / v item c: k + (c / heads) · batchK + (c % heads) · headK + j · ldk (in elements:
                          // 2-byte patterns of T, or e4m3fn bytes in the fp8 forms)
  long ldk, headK, batchK, ldv, headV, batchV;
  const int32_t* k_lens;  // [items / lens_div], clamped to [0, Smax] where read
  int lens_div;
  float scale;
  uint16_t* out;
  long ldo, strideO;
  float* lse;  // [items · group][T]
  float* ws;   // [items][T][chunks][group][D + 2]: m, l, o[D] — read and written only with chunks > 1
  // the paged forms: k and v are pools of pages of 1 << page_shift keys; key j of k / v item c lies at
  // k + table[(c / heads) · table_ld + (j >> page_shift)] · pageK + (c % heads) · headK + (j & (page − 1)) · ldk
  const int32_t* table;  // [items / heads][table_ld]; an entry outside [0, pages) hides the keys of its logical page
  long table_ld;
  int pages, page_shift;
  long pageK, pageV;
  // the fp8 forms: the real key is k8 · k_scale[h], the real value v8 · v_scale[h]; a null pointer is 1,
  // a count of 1 one scale for all heads, else one per k / v head
  const float *k_scale, *v_scale;
  int k_scale_count, v_scale_count;
  // the list source of the *_lists entries: `col` is block_ids [items][T][list_k], the list of token t of
  // item c its first clamp(counts[c · T + t], 0, list_k) entries; rowptr, nnz and layouts are not looked at
  const int32_t* counts;
  int list_k;
  // the tree form of the tree_decode entries: word (b, t) of tree_mask [mask_rows][T] — mask_rows 1: one row for the
  // batch — names the keys of the window [k_len − T, k_len) that token t sees beside itself: bit i < t is key k_len − T + i
  const int64_t* tree_mask;
  int mask_rows;
  // the window of the window_decode entries, looked at by the Tree<…> kernels only: beside its other rules the
  // token at pos sees key j iff j > pos − window or j < sink.  The tree_decode entries pass 2³¹ − 1 and 0: nothing is hidden
  int window, sink;
};

// The hide word of a tile (tree form): bit r is set iff row r of the tile is a draft key that the token does not see.  `hide`
// is 0 in every plain kernel — a constant, so the tests on it fold away there.  A lane looks at its own rows through one
// shift by its lane coordinate; the row's number inside the lane is a constant.
typedef unsigned long long HideWord;
__device__ __forceinline__ bool hidden(HideWord mine, int row) { return (mine >> row) & 1ull; }

__device__ __forceinline__ void fence_wave() {  // LDS writes of this wave before, its reads after
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The k tile of a block as A fragments: lane (li, lg) holds columns 32s + 8lg … + 7 of row 16f + li; rows at or beyond
// `limit` (keys beyond pos) are zero fragments, whatever memory holds
template <int D, class F, class E>
__device__ __forceinline__ void load_k(F (&kf)[4][D / 32], const E* src, long ld, int li, int lg, int limit, HideWord hide) {
  const HideWord mine = hide >> li;  // row 16f + li at bit 16f
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int s = 0; s < D / 32; ++s) {
      if (16 * f + li < limit && !hidden(mine, 16 * f))
        kf[f][s] = *reinterpret_cast<const F*>(src + (long)(16 * f + li) * ld + 32 * s + 8 * lg);
      else
        kf[f][s] = zero_frag<F>();
    }
}

// The v tile of a block in one wave's registers: lane (li, lg) holds rows 4li … + 3, columns 8(lg + 4i) … + 7
template <int D, class F, class E>
__device__ __forceinline__ void load_v(F (&vr)[D / 32][4], const E* src, long ld, int li, int lg, int limit, HideWord hide) {
  const HideWord mine = hide >> (4 * li);  // row 4li + r at bit r
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (4 * li + r < limit && !hidden(mine, r))
        vr[i][r] = *reinterpret_cast<const F*>(src + (long)(4 * li + r) * ld + 8 * (lg + 4 * i));
      else
        vr[i][r] = zero_frag<F>();
    }
}

// load_k over pages of 16 or 32 keys: fragment f (rows 16f … 16f + 15 of the tile) starts at row (16f) & (page − 1) of its
// own page e[f]; a fragment of an invalid page is zero, whatever its entry holds
template <int D, class F, class E>
__device__ __forceinline__ void load_k_pages(F (&kf)[4][D / 32], const E* pool, long ld, long pageStride, const int (&e)[4],
                                             unsigned ok, int in_page, int li, int lg, int limit, HideWord hide) {
  const HideWord mine = hide >> li;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const E* src = pool + (long)e[f] * pageStride + (long)(((16 * f) & in_page) + li) * ld + 8 * lg;
    const bool take = ((ok >> f) & 1u) && 16 * f + li < limit && !hidden(mine, 16 * f);
#pragma unroll
    for (int s = 0; s < D / 32; ++s) {
      if (take)
        kf[f][s] = *reinterpret_cast<const F*>(src + 32 * s);
      else
        kf[f][s] = zero_frag<F>();
    }
  }
}

// load_v over pages of 16 or 32 keys: the lane's rows 4li … 4li + 3 lie in fragment li / 4, so in one page (4 divides 16)
template <int D, class F, class E>
__device__ __forceinline__ void load_v_pages(F (&vr)[D / 32][4], const E* pool, long ld, long pageStride, const int (&e)[4],
                                             unsigned ok, int in_page, int li, int lg, int limit, HideWord hide) {
  const HideWord own = hide >> (4 * li);
  const int f = li >> 2;
  const int mine = f == 0 ? e[0] : f == 1 ? e[1] : f == 2 ? e[2] : e[3];
  const E* src = pool + (long)mine * pageStride + (long)((4 * li) & in_page) * ld + 8 * lg;
  const bool valid = (ok >> f) & 1u;
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (valid && 4 * li + r < limit && !hidden(own, r))
        vr[i][r] = *reinterpret_cast<const F*>(src + (long)r * ld + 32 * i);
      else
        vr[i][r] = zero_frag<F>();
    }
}

// … into the wave's transposed image [D][64 + 8]
template <class T, int D>
__device__ __forceinline__ void store_transposed(unsigned short* Tt, const uint4 (&vr)[D / 32][4], int li, int lg) {
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // mfma_device.h's store_rc for unit li + 16(lg + 4i), written out: the call changed 48 kernels
      const uint2 w = {half_of(vr[i][0], e) | (half_of(vr[i][1], e) << 16), half_of(vr[i][2], e) | (half_of(vr[i][3], e) << 16)};
      *reinterpret_cast<uint2*>(Tt + (8 * (lg + 4 * i) + e) * kTStr + 4 * li) = w;
    }
}
// … of e4m3fn bytes: widened on the way, so the image holds T either way
template <class T, int D>
__device__ __forceinline__ void store_transposed(unsigned short* Tt, const uint2 (&vr)[D / 32][4], int li, int lg) {
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const uint4 x[4] = {widen<T>(vr[i][0]), widen<T>(vr[i][1]), widen<T>(vr[i][2]), widen<T>(vr[i][3])};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint2 w = {half_of(x[0], e) | (half_of(x[1], e) << 16), half_of(x[2], e) | (half_of(x[3], e) << 16)};
      *reinterpret_cast<uint2*>(Tt + (8 * (lg + 4 * i) + e) * kTStr + 4 * li) = w;
    }
  }
}

// acc[f][r] = ⟨key 16f + 4lg + r of the block, own row li⟩ over d
template <class T, int D, class F>
__device__ __forceinline__ void score(f32x4 (&acc)[4], const F (&kf)[4][D / 32], const uint4 (&own)[D / 32]) {
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < D / 32; ++s) acc[f] = mfma<T>(widen<T>(kf[f][s]), own[s], acc[f]);
  }
}

// the next entry of this wave at or after p (in steps of the workgroup's waves) that is computed: inside the grid and
// not wholly beyond pos — nor (WINDOW: the Tree<…> kernels) wholly behind the window: a block of keys
// [64j, 64j + 64) ⊂ [sink, edge), edge = pos − window + 1 the first key the window shows.  A skipped entry keeps its list position.
template <bool WINDOW>
__device__ __forceinline__ int next_entry(const int32_t* col, int p, int end, int pos, int blocks, int edge, int sink) {
  for (; p < end; p += kWaves) {
    const int j = col[p];
    if ((unsigned)j >= (unsigned)blocks || (long)j * kB > pos) continue;
    if constexpr (WINDOW)
      if ((long)j * kB >= sink && (long)j * kB + kB <= edge) continue;
    break;
  }
  return p;
}

// the weight of a partial with maximum m in a merge to the maximum M (an empty partial, m = −inf, weighs nothing)
__device__ __forceinline__ float merge_weight(float m, float M) { return m == -INFINITY ? 0.f : __expf(m - M); }

// element d of the row of query head g of (c, t): normalised, rounded once; the row's log-sum-exp with its element 0.
// SCALED: `vs`, the fp8 forms' v_scale of the item's head (value_scale: read once at the kernel's start, 1 for a null
// pointer — every 2-byte call), multiplies the normalised element; the 2-byte walk, which never has one, does not look.
// The last product is rounded to fp32 BEFORE it is narrowed, whatever T and SCALED: left alone, the compiler folds the
// product and the narrowing to float16 into one v_fma_mixlo_f16, which rounds the exact product once — O · inv in the
// 2-byte walk, x · vs in the other forms — and the fp8 call at scale 1 then differs from the 2-byte call on the widened
// cache in the last bit of about one float16 element in 10⁴ (found at 64-entry lists).  The empty asm keeps them apart.
template <class T, bool SCALED>
__device__ __forceinline__ void finish(const Args& a, int c, int t, int g, int d, float M, float L, float O, float vs) {
  const float inv = L == 0.f ? 0.f : 1.f / L;
  const long item = (long)c * a.group + g;
  float x = O * inv;
  if constexpr (SCALED) x *= vs;
  asm("" : "+v"(x));  // (no instruction: x is an fp32 value of its own before it is narrowed)
  a.out[item * a.strideO + (long)t * a.ldo + d] = T::down(x);
  if (d == 0) a.lse[item * a.T + t] = L == 0.f ? -INFINITY : M + __logf(L);
}

// The walk of one chunk and the merge of its four waves, in the three forms of tile addressing (FORM).  The paged forms
// differ from the contiguous one in where a tile's rows are loaded from and in the validity of a page, which joins the
// position mask — the summation, the chunking and the merge are the same statements, so a paged call has the bits of the
// contiguous call on the gathered cache.
// The cache element is part of the kernel's first parameter: T itself (k and v hold T), or Fp8<T> — the cache holds e4m3fn
// bytes: the loads, the widening and the two scales differ, nothing else.
// Where a token's list comes from is part of the kernel's first parameter too: row pos / 64 of the CSR layout of its k / v
// item, or — Listed<TC>, the *_lists and *_lists_decode entries, over either cache element — row (c, t)
// of the caller's block_ids, cut to block_counts.  A compile-time form of the walk: what follows the two bounds is the same
// statements, so a list has the bits of the layout row that lists the same blocks in the same order.
template <class TS, int D, int FORM>
__global__ __launch_bounds__(256) void block_attention_decode_kernel(Args a) {
  typedef typename Source<TS>::cache TC;
  constexpr bool LISTS = Source<TS>::lists;
  constexpr bool TREE = Source<TS>::tree;
  typedef typename Operand<TC>::type T;
  constexpr bool FP8 = Operand<TC>::fp8;
  typedef typename Cache<FP8>::elem E;
  typedef typename Cache<FP8>::frag F;
  constexpr int kPStr = D + 4;  // a wave's partial in its own image: [16][D + 4] floats — o[D], m, l
  __shared__ __attribute__((aligned(16))) unsigned short Vt[kWaves][D * kTStr];
  static_assert(kMaxGroup * kPStr * 4 <= D * kTStr * 2, "the partial fits the image");
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
  // the paged forms say that the wave's number is uniform: list positions, columns and table entries stay in scalar
  // registers, and the page bases cost the vector file nothing
  // (so does the tree form: the tile's column and with it the hide word stay scalar)
  const int w = FORM == kContiguous && !TREE ? tid >> 6 : __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ch = blockIdx.x, c = blockIdx.y, t = blockIdx.z;
  const int G = a.group;
  int klen = a.k_lens[c / a.lens_div];
  klen = klen < 0 ? 0 : klen > a.smax ? (int)a.smax : klen;
  const int pos = klen - a.T + t;  // the token's position: it sees keys j ≤ pos of the blocks its layout row lists
  int beg = 0, end = 0;            // this chunk's part of the list
  if (pos >= 0) {
    long lo, hi;
    if constexpr (LISTS) {
      const long row = (long)c * a.T + t;
      const int n = a.counts[row];
      lo = row * a.list_k;
      hi = lo + (n < 0 ? 0 : n > a.list_k ? a.list_k : n);
    } else {
      const int32_t* rp = a.rowptr + (long)(c % a.layouts) * (a.blocks + 1);
      lo = rp[pos / kB], hi = rp[pos / kB + 1];
      lo = lo < 0 ? 0 : lo;
      hi = hi > a.nnz ? a.nnz : hi;
    }
    lo += (long)ch * a.chunk;
    hi = hi < lo + a.chunk ? hi : lo + a.chunk;
    if (lo < hi) beg = (int)lo, end = (int)hi;
  }
  if (beg == end) {  // no token, or the chunk lies beyond the list's end: the empty partial (−inf, 0, 0), and leave
    for (int e = tid; e < G * D; e += 256) {
      const int g = e / D, d = e - g * D;
      if (a.chunks == 1) {
        finish<T, FP8>(a, c, t, g, d, -INFINITY, 0.f, 0.f, 1.f);
      } else {
        float* row = a.ws + ((((long)c * a.T + t) * a.chunks + ch) * G + g) * (D + 2);
        row[2 + d] = 0.f;
        if (d == 0) row[0] = -INFINITY, row[1] = 0.f;
      }
    }
    return;
  }
  // (a pool has no batch stride: the item's pages come from its table row)
  const E* K = static_cast<const E*>(a.k) + (FORM == kContiguous ? (long)(c / a.heads) * a.batchK : 0L) + (long)(c % a.heads) * a.headK;
  const E* V = static_cast<const E*>(a.v) + (FORM == kContiguous ? (long)(c / a.heads) * a.batchV : 0L) + (long)(c % a.heads) * a.headV;
  unsigned short* Vw = Vt[w];
  // The tree form: token t sees key j iff the plain rule holds and (j < base, or j == pos, or bit j − base of its word is set).
  // H: the hidden keys in window coordinates (bit i: key base + i), of the bits below t only — the token sees itself, and the
  // keys beyond pos are the plain rule's.  Read once per workgroup through a uniform address, shifted per tile in scalar
  // registers; a hidden key is treated like a key beyond pos: never loaded, staged as zeros, its score −inf.
  // The window is the word's second source: the keys [sink, edge), edge = pos − window + 1, are hidden — in
  // tile J the bits [max(sink − 64 J, 0), min(edge − 64 J, 64)), made in scalar registers.  edge and sink are clamped to
  // [0, pos + 1] and [0, Smax] once, so the differences below stay int32s; a null tree_mask is "no tree": H = 0, T unbound.
  [[maybe_unused]] HideWord H = 0;
  [[maybe_unused]] int base = 0, edge = 0, sink = 0;
  if constexpr (TREE) {
    base = klen - a.T;
    if (a.tree_mask) {
      const HideWord mask = (HideWord)a.tree_mask[(long)(a.mask_rows == 1 ? 0 : c / a.heads) * a.T + t];
      H = ~mask & ((1ull << t) - 1ull);  // (t < T ≤ 64)
    }
    edge = pos - a.window + 1 < 0 ? 0 : pos - a.window + 1;  // (pos ≥ 0 here, window ≥ 1: no overflow)
    sink = a.sink > a.smax ? (int)a.smax : a.sink;
  }
  auto hide_of = [&](int J) -> HideWord {  // the hide word of tile J: H moved by off = base − 64 J, 0 unless −64 < off < 64
    if constexpr (TREE) {
      const int off = base - J * kB;
      HideWord h = off <= -kB || off >= kB ? 0ull : off >= 0 ? H << off : H >> -off;
      const int lo = sink - J * kB < 0 ? 0 : sink - J * kB, hi = edge - J * kB > kB ? kB : edge - J * kB;
      if (lo < hi) h |= (hi == kB ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);  // (lo < hi ≤ 64: a shift by 64 is none)
      return h;
    } else {
      return 0ull;
    }
  };
  // what multiplies a score: scale, or in the fp8 forms scale · k_scale[h] — one fp32 product per workgroup
  const float sc = FP8 ? a.scale * head_scale(a.k_scale, a.k_scale_count, c % a.heads) : a.scale;
  // … and the stored element (only a one-chunk walk stores): read here, long before it is used
  const float vs = FP8 && a.chunks == 1 ? head_scale(a.v_scale, a.v_scale_count, c % a.heads) : 1.f;

  uint4 qf[D / 32];  // the own rows as B fragments: lane (li, lg) holds columns 32s + 8lg … + 7 of query head li
#pragma unroll
  for (int s = 0; s < D / 32; ++s) qf[s] = uint4{0u, 0u, 0u, 0u};
  int p = next_entry<TREE>(a.col, beg + w, end, pos, a.blocks, edge, sink);
  if (li < G && p < end) {
    const uint16_t* row = a.q + ((long)c * G + li) * a.strideQ + (long)t * a.ldq;
#pragma unroll
    for (int s = 0; s < D / 32; ++s) qf[s] = *reinterpret_cast<const uint4*>(row + 32 * s + 8 * lg);
  }
  f32x4 o[D / 16];
#pragma unroll
  for (int fd = 0; fd < D / 16; ++fd) o[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  F kf[4][D / 32], vr[D / 32][4];
  // Paged forms: the tile whose loads are in flight (J, its table entries e, their validity ok) and the entry after it
  // (pn, Jn, en).  The chain col[p] → table → tile is cut in two: the column and the table entries of an entry are read
  // ONE ITERATION EARLY, right after the loads of the entry before it were issued, and have that entry's softmax and P·V
  // to arrive — so the tile loads are issued right after the score MFMAs from values that are already there.
  int J = 0, Jn = 0, pn = end, e[4] = {0, 0, 0, 0}, en[4] = {0, 0, 0, 0};
  unsigned ok = 0;
  const int32_t* trow = nullptr;
  const int in_page = FORM == kContiguous ? 0 : (1 << a.page_shift) - 1;
  auto issue = [&]() {  // the loads of tile J of the pool; an invalid page loads nothing and stages zeros
    const int limit = pos + 1 - J * kB;
    const HideWord hide = hide_of(J);
    if constexpr (FORM == kPaged) {
      const long row = (J * kB) & in_page;
      load_k<D>(kf, K + (long)e[0] * a.pageK + row * a.ldk, a.ldk, li, lg, ok ? limit : 0, hide);
      load_v<D>(vr, V + (long)e[0] * a.pageV + row * a.ldv, a.ldv, li, lg, ok ? limit : 0, hide);
    } else {
      load_k_pages<D>(kf, K, a.ldk, a.pageK, e, ok, in_page, li, lg, limit, hide);
      load_v_pages<D>(vr, V, a.ldv, a.pageV, e, ok, in_page, li, lg, limit, hide);
    }
  };
  auto look_ahead = [&](int from) {  // the next computed entry at or after `from`, its column and its table entries
    pn = next_entry<TREE>(a.col, from, end, pos, a.blocks, edge, sink);
    if (pn < end) {
      Jn = a.col[pn];
      read_pages<FORM>(en, trow, Jn, a.page_shift);
    }
  };
  if constexpr (FORM == kContiguous) {
    if (p < end) {
      const int J = a.col[p];
      load_k<D>(kf, K + (long)J * kB * a.ldk, a.ldk, li, lg, pos + 1 - J * kB, hide_of(J));
      load_v<D>(vr, V + (long)J * kB * a.ldv, a.ldv, li, lg, pos + 1 - J * kB, hide_of(J));
    }
  } else {
    trow = a.table + (long)(c / a.heads) * a.table_ld;
    if (p < end) {
      J = a.col[p];
      read_pages<FORM>(e, trow, J, a.page_shift);
      ok = valid_pages(e, a.pages);
      issue();
      look_ahead(p + kWaves);
    }
  }
  while (p < end) {
    // keys of this block the token sees (≥ 1; 64 or more: all)
    const int visible = pos + 1 - (FORM == kContiguous ? a.col[p] : J) * kB;
    // … and the draft keys among them that it does not (tree form): element 16f + 4lg + r at bit 16f + r
    [[maybe_unused]] const HideWord unseen = hide_of(FORM == kContiguous ? a.col[p] : J) >> (4 * lg);
    const unsigned seen = ok;  // … and the fragments of it that lie in a page (paged forms)
    fence_wave();  // the previous entry's reads of the image are done
    store_transposed<T, D>(Vw, vr, li, lg);
    fence_wave();
    f32x4 s[4];
    score<T, D>(s, kf, qf);
    if constexpr (FORM == kContiguous) {
      p = next_entry<TREE>(a.col, p + kWaves, end, pos, a.blocks, edge, sink);
      if (p < end) {  // the next entry's loads are in flight while this one is computed
        const int J = a.col[p];
        load_k<D>(kf, K + (long)J * kB * a.ldk, a.ldk, li, lg, pos + 1 - J * kB, hide_of(J));
        load_v<D>(vr, V + (long)J * kB * a.ldv, a.ldv, li, lg, pos + 1 - J * kB, hide_of(J));
      }
    } else {
      p = pn;
      if (p < end) {  // … from the column and the table entries read an iteration ago; then the look-ahead moves on
        J = Jn;
#pragma unroll
        for (int f = 0; f < 4; ++f) e[f] = en[f];
        ok = valid_pages(e, a.pages);
        issue();
        look_ahead(p + kWaves);
      }
    }
    float mt = -INFINITY;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = s[f][r] * sc;
        if (16 * f + 4 * lg + r >= visible) x = -INFINITY;
        if (TREE && hidden(unseen, 16 * f + r)) x = -INFINITY;  // a hidden draft key
        if (FORM != kContiguous && !((seen >> f) & 1u)) x = -INFINITY;  // a key of an invalid page
        s[f][r] = x;
        mt = fmaxf(mt, x);
      }
    const float mn = fmaxf(m, group_max(mt));
    const float alpha = m == mn ? 1.f : __expf(m - mn);  // (−inf stays: nothing seen yet)
    float sum = 0.f;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = s[f][r] == -INFINITY ? 0.f : __expf(s[f][r] - mn);
        s[f][r] = e;
        sum += e;
      }
    l = l * alpha + sum;  // this lane's share of the row sum; the four shares meet after the walk
    m = mn;
#pragma unroll
    for (int fd = 0; fd < D / 16; ++fd)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[fd][r] *= alpha;
    uint4 pb[2];
    pack_tile<T>(pb, s);
    accumulate<T, D>(o, Vw, pb, li, lg);
  }
  l = group_sum(l);

  // the four waves' partials meet through LDS, each in its own image, and are merged in wave order
  fence_wave();
  float* P = reinterpret_cast<float*>(Vw);
  if (li < G) {
#pragma unroll
    for (int fd = 0; fd < D / 16; ++fd) *reinterpret_cast<f32x4*>(P + li * kPStr + 16 * fd + 4 * lg) = o[fd];
    if (lg == 0) P[li * kPStr + D] = m, P[li * kPStr + D + 1] = l;
  }
  __syncthreads();
  for (int e = tid; e < G * D; e += 256) {
    const int g = e / D, d = e - g * D;
    float M = -INFINITY;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) M = fmaxf(M, reinterpret_cast<const float*>(Vt[i])[g * kPStr + D]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
      const float* Pi = reinterpret_cast<const float*>(Vt[i]) + g * kPStr;
      const float wt = merge_weight(Pi[D], M);
      L += Pi[D + 1] * wt;
      O += Pi[d] * wt;
    }
    if (a.chunks == 1) {
      finish<T, FP8>(a, c, t, g, d, M, L, O, vs);
    } else {
      float* row = a.ws + ((((long)c * a.T + t) * a.chunks + ch) * G + g) * (D + 2);
      row[2 + d] = O;
      if (d == 0) row[0] = M, row[1] = L;
    }
  }
}

// merges the chunks' partials of the rows of (c, t) in ascending chunk order, normalises, stores out and lse
template <class T>
__global__ __launch_bounds__(128) void block_attention_decode_combine_kernel(Args a, int D) {
  const int c = blockIdx.x, t = blockIdx.y, G = a.group;
  const float vs = head_scale(a.v_scale, a.v_scale_count, c % a.heads);  // (null in every 2-byte call: 1)
  const float* base = a.ws + (((long)c * a.T + t) * a.chunks) * G * (D + 2);
  for (int e = threadIdx.x; e < G * D; e += 128) {
    const int g = e / D, d = e - g * D;
    float M = -INFINITY;
    for (int i = 0; i < a.chunks; ++i) M = fmaxf(M, base[((long)i * G + g) * (D + 2)]);
    float L = 0.f, O = 0.f;
    for (int i = 0; i < a.chunks; ++i) {
      const float* row = base + ((long)i * G + g) * (D + 2);
      const float wt = merge_weight(row[0], M);
      L += row[1] * wt;
      O += row[2 + d] * wt;
    }
    finish<T, true>(a, c, t, g, d, M, L, O, vs);
  }
}

// the caller's lists of the *_lists entries: block_counts [items][T] and K, the entries of a row of block_ids
struct Lists {
  const int32_t* counts = nullptr;
  int32_t K = 0;
};

int chunks_of(int32_t Smax, int32_t chunk) {  // from the shape alone; a list has at most Smax / 64 entries
  const long blocks = Smax / kB;
  const long n = (blocks + chunk - 1) / chunk;
  return (int)(n < 1 ? 1 : n);
}

// the walk's launch checked, then — with more than one chunk — the combine kernel
template <class T>
int finish_launch(const Args& a, int items, int D, hipStream_t s) {
  const int st = mi::check_launch();
  if (st != MI_OK || a.chunks == 1) return st;
  hipLaunchKernelGGL((block_attention_decode_combine_kernel<T>), dim3((unsigned)items, (unsigned)a.T), dim3(128), 0, s, a, D);
  return mi::check_launch();
}

template <class T, int D, bool FP8, bool TREE>
int launch(const Args& a, int items, hipStream_t s) {
  const dim3 grid((unsigned)a.chunks, (unsigned)items, (unsigned)a.T);
  typedef std::conditional_t<FP8, Fp8<T>, T> TC;  // the cache element type is part of the kernel's first parameter
  typedef std::conditional_t<TREE, Tree<TC>, TC> OfLayout;  // … and so is the tree form, around either list source
  typedef std::conditional_t<TREE, Tree<Listed<TC>>, Listed<TC>> OfLists;
  with_form(a, [&](auto form) {
    constexpr int FORM = decltype(form)::value;
    if (a.counts) {  // the list source
      hipLaunchKernelGGL((block_attention_decode_kernel<OfLists, D, FORM>), grid, dim3(256), 0, s, a);
      return 0;
    }
    hipLaunchKernelGGL((block_attention_decode_kernel<OfLayout, D, FORM>), grid, dim3(256), 0, s, a);
    return 0;
  });
  return finish_launch<T>(a, items, D, s);
}

// the tree mask of the tree_decode entries: [rows][T] words, rows 1 (one row for the batch) or the batch size
struct TreeMask {
  const int64_t* mask = nullptr;
  int32_t rows = 0;
};
constexpr int kMaxTree = 64;  // the T of a tree call: a token's word names the window's keys

// the window of the window_decode entries; what the other entries pass hides nothing
struct Window {
  int32_t window = 0x7fffffff, sink = 0;
};

// Every check comes before the first HIP call.  `r`: what every reading entry takes (block_attention_cache_device.h), FP8 its
// cache type, TREE that it is a tree_decode entry (`tree` is looked at), WINDOW that it is a window_decode entry (`win` is; it
// runs on the Tree<…> kernels with no mask); q, chunk and the workspace are this entry's own.
template <class T, bool FP8 = false, bool TREE = false, bool WINDOW = false>
int decode_entry(const ReadCall& r, const uint16_t* q, int64_t ldq, int64_t strideQ, int32_t chunk, void* workspace,
                 size_t workspace_bytes, hipStream_t s, const Lists& lists = Lists(), const TreeMask& tree = TreeMask(),
                 const Window& win = Window()) {
  static_assert(!(TREE && WINDOW), "a window's lower edge is the slot's: no windows over tree masks");
  if (WINDOW && (win.window < 1 || win.sink < 0)) return MI_EINVAL;
  // the list source: `col` is block_ids, nnz its items · T · K entries; a list has at most K entries, so the chunks — and
  // the workspace — are those of a cache of K blocks
  const bool listed = lists.K != 0 || lists.counts;
  if (listed && (lists.K < 1 || lists.K > 0x7fffffff / kB || !lists.counts || !aligned4(lists.counts) || !aligned4(r.col))) return MI_EINVAL;
  const int32_t span = listed ? lists.K * kB : r.Smax;  // what the chunks are counted over
  if (r.group > kMaxGroup || chunk < 1) return MI_EINVAL;
  if (const int st = read_sizes_status(FP8, r)) return st;
  if (r.items > 65535 || r.T > 65535) return MI_EINVAL;  // the grid's y and z: no item loop
  if (TREE && r.T > kMaxTree) return MI_EINVAL;
  if (read_is_empty(r)) return MI_OK;
  if (!q || !mi::aligned16(q) || ldq < r.D || !stride_ok(ldq) || !stride_ok(strideQ)) return MI_EINVAL;
  if (!read_operands_ok(FP8, r, listed)) return MI_EINVAL;
  if (TREE && (!tree.mask || reinterpret_cast<uintptr_t>(tree.mask) % 8 != 0 || (tree.rows != 1 && tree.rows != r.items / r.heads)))
    return MI_EINVAL;
  const int chunks = chunks_of(span, chunk);
  if (chunks > 1) {
    if (!workspace || !mi::aligned16(workspace)) return MI_EINVAL;
    if (workspace_bytes < mi_block_attention_decode_workspace_bytes(r.items, r.T, r.group, r.D, span, chunk)) return MI_ENOMEM;
  }
  Args a = {};
  fill_read_args(a, FP8, r);
  a.chunk = chunk, a.chunks = chunks;
  a.q = q, a.ldq = ldq, a.strideQ = strideQ;
  a.ws = static_cast<float*>(workspace);
  if (listed) a.counts = lists.counts, a.list_k = lists.K;
  if (TREE) a.tree_mask = tree.mask, a.mask_rows = tree.rows;
  a.window = win.window, a.sink = win.sink;
  return with_width(r.D, [&](auto d) { return launch<T, decltype(d)::value, FP8, TREE || WINDOW>(a, r.items, s); });
}

}  // namespace

extern "C" {

size_t mi_block_attention_decode_workspace_bytes(int32_t items, int32_t T, int32_t group, int32_t D, int32_t Smax, int32_t chunk) {
  if (items <= 0 || T <= 0 || group <= 0 || D <= 0 || Smax < 0 || chunk < 1) return 0;
  const int chunks = chunks_of(Smax, chunk);
  if (chunks == 1) return 0;  // the walk stores out itself
  return (size_t)items * (size_t)T * (size_t)chunks * (size_t)group * (size_t)(D + 2) * sizeof(float);
}

// The 48 entries of the header, two per line of the table below (bf16, f16).  The header's parameter lists in pieces: the
// list — a LAYOUT's, or the caller's LISTS —, the sizes, [the table] of a PAGED entry, the operands, [the
// scales] of an fp8 entry (§3.20, §3.32), [what the entry's form adds], the outputs …
#define MI_DECODE_HEAD_LAYOUT const int32_t *rowptr, const int32_t *col, int64_t nnz, int32_t layouts
#define MI_DECODE_HEAD_LISTS const int32_t *block_ids, const int32_t *block_counts, int32_t K
#define MI_DECODE_SIZES int32_t items, int32_t heads, int32_t T, int32_t Smax
#define MI_DECODE_TABLE_FLAT
#define MI_DECODE_TABLE_PAGED const int32_t *block_table, int64_t table_ld, int32_t pages, int32_t page,
#define MI_DECODE_OPERANDS(CT)                                                                                                  \
  int32_t D, const uint16_t *q, int64_t ldq, int64_t strideQ, const CT *k, int64_t ldk, int64_t headK, int64_t batchK,          \
      const CT *v, int64_t ldv, int64_t headV, int64_t batchV, const int32_t *k_lens, int32_t lens_count, int32_t group,        \
      int32_t chunk, float scale
#define MI_DECODE_SCALES_false
#define MI_DECODE_SCALES_true const float *k_scale, int32_t k_scale_count, const float *v_scale, int32_t v_scale_count,
#define MI_DECODE_OUT \
  uint16_t *out, int64_t ldo, int64_t strideO, float *lse, void *workspace, size_t workspace_bytes, mi_stream_t stream
// … and what an entry passes on: the reading call, then its own.  The list source hands block_ids over as col, its
// items · T · K entries as nnz, no rowptr and one layout.  (A K that is no positive int32 is refused inside, before the
// product is looked at.)
#define MI_DECODE_CALL_LAYOUT(...) MI_READ_CALL(rowptr, col, nnz, layouts, __VA_ARGS__)
#define MI_DECODE_CALL_LISTS(...) MI_READ_CALL(nullptr, block_ids, K < 1 ? 0 : (int64_t)items * T * K, 1, __VA_ARGS__)
#define MI_DECODE_LISTS_LAYOUT Lists()
#define MI_DECODE_LISTS_LISTS Lists{block_counts, K < 1 ? -1 : K}
#define MI_DECODE_OWN q, ldq, strideQ, chunk, workspace, workspace_bytes, static_cast<hipStream_t>(stream)
// The forms, by the token a line ends in — its parameters between the operands and the outputs, and what is passed for them:
// PLAIN; TREE (§3.34): int64 words [mask_rows][T], mask_rows 1 (one row for the batch) or the batch size items / heads, T ≤ 64;
// WINDOW (§3.35): window ≥ 1, sink ≥ 0 — these entries run on the Tree<…> kernels with no mask.
#define MI_DECODE_ADDS_PLAIN
#define MI_DECODE_ADDS_TREE const int64_t *tree_mask, int32_t mask_rows,
#define MI_DECODE_ADDS_WINDOW int32_t window, int32_t sink,
#define MI_DECODE_PASS_PLAIN TreeMask()
#define MI_DECODE_PASS_TREE TreeMask{tree_mask, mask_rows}
#define MI_DECODE_PASS_WINDOW TreeMask(), Window{window, sink}

#define MI_DECODE_ENTRY(STEM, TYPE, SUFFIX, HEAD, PAGED, FP8, TREE, WINDOW, FORM)                                               \
  int mi_block_attention_##STEM##SUFFIX(MI_DECODE_HEAD_##HEAD, MI_DECODE_SIZES, MI_DECODE_TABLE_##PAGED                         \
                                        MI_DECODE_OPERANDS(MI_READ_CACHE_##FP8), MI_DECODE_SCALES_##FP8 MI_DECODE_ADDS_##FORM   \
                                        MI_DECODE_OUT) {                                                                        \
    return MI_READ_GUARD_##PAGED decode_entry<TYPE, FP8, TREE, WINDOW>(                                                         \
        MI_DECODE_CALL_##HEAD(MI_READ_TABLE_##PAGED, MI_READ_SCALES_##FP8), MI_DECODE_OWN, MI_DECODE_LISTS_##HEAD,              \
        MI_DECODE_PASS_##FORM);                                                                                                 \
  }
// one line of the table: the entry's name stem as the header spells it, the list, the cache's storage, FP8, the TREE and WINDOW
// of decode_entry, the form
#define MI_DECODE_ENTRIES(STEM, HEAD, PAGED, FP8, TREE, WINDOW, FORM)          \
  MI_DECODE_ENTRY(STEM, Bf16, _bf16, HEAD, PAGED, FP8, TREE, WINDOW, FORM)     \
  MI_DECODE_ENTRY(STEM, F16, _f16, HEAD, PAGED, FP8, TREE, WINDOW, FORM)

// clang-format off
MI_DECODE_ENTRIES(decode,                            LAYOUT, FLAT,  false, false, false, PLAIN)
MI_DECODE_ENTRIES(decode_paged,                      LAYOUT, PAGED, false, false, false, PLAIN)
MI_DECODE_ENTRIES(decode_fp8,                        LAYOUT, FLAT,  true,  false, false, PLAIN)
MI_DECODE_ENTRIES(decode_paged_fp8,                  LAYOUT, PAGED, true,  false, false, PLAIN)
MI_DECODE_ENTRIES(decode_lists,                      LISTS,  FLAT,  false, false, false, PLAIN)
MI_DECODE_ENTRIES(decode_lists_paged,                LISTS,  PAGED, false, false, false, PLAIN)
// (over an fp8 cache the names put `lists` first: `mi_block_attention_decode…` was a closed family when these came)
MI_DECODE_ENTRIES(lists_decode_fp8,                  LISTS,  FLAT,  true,  false, false, PLAIN)
MI_DECODE_ENTRIES(lists_decode_paged_fp8,            LISTS,  PAGED, true,  false, false, PLAIN)
MI_DECODE_ENTRIES(tree_decode,                       LAYOUT, FLAT,  false, true,  false, TREE)
MI_DECODE_ENTRIES(tree_decode_paged,                 LAYOUT, PAGED, false, true,  false, TREE)
MI_DECODE_ENTRIES(tree_decode_fp8,                   LAYOUT, FLAT,  true,  true,  false, TREE)
MI_DECODE_ENTRIES(tree_decode_paged_fp8,             LAYOUT, PAGED, true,  true,  false, TREE)
MI_DECODE_ENTRIES(tree_decode_lists,                 LISTS,  FLAT,  false, true,  false, TREE)
MI_DECODE_ENTRIES(tree_decode_lists_paged,           LISTS,  PAGED, false, true,  false, TREE)
MI_DECODE_ENTRIES(tree_decode_lists_fp8,             LISTS,  FLAT,  true,  true,  false, TREE)
MI_DECODE_ENTRIES(tree_decode_lists_paged_fp8,       LISTS,  PAGED, true,  true,  false, TREE)
MI_DECODE_ENTRIES(window_decode,                     LAYOUT, FLAT,  false, false, true,  WINDOW)
MI_DECODE_ENTRIES(window_decode_paged,               LAYOUT, PAGED, false, false, true,  WINDOW)
MI_DECODE_ENTRIES(window_decode_fp8,                 LAYOUT, FLAT,  true,  false, true,  WINDOW)
MI_DECODE_ENTRIES(window_decode_paged_fp8,           LAYOUT, PAGED, true,  false, true,  WINDOW)
MI_DECODE_ENTRIES(window_decode_lists,               LISTS,  FLAT,  false, false, true,  WINDOW)
MI_DECODE_ENTRIES(window_decode_lists_paged,         LISTS,  PAGED, false, false, true,  WINDOW)
MI_DECODE_ENTRIES(window_decode_lists_fp8,           LISTS,  FLAT,  true,  false, true,  WINDOW)
MI_DECODE_ENTRIES(window_decode_lists_paged_fp8,     LISTS,  PAGED, true,  false, true,  WINDOW)
// clang-format on

}  // extern "C"
