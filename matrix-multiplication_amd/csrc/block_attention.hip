// Block-sparse attention in bfloat16 and float16 on the matrix cores: out = softmax(scale · q·kᵀ + mask) · v, where the mask
// keeps the 64 × 64 blocks a CSR block layout lists (and, causal, the positions j ≤ i), with its backward.  q, k, v, out
// and the gradients are all of one type T ∈ {bf16, fp16} (2-byte bit patterns at the C-ABI).
//
// What it computes (contract of include/mi_spmm.h, mi_block_attention_{fwd,bwd}_{bf16,f16} — DESIGN.md §3.14):
//  * ONE instruction for every product: v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulators.  Scores, row maxima, row sums,
//    the log-sum-exp and δ = rowsum(dO ∘ O) stay in fp32; P is narrowed to T only as the operand of P·V (and of dOᵀ·P),
//    dS only as the operand of dS·K and dSᵀ·Q; out, dq, dk and dv are rounded once, at the store.
//  * Order: a query block walks its kept key blocks in the order of the CSR list, a key block (backward) the query blocks
//    of the TRANSPOSED list in its order; every output element is one accumulator of one wave.  The bits of an output
//    depend on its own item and its layout only — never on the batch, the neighbours or the launch.  No atomics, no host
//    read-back: graph-capturable.
//  * A block outside the list is never loaded.  causal: a listed block strictly above the diagonal is skipped, the
//    diagonal block masked by position.  A query row that sees nothing gives a zero row of out and dq and −inf as its
//    log-sum-exp; a key nobody sees zero rows of dk and dv.  A listed column outside [0, blocks) is skipped, offsets are
//    clamped to the list: a malformed layout cannot make a kernel read outside the operands.
//
//  * Grouped-query heads and per-item lengths (the _ex entries — DESIGN.md §3.17): query item b reads k / v item b / group,
//    and a key block sums dk, dv over its group's query items (g ascending, each over its own transposed list) in the same
//    accumulators.  With lengths (LENS, a compile-time form: a call without them runs kernels without any of it) a
//    position at or beyond its item's length does not exist: blocks wholly beyond are skipped, rows beyond are staged as
//    zeros and never enter an MFMA, scores / probabilities are masked by position, their outputs are zero rows.
//
// Kernels: a 256-thread workgroup owns one 64-row block of one item; wave w its rows 16w … 16w + 15 ("own" rows), held
// as MFMA B fragments in registers for the whole walk.  Each listed block of the other side ("walk" rows, 64 of them)
// is staged through registers into LDS (the global loads of the next block are in flight while this one is computed):
// a row image [64][D + 8] for the products that sum over d, and a transposed image [D][64 + 8] for those that sum over
// the walk rows.  With the walk rows as the MFMA A operand a score tile arrives with the OWN row on the lane (lane & 15)
// and 16 walk rows in its registers (16f + 4(lane >> 4) + r): the softmax constants of an own row are lane scalars, a row
// reduction is 15 in-register steps and two cross-lane ones, and the tile, packed, is already the B operand of the
// product that sums over the walk rows (k-slot (lane >> 4, j) of step s ↦ walk row 32s + 16(j >> 2) + 4(lane >> 4) + (j & 3);
// the transposed image is read in the same permuted order).  Results arrive as [d][own row]: four adjacent d per lane.
//  * forward: own = q; walk = k (scores), vᵀ (P·V); online softmax (running maximum and sum, rescale).
//  * backward, query blocks: own = q, dO; walk = k (S), v (dP), kᵀ (dQ += dS·K); δ computed in the prologue and written
//    for the key-block kernel; P = exp(scale·S − lse).
//  * backward, key blocks over the transposed layout: own = k, v; walk = q (Sᵀ), dO (dPᵀ), dOᵀ (dV += Pᵀ·dO),
//    qᵀ (dK += dSᵀ·Q); lse and δ of the walk rows are read per tile.
//
// kB, the transposed image's stride, pack_tile, accumulate and group_max / group_sum are block_attention_device.h's, which
// block_attention_decode.hip shares, as is `score` from a row image, which block_attention_prefill.hip shares; mfma<T> and
// half_of are mfma_device.h's.
#include "block_attention_device.h"

namespace {

struct Dense {  // a [batch][rows][D] operand: leading dimension and item stride in elements
  uint16_t* p;
  long ld, stride;
};

struct Args {
  const int32_t* rowptr;  // [layouts][own blocks + 1], with the layouts' bases
  const int32_t* col;     // [nnz], layout-local block columns
  long nnz;
  int layouts, batch, own_blocks, walk_blocks;
  long own_rows;  // rows of an item on the own side (lse, δ: [batch][own_rows]; walk side: walk_rows)
  long walk_rows;
  float scale;
  Dense q, k, v, o, dout, dq, dk, dv;
  float* lse;    // [batch][Sq]
  float* delta;  // [batch][Sq]
  int group;     // query items per k / v item: query item b reads (and dk, dv sum into) k / v item b / group
  int lens_div;  // query items per length entry: query item b has lengths q_lens[b / lens_div], k_lens[b / lens_div]
  const int32_t* q_lens;  // [batch / lens_div] or null (every query position exists); clamped to [0, Sq] where read
  const int32_t* k_lens;  // [batch / lens_div] or null; clamped to [0, Sk]
};

// the length of an item on a side of `rows` positions, clamped to [0, rows]; without LENS (or without the array) `rows`
template <bool LENS>
__device__ __forceinline__ int length_of(const int32_t* lens, int entry, long rows) {
  if (!LENS || lens == nullptr) return (int)rows;
  const int n = lens[entry];
  return n < 0 ? 0 : n > rows ? (int)rows : n;
}

// One 64 × D block in registers: unit u = tid < 2D holds rows 4(u & 15) … + 3, columns 8(u >> 4) … + 7.
template <int D>
struct Tile {
  uint4 v[4];
  // LIMIT: rows at or beyond `limit` (the part of the block beyond an item's length) are zero rows, whatever memory holds
  template <bool LIMIT>
  __device__ __forceinline__ void load(const uint16_t* src, long ld, int tid, int limit) {
    if (tid < 2 * D) {
      const uint16_t* p = src + (long)(4 * (tid & 15)) * ld + 8 * (tid >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!LIMIT || 4 * (tid & 15) + i < limit)
          v[i] = *reinterpret_cast<const uint4*>(p + i * ld);
        else
          v[i] = uint4{0u, 0u, 0u, 0u};
      }
    }
  }
  // the row image [64][D + 8]
  __device__ __forceinline__ void store_rows(unsigned short* R, int tid) const {
    if (tid < 2 * D) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(R + (4 * (tid & 15) + i) * (D + 8) + 8 * (tid >> 4)) = v[i];
    }
  }
  // the transposed image [D][64 + 8]: the unit is store_rc's, the walk rows its k
  __device__ __forceinline__ void store_transposed(unsigned short* Tt, int tid) const {
    if (tid < 2 * D) store_rc(Tt, v, tid);
  }
};

// The wave's 16 own rows as B fragments: lane (li, lg) holds columns 32s + 8lg … + 7 of row li.
template <int D>
__device__ __forceinline__ void load_own(uint4 (&f)[D / 32], const uint16_t* rows, long ld, int li, int lg) {
#pragma unroll
  for (int s = 0; s < D / 32; ++s) f[s] = *reinterpret_cast<const uint4*>(rows + (long)li * ld + 32 * s + 8 * lg);
}
template <int D>
__device__ __forceinline__ void zero_own(uint4 (&f)[D / 32]) {
#pragma unroll
  for (int s = 0; s < D / 32; ++s) f[s] = uint4{0u, 0u, 0u, 0u};
}

// rows [d][own row li] → own row li, columns 16fd + 4lg … + 3, each value times `mul`, rounded once
template <class T, int D>
__device__ __forceinline__ void store_own(const f32x4 (&acc)[D / 16], float mul, uint16_t* rows, long ld, int li, int lg) {
#pragma unroll
  for (int fd = 0; fd < D / 16; ++fd) {
    const f32x4 x = acc[fd];
    *reinterpret_cast<uint2*>(rows + (long)li * ld + 16 * fd + 4 * lg) =
        uint2{pack2<T>(x[0] * mul, x[1] * mul), pack2<T>(x[2] * mul, x[3] * mul)};
  }
}

// own row li, columns 16fd + 4lg … + 3: zeros
template <int D>
__device__ __forceinline__ void store_zero(uint16_t* rows, long ld, int li, int lg) {
#pragma unroll
  for (int fd = 0; fd < D / 16; ++fd) *reinterpret_cast<uint2*>(rows + (long)li * ld + 16 * fd + 4 * lg) = uint2{0u, 0u};
}
template <int D>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[D / 16]) {
#pragma unroll
  for (int fd = 0; fd < D / 16; ++fd) acc[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// the next listed block at or after p that is computed: inside the grid and, causal, not beyond the own block's diagonal.
// own_first: the own side is the query side (skip walk blocks J > I); else the key side (skip walk blocks I < J).
// walk_blocks is the grid cut to the walk side's length: a block wholly beyond it is skipped like one outside the list.
template <bool CAUSAL, bool OWN_IS_QUERY>
__device__ __forceinline__ int next_block(const int32_t* col, int p, int end, int own_block, int walk_blocks) {
  for (; p < end; ++p) {
    const int j = col[p];
    if ((unsigned)j >= (unsigned)walk_blocks) continue;
    if (CAUSAL && (OWN_IS_QUERY ? j > own_block : j < own_block)) continue;
    break;
  }
  return p;
}

struct Walk {  // the part of a layout's list one workgroup walks
  const int32_t* col;
  int beg, end;
};
__device__ __forceinline__ Walk walk_of(const Args& a, int item, int own_block) {
  const int lay = item % a.layouts;
  const int32_t* rp = a.rowptr + (long)lay * (a.own_blocks + 1);
  long beg = rp[own_block], end = rp[own_block + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > a.nnz ? a.nnz : end;
  return Walk{a.col, (int)beg, (int)end};
}

template <class T, int D, bool CAUSAL, bool LENS>
__global__ __launch_bounds__(256) void block_attention_fwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) unsigned short Ks[kB * (D + 8)];
  __shared__ __attribute__((aligned(16))) unsigned short Vt[D * kTStr];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int I = blockIdx.x;
  for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
    const Walk wk = walk_of(a, b, I);
    const int c = b / a.group;
    const uint16_t* K = a.k.p + (long)c * a.k.stride;
    const uint16_t* V = a.v.p + (long)c * a.v.stride;
    const long row0 = (long)I * kB + 16 * w;
    uint16_t* orows = a.o.p + (long)b * a.o.stride + row0 * a.o.ld;
    const int qlen = length_of<LENS>(a.q_lens, b / a.lens_div, a.own_rows);
    const int klen = length_of<LENS>(a.k_lens, b / a.lens_div, a.walk_rows);
    const int kblocks = LENS ? (klen + kB - 1) / kB : a.walk_blocks;
    if (LENS && (long)I * kB >= qlen) {  // the whole block is beyond the item's length
      store_zero<D>(orows, a.o.ld, li, lg);
      if (lg == 0) a.lse[(long)b * a.own_rows + row0 + li] = -INFINITY;
      continue;
    }
    const bool dead = LENS && row0 + li >= qlen;  // an own row beyond the length: never an MFMA operand
    uint4 qf[D / 32];
    load_own<D>(qf, a.q.p + (long)b * a.q.stride + row0 * a.q.ld, a.q.ld, li, lg);
    if (dead) zero_own<D>(qf);
    f32x4 o[D / 16];
    zero_acc<D>(o);
    float m = -INFINITY, l = 0.f;

    Tile<D> tk, tv;
    int p = next_block<CAUSAL, true>(wk.col, wk.beg, wk.end, I, kblocks);
    if (p < wk.end) {
      tk.template load<LENS>(K + (long)wk.col[p] * kB * a.k.ld, a.k.ld, tid, klen - wk.col[p] * kB);
      tv.template load<LENS>(V + (long)wk.col[p] * kB * a.v.ld, a.v.ld, tid, klen - wk.col[p] * kB);
    }
    while (p < wk.end) {
      const int J = wk.col[p];
      __syncthreads();  // the previous block's reads are done
      tk.store_rows(Ks, tid);
      tv.store_transposed(Vt, tid);
      __syncthreads();
      p = next_block<CAUSAL, true>(wk.col, p + 1, wk.end, I, kblocks);
      if (p < wk.end) {
        tk.template load<LENS>(K + (long)wk.col[p] * kB * a.k.ld, a.k.ld, tid, klen - wk.col[p] * kB);
        tv.template load<LENS>(V + (long)wk.col[p] * kB * a.v.ld, a.v.ld, tid, klen - wk.col[p] * kB);
      }
      const int kleft = klen - J * kB;  // keys of this block that exist
      f32x4 s[4];
      score<T, D>(s, Ks, qf, li, lg);
      float mt = -INFINITY;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = s[f][r] * a.scale;
          if (CAUSAL && J == I && 16 * f + 4 * lg + r > 16 * w + li) t = -INFINITY;
          if (LENS && 16 * f + 4 * lg + r >= kleft) t = -INFINITY;
          s[f][r] = t;
          mt = fmaxf(mt, t);
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
      accumulate<T, D>(o, Vt, pb, li, lg);
    }
    l = group_sum(l);
    if (dead) {
      l = 0.f;
      zero_acc<D>(o);
    }
    const float inv = l == 0.f ? 0.f : 1.f / l;
    store_own<T, D>(o, inv, orows, a.o.ld, li, lg);
    if (lg == 0) a.lse[(long)b * a.own_rows + row0 + li] = l == 0.f ? -INFINITY : m + __logf(l);
    __syncthreads();  // the next item restages
  }
}

// P of a score tile from the rows' log-sum-exp: own row on the lane (lse a lane scalar)
__device__ __forceinline__ float prob(float t, float lse) {
  return (lse == -INFINITY || t == -INFINITY) ? 0.f : __expf(t - lse);
}

// dQ over the layout; own = q and dO.  Also writes δ = rowsum(dO ∘ O) of its rows (0 for a row beyond the length).
template <class T, int D, bool CAUSAL, bool LENS>
__global__ __launch_bounds__(256) void block_attention_dq_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) unsigned short Ks[kB * (D + 8)];
  __shared__ __attribute__((aligned(16))) unsigned short Vs[kB * (D + 8)];
  __shared__ __attribute__((aligned(16))) unsigned short Kt[D * kTStr];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int I = blockIdx.x;
  for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
    const Walk wk = walk_of(a, b, I);
    const int c = b / a.group;
    const uint16_t* K = a.k.p + (long)c * a.k.stride;
    const uint16_t* V = a.v.p + (long)c * a.v.stride;
    const long row0 = (long)I * kB + 16 * w;
    uint16_t* dqrows = a.dq.p + (long)b * a.dq.stride + row0 * a.dq.ld;
    const int qlen = length_of<LENS>(a.q_lens, b / a.lens_div, a.own_rows);
    const int klen = length_of<LENS>(a.k_lens, b / a.lens_div, a.walk_rows);
    const int kblocks = LENS ? (klen + kB - 1) / kB : a.walk_blocks;
    if (LENS && (long)I * kB >= qlen) {  // the whole block is beyond the item's length
      store_zero<D>(dqrows, a.dq.ld, li, lg);
      if (lg == 0) a.delta[(long)b * a.own_rows + row0 + li] = 0.f;
      continue;
    }
    const bool dead = LENS && row0 + li >= qlen;
    uint4 qf[D / 32], gf[D / 32], of[D / 32];
    load_own<D>(qf, a.q.p + (long)b * a.q.stride + row0 * a.q.ld, a.q.ld, li, lg);
    load_own<D>(gf, a.dout.p + (long)b * a.dout.stride + row0 * a.dout.ld, a.dout.ld, li, lg);
    load_own<D>(of, a.o.p + (long)b * a.o.stride + row0 * a.o.ld, a.o.ld, li, lg);
    if (dead) {
      zero_own<D>(qf);
      zero_own<D>(gf);
      zero_own<D>(of);
    }
    float delta = 0.f;
#pragma unroll
    for (int s = 0; s < D / 32; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) delta = fmaf(up<T>((unsigned short)half_of(gf[s], e)), up<T>((unsigned short)half_of(of[s], e)), delta);
    delta = group_sum(delta);
    float lse = a.lse[(long)b * a.own_rows + row0 + li];
    if (dead) lse = -INFINITY;
    if (lg == 0) a.delta[(long)b * a.own_rows + row0 + li] = delta;
    f32x4 dq[D / 16];
    zero_acc<D>(dq);

    Tile<D> tk, tv;
    int p = next_block<CAUSAL, true>(wk.col, wk.beg, wk.end, I, kblocks);
    if (p < wk.end) {
      tk.template load<LENS>(K + (long)wk.col[p] * kB * a.k.ld, a.k.ld, tid, klen - wk.col[p] * kB);
      tv.template load<LENS>(V + (long)wk.col[p] * kB * a.v.ld, a.v.ld, tid, klen - wk.col[p] * kB);
    }
    while (p < wk.end) {
      const int J = wk.col[p];
      __syncthreads();
      tk.store_rows(Ks, tid);
      tk.store_transposed(Kt, tid);
      tv.store_rows(Vs, tid);
      __syncthreads();
      p = next_block<CAUSAL, true>(wk.col, p + 1, wk.end, I, kblocks);
      if (p < wk.end) {
        tk.template load<LENS>(K + (long)wk.col[p] * kB * a.k.ld, a.k.ld, tid, klen - wk.col[p] * kB);
        tv.template load<LENS>(V + (long)wk.col[p] * kB * a.v.ld, a.v.ld, tid, klen - wk.col[p] * kB);
      }
      const int kleft = klen - J * kB;
      f32x4 s[4], dp[4];
      score<T, D>(s, Ks, qf, li, lg);
      score<T, D>(dp, Vs, gf, li, lg);
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = s[f][r] * a.scale;
          if (CAUSAL && J == I && 16 * f + 4 * lg + r > 16 * w + li) t = -INFINITY;
          float pr = prob(t, lse);
          if (LENS && 16 * f + 4 * lg + r >= kleft) pr = 0.f;  // (the probability, not the score: the arithmetic above is
          s[f][r] = pr == 0.f ? 0.f : pr * (dp[f][r] - delta);  //  the no-lengths form's, operation for operation)
        }
      uint4 db[2];
      pack_tile<T>(db, s);
      accumulate<T, D>(dq, Kt, db, li, lg);
    }
    if (dead) zero_acc<D>(dq);
    store_own<T, D>(dq, a.scale, dqrows, a.dq.ld, li, lg);
    __syncthreads();
  }
}

// The walk of a key block over the query heads of its group: (g, p) is entry p of the transposed list of query item
// c · group + g, `end` that list's end.  Moves (g, p) to the next computed block at or after it, over the boundary between
// two heads' lists; p == end afterwards (with g == group − 1): the walk is over.
template <bool CAUSAL>
__device__ __forceinline__ void next_walk(const Args& a, int c, int J, int qblocks, int& g, int& p, int& end) {
  for (;;) {
    p = next_block<CAUSAL, false>(a.col, p, end, J, qblocks);
    if (p < end || g + 1 >= a.group) return;
    ++g;
    const Walk wk = walk_of(a, c * a.group + g, J);
    p = wk.beg, end = wk.end;
  }
}

// dK and dV over the transposed layout; own = k and v (a.rowptr / a.col are the transposed list, own_* the key side) of
// k / v item c, summed over the group's query items c · group + g, g ascending, each over its own transposed list.
template <class T, int D, bool CAUSAL, bool LENS>
__global__ __launch_bounds__(256) void block_attention_dkv_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) unsigned short Qs[kB * (D + 8)];
  __shared__ __attribute__((aligned(16))) unsigned short Gs[kB * (D + 8)];
  __shared__ __attribute__((aligned(16))) unsigned short Qt[D * kTStr];
  __shared__ __attribute__((aligned(16))) unsigned short Gt[D * kTStr];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int J = blockIdx.x;
  const int items = a.batch / a.group;
  for (int c = blockIdx.y; c < items; c += gridDim.y) {
    const long row0 = (long)J * kB + 16 * w;
    uint16_t* dkrows = a.dk.p + (long)c * a.dk.stride + row0 * a.dk.ld;
    uint16_t* dvrows = a.dv.p + (long)c * a.dv.stride + row0 * a.dv.ld;
    const int entry = (c * a.group) / a.lens_div;  // the heads of a group share one length
    const int qlen = length_of<LENS>(a.q_lens, entry, a.walk_rows);
    const int klen = length_of<LENS>(a.k_lens, entry, a.own_rows);
    const int qblocks = LENS ? (qlen + kB - 1) / kB : a.walk_blocks;
    if (LENS && (long)J * kB >= klen) {  // the whole block is beyond the item's length
      store_zero<D>(dvrows, a.dv.ld, li, lg);
      store_zero<D>(dkrows, a.dk.ld, li, lg);
      continue;
    }
    const bool dead = LENS && row0 + li >= klen;
    uint4 kf[D / 32], vf[D / 32];
    load_own<D>(kf, a.k.p + (long)c * a.k.stride + row0 * a.k.ld, a.k.ld, li, lg);
    load_own<D>(vf, a.v.p + (long)c * a.v.stride + row0 * a.v.ld, a.v.ld, li, lg);
    if (dead) {
      zero_own<D>(kf);
      zero_own<D>(vf);
    }
    f32x4 dk[D / 16], dv[D / 16];
    zero_acc<D>(dk);
    zero_acc<D>(dv);

    Tile<D> tq, tg;
    int g = 0, p, end;
    {
      const Walk wk = walk_of(a, c * a.group, J);
      p = wk.beg, end = wk.end;
    }
    next_walk<CAUSAL>(a, c, J, qblocks, g, p, end);
    if (p < end) {
      const long b = (long)c * a.group + g;
      tq.template load<LENS>(a.q.p + b * a.q.stride + (long)a.col[p] * kB * a.q.ld, a.q.ld, tid, qlen - a.col[p] * kB);
      tg.template load<LENS>(a.dout.p + b * a.dout.stride + (long)a.col[p] * kB * a.dout.ld, a.dout.ld, tid, qlen - a.col[p] * kB);
    }
    while (p < end) {
      const int I = a.col[p];
      const long bq = (long)c * a.group + g;  // the query item of this tile
      __syncthreads();
      tq.store_rows(Qs, tid);
      tq.store_transposed(Qt, tid);
      tg.store_rows(Gs, tid);
      tg.store_transposed(Gt, tid);
      __syncthreads();
      ++p;
      next_walk<CAUSAL>(a, c, J, qblocks, g, p, end);
      if (p < end) {  // the next tile's loads are in flight, across the boundary between two heads' lists too
        const long b = (long)c * a.group + g;
        tq.template load<LENS>(a.q.p + b * a.q.stride + (long)a.col[p] * kB * a.q.ld, a.q.ld, tid, qlen - a.col[p] * kB);
        tg.template load<LENS>(a.dout.p + b * a.dout.stride + (long)a.col[p] * kB * a.dout.ld, a.dout.ld, tid, qlen - a.col[p] * kB);
      }
      const float* lse = a.lse + bq * a.walk_rows + (long)I * kB;
      const float* delta = a.delta + bq * a.walk_rows + (long)I * kB;
      const int qleft = qlen - I * kB;  // queries of this block that exist
      f32x4 s[4], dp[4];
      score<T, D>(s, Qs, kf, li, lg);   // s[f][r]: query 16f + 4lg + r of block I against key li of the wave
      score<T, D>(dp, Gs, vf, li, lg);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const f32x4 ls = *reinterpret_cast<const f32x4*>(lse + 16 * f + 4 * lg);
        const f32x4 dl = *reinterpret_cast<const f32x4*>(delta + 16 * f + 4 * lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = s[f][r] * a.scale;
          if (CAUSAL && I == J && 16 * w + li > 16 * f + 4 * lg + r) t = -INFINITY;
          float pr = prob(t, ls[r]);
          if (LENS && (dead || 16 * f + 4 * lg + r >= qleft)) pr = 0.f;  // (the probability, not the score: as in dq)
          s[f][r] = pr;
          dp[f][r] = pr == 0.f ? 0.f : pr * (dp[f][r] - dl[r]);
        }
      }
      uint4 pb[2], db[2];
      pack_tile<T>(pb, s);
      pack_tile<T>(db, dp);
      accumulate<T, D>(dv, Gt, pb, li, lg);
      accumulate<T, D>(dk, Qt, db, li, lg);
    }
    if (dead) {
      zero_acc<D>(dk);
      zero_acc<D>(dv);
    }
    store_own<T, D>(dv, 1.f, dvrows, a.dv.ld, li, lg);
    store_own<T, D>(dk, a.scale, dkrows, a.dk.ld, li, lg);
    __syncthreads();
  }
}

bool takes_width(int32_t D) { return D == 32 || D == 64 || D == 96 || D == 128; }

// a [batch][rows][D] operand whose rows move as 16-byte pieces
bool dense_ok(const uint16_t* p, int64_t ld, int64_t stride, int32_t D) {
  return p != nullptr && mi::aligned16(p) && ld >= D && ld % 8 == 0 && stride >= 0 && stride % 8 == 0;
}

// The checks every entry makes before its first HIP call.  MI_OK with *empty set: nothing to compute.
int validate(int64_t nnz, int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk, int32_t D, int32_t causal, bool* empty) {
  *empty = false;
  if (nnz < 0 || layouts < 0 || batch < 0 || Sq < 0 || Sk < 0 || D < 0) return MI_EINVAL;
  if (nnz > 0x7fffffffLL) return MI_ERANGE;
  if (!takes_width(D) || Sq % kB != 0 || Sk % kB != 0) return MI_EINVAL;
  if (causal && Sq != Sk) return MI_EINVAL;
  if (batch == 0 || Sq == 0) {
    *empty = true;
    return MI_OK;
  }
  if (layouts == 0 || (nnz > 0 && Sk == 0)) return MI_EINVAL;
  return MI_OK;
}

// group and lengths of the _ex entries, checked before any HIP call (batch > 0): the k / v items and the length entries
// divide the query items, and the heads of a group share one length entry
int validate_ex(int32_t batch, int32_t group, const int32_t* q_lens, const int32_t* k_lens, int32_t lens_count) {
  if (group < 1 || batch % group != 0) return MI_EINVAL;
  if (q_lens == nullptr && k_lens == nullptr) return MI_OK;
  if (lens_count < 1 || batch % lens_count != 0 || (batch / lens_count) % group != 0) return MI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(q_lens) & 3u) || (reinterpret_cast<uintptr_t>(k_lens) & 3u)) return MI_EINVAL;
  return MI_OK;
}

void set_ex(Args& a, int32_t group, const int32_t* q_lens, const int32_t* k_lens, int32_t lens_count) {
  const bool lens = q_lens != nullptr || k_lens != nullptr;
  a.group = group, a.q_lens = q_lens, a.k_lens = k_lens, a.lens_div = lens ? a.batch / lens_count : a.batch;
}

// LENS is a compile-time form: a call without lengths runs kernels that hold no length arithmetic at all
template <class T, int D, bool CAUSAL, bool LENS>
int launch_fwd_form(const Args& a, hipStream_t s) {
  const dim3 grid((unsigned)a.own_blocks, (unsigned)(a.batch < 65535 ? a.batch : 65535));
  hipLaunchKernelGGL((block_attention_fwd_kernel<T, D, CAUSAL, LENS>), grid, dim3(256), 0, s, a);
  return mi::check_launch();
}

template <class T, int D>
int launch_fwd(const Args& a, bool causal, hipStream_t s) {
  const bool lens = a.q_lens != nullptr || a.k_lens != nullptr;
  if (causal) return lens ? launch_fwd_form<T, D, true, true>(a, s) : launch_fwd_form<T, D, true, false>(a, s);
  return lens ? launch_fwd_form<T, D, false, true>(a, s) : launch_fwd_form<T, D, false, false>(a, s);
}

template <class T, int D, bool CAUSAL, bool LENS>
int launch_bwd_form(const Args& aq, const Args& ak, hipStream_t s) {
  const unsigned gy = (unsigned)(aq.batch < 65535 ? aq.batch : 65535);
  hipLaunchKernelGGL((block_attention_dq_kernel<T, D, CAUSAL, LENS>), dim3((unsigned)aq.own_blocks, gy), dim3(256), 0, s, aq);
  const int st = mi::check_launch();
  if (st != MI_OK || ak.own_blocks == 0) return st;
  const int items = ak.batch / ak.group;  // a workgroup owns a key block of a k / v item
  const unsigned gk = (unsigned)(items < 65535 ? items : 65535);
  hipLaunchKernelGGL((block_attention_dkv_kernel<T, D, CAUSAL, LENS>), dim3((unsigned)ak.own_blocks, gk), dim3(256), 0, s, ak);
  return mi::check_launch();
}

template <class T, int D>
int launch_bwd(const Args& aq, const Args& ak, bool causal, hipStream_t s) {
  const bool lens = aq.q_lens != nullptr || aq.k_lens != nullptr;
  if (causal) return lens ? launch_bwd_form<T, D, true, true>(aq, ak, s) : launch_bwd_form<T, D, true, false>(aq, ak, s);
  return lens ? launch_bwd_form<T, D, false, true>(aq, ak, s) : launch_bwd_form<T, D, false, false>(aq, ak, s);
}

Dense dense(const uint16_t* p, int64_t ld, int64_t stride) { return Dense{const_cast<uint16_t*>(p), (long)ld, (long)stride}; }

template <class T>
int forward_entry(const int32_t* rowptr, const int32_t* col, int64_t nnz, int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk,
                  int32_t D, int32_t causal, const uint16_t* q, int64_t ldq, int64_t strideQ, const uint16_t* k, int64_t ldk,
                  int64_t strideK, const uint16_t* v, int64_t ldv, int64_t strideV, float scale, uint16_t* out, int64_t ldo,
                  int64_t strideO, float* lse, int32_t group, const int32_t* q_lens, const int32_t* k_lens, int32_t lens_count,
                  hipStream_t s) {
  if (group < 1) return MI_EINVAL;
  bool empty;
  const int st = validate(nnz, layouts, batch, Sq, Sk, D, causal, &empty);
  if (st != MI_OK || empty) return st;
  if (validate_ex(batch, group, q_lens, k_lens, lens_count) != MI_OK) return MI_EINVAL;
  if (!rowptr || !lse || (nnz > 0 && !col) || (reinterpret_cast<uintptr_t>(lse) & 3u)) return MI_EINVAL;
  if (!dense_ok(q, ldq, strideQ, D) || !dense_ok(out, ldo, strideO, D)) return MI_EINVAL;
  if (nnz > 0 && (!dense_ok(k, ldk, strideK, D) || !dense_ok(v, ldv, strideV, D))) return MI_EINVAL;
  Args a = {};
  a.rowptr = rowptr, a.col = col, a.nnz = nnz, a.layouts = layouts, a.batch = batch;
  a.own_blocks = Sq / kB, a.walk_blocks = Sk / kB, a.own_rows = Sq, a.walk_rows = Sk, a.scale = scale;
  a.q = dense(q, ldq, strideQ), a.k = dense(k, ldk, strideK), a.v = dense(v, ldv, strideV), a.o = dense(out, ldo, strideO);
  a.lse = lse;
  set_ex(a, group, q_lens, k_lens, lens_count);
  switch (D) {
    case 32: return launch_fwd<T, 32>(a, causal != 0, s);
    case 64: return launch_fwd<T, 64>(a, causal != 0, s);
    case 96: return launch_fwd<T, 96>(a, causal != 0, s);
    default: return launch_fwd<T, 128>(a, causal != 0, s);
  }
}

template <class T>
int backward_entry(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, int64_t nnz,
                   int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk, int32_t D, int32_t causal, const uint16_t* q,
                   int64_t ldq, int64_t strideQ, const uint16_t* k, int64_t ldk, int64_t strideK, const uint16_t* v, int64_t ldv,
                   int64_t strideV, const uint16_t* out, int64_t ldo, int64_t strideO, const uint16_t* dout, int64_t lddo,
                   int64_t strideDO, const float* lse, float scale, uint16_t* dq, int64_t lddq, int64_t strideDQ, uint16_t* dk,
                   int64_t lddk, int64_t strideDK, uint16_t* dv, int64_t lddv, int64_t strideDV, void* workspace,
                   size_t workspace_bytes, int32_t group, const int32_t* q_lens, const int32_t* k_lens, int32_t lens_count,
                   hipStream_t s) {
  if (group < 1) return MI_EINVAL;
  bool empty;
  const int st = validate(nnz, layouts, batch, Sq, Sk, D, causal, &empty);
  if (st != MI_OK || empty) return st;
  if (validate_ex(batch, group, q_lens, k_lens, lens_count) != MI_OK) return MI_EINVAL;
  if (!rowptr || !t_rowptr || !lse || (nnz > 0 && (!col || !t_col)) || !mi::aligned16(lse)) return MI_EINVAL;
  if (!dense_ok(q, ldq, strideQ, D) || !dense_ok(out, ldo, strideO, D) || !dense_ok(dout, lddo, strideDO, D) ||
      !dense_ok(dq, lddq, strideDQ, D))
    return MI_EINVAL;
  if (Sk > 0 && (!dense_ok(k, ldk, strideK, D) || !dense_ok(v, ldv, strideV, D) || !dense_ok(dk, lddk, strideDK, D) ||
                 !dense_ok(dv, lddv, strideDV, D)))
    return MI_EINVAL;
  if (!workspace || !mi::aligned16(workspace)) return MI_EINVAL;
  if (workspace_bytes < mi_block_attention_workspace_bytes(batch, Sq)) return MI_ENOMEM;
  Args aq = {};
  aq.rowptr = rowptr, aq.col = col, aq.nnz = nnz, aq.layouts = layouts, aq.batch = batch;
  aq.own_blocks = Sq / kB, aq.walk_blocks = Sk / kB, aq.own_rows = Sq, aq.walk_rows = Sk, aq.scale = scale;
  aq.q = dense(q, ldq, strideQ), aq.k = dense(k, ldk, strideK), aq.v = dense(v, ldv, strideV), aq.o = dense(out, ldo, strideO);
  aq.dout = dense(dout, lddo, strideDO), aq.dq = dense(dq, lddq, strideDQ), aq.dk = dense(dk, lddk, strideDK);
  aq.dv = dense(dv, lddv, strideDV);
  aq.lse = const_cast<float*>(lse), aq.delta = static_cast<float*>(workspace);
  set_ex(aq, group, q_lens, k_lens, lens_count);
  Args ak = aq;  // the key side owns: the transposed list, lse and δ indexed by the walk (query) rows
  ak.rowptr = t_rowptr, ak.col = t_col;
  ak.own_blocks = Sk / kB, ak.walk_blocks = Sq / kB, ak.own_rows = Sk, ak.walk_rows = Sq;
  switch (D) {
    case 32: return launch_bwd<T, 32>(aq, ak, causal != 0, s);
    case 64: return launch_bwd<T, 64>(aq, ak, causal != 0, s);
    case 96: return launch_bwd<T, 96>(aq, ak, causal != 0, s);
    default: return launch_bwd<T, 128>(aq, ak, causal != 0, s);
  }
}

}  // namespace

extern "C" {

size_t mi_block_attention_workspace_bytes(int32_t batch, int32_t Sq) {
  return batch > 0 && Sq > 0 ? (size_t)batch * (size_t)Sq * sizeof(float) : 0;
}

#define MI_BLOCK_FWD_ARGS                                                                                                    \
  const int32_t *rowptr, const int32_t *col, int64_t nnz, int32_t layouts, int32_t batch, int32_t Sq, int32_t Sk, int32_t D,  \
      int32_t causal, const uint16_t *q, int64_t ldq, int64_t strideQ, const uint16_t *k, int64_t ldk, int64_t strideK,      \
      const uint16_t *v, int64_t ldv, int64_t strideV, float scale, uint16_t *out, int64_t ldo, int64_t strideO, float *lse
#define MI_BLOCK_FWD_PASS \
  rowptr, col, nnz, layouts, batch, Sq, Sk, D, causal, q, ldq, strideQ, k, ldk, strideK, v, ldv, strideV, scale, out, ldo, strideO, lse

// the plain entries are the group = 1, no-lengths case of the _ex ones
#define MI_BLOCK_PLAIN 1, nullptr, nullptr, 0, static_cast<hipStream_t>(stream)
#define MI_BLOCK_EX group, q_lens, k_lens, lens_count, static_cast<hipStream_t>(stream)
#define MI_BLOCK_EX_ARGS int32_t group, const int32_t *q_lens, const int32_t *k_lens, int32_t lens_count, mi_stream_t stream

int mi_block_attention_fwd_bf16(MI_BLOCK_FWD_ARGS, mi_stream_t stream) { return forward_entry<Bf16>(MI_BLOCK_FWD_PASS, MI_BLOCK_PLAIN); }
int mi_block_attention_fwd_f16(MI_BLOCK_FWD_ARGS, mi_stream_t stream) { return forward_entry<F16>(MI_BLOCK_FWD_PASS, MI_BLOCK_PLAIN); }
int mi_block_attention_fwd_ex_bf16(MI_BLOCK_FWD_ARGS, MI_BLOCK_EX_ARGS) { return forward_entry<Bf16>(MI_BLOCK_FWD_PASS, MI_BLOCK_EX); }
int mi_block_attention_fwd_ex_f16(MI_BLOCK_FWD_ARGS, MI_BLOCK_EX_ARGS) { return forward_entry<F16>(MI_BLOCK_FWD_PASS, MI_BLOCK_EX); }

#define MI_BLOCK_BWD_ARGS                                                                                                      \
  const int32_t *rowptr, const int32_t *col, const int32_t *t_rowptr, const int32_t *t_col, int64_t nnz, int32_t layouts,       \
      int32_t batch, int32_t Sq, int32_t Sk, int32_t D, int32_t causal, const uint16_t *q, int64_t ldq, int64_t strideQ,       \
      const uint16_t *k, int64_t ldk, int64_t strideK, const uint16_t *v, int64_t ldv, int64_t strideV, const uint16_t *out,   \
      int64_t ldo, int64_t strideO, const uint16_t *dout, int64_t lddo, int64_t strideDO, const float *lse, float scale,       \
      uint16_t *dq, int64_t lddq, int64_t strideDQ, uint16_t *dk, int64_t lddk, int64_t strideDK, uint16_t *dv, int64_t lddv, \
      int64_t strideDV, void *workspace, size_t workspace_bytes
#define MI_BLOCK_BWD_PASS                                                                                                       \
  rowptr, col, t_rowptr, t_col, nnz, layouts, batch, Sq, Sk, D, causal, q, ldq, strideQ, k, ldk, strideK, v, ldv, strideV, out, \
      ldo, strideO, dout, lddo, strideDO, lse, scale, dq, lddq, strideDQ, dk, lddk, strideDK, dv, lddv, strideDV, workspace,    \
      workspace_bytes

int mi_block_attention_bwd_bf16(MI_BLOCK_BWD_ARGS, mi_stream_t stream) { return backward_entry<Bf16>(MI_BLOCK_BWD_PASS, MI_BLOCK_PLAIN); }
int mi_block_attention_bwd_f16(MI_BLOCK_BWD_ARGS, mi_stream_t stream) { return backward_entry<F16>(MI_BLOCK_BWD_PASS, MI_BLOCK_PLAIN); }
int mi_block_attention_bwd_ex_bf16(MI_BLOCK_BWD_ARGS, MI_BLOCK_EX_ARGS) { return backward_entry<Bf16>(MI_BLOCK_BWD_PASS, MI_BLOCK_EX); }
int mi_block_attention_bwd_ex_f16(MI_BLOCK_BWD_ARGS, MI_BLOCK_EX_ARGS) { return backward_entry<F16>(MI_BLOCK_BWD_PASS, MI_BLOCK_EX); }

}  // extern "C"
