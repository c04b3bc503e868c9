// Query-aware key-block selection for decoding: every 64-key block of an item's cache is scored against the newest tokens'
// queries from its per-block key bounds (kv_block_bounds.hip) — the Quest upper bound — and the K best blocks of every token
// are written as an ascending list, the list that block_attention_decode.hip's list source walks.
//
// What it computes (contract of include/mi_spmm.h, mi_block_select_{bf16,f16}):
//  * Token t of k / v item c stands at pos = clamp(k_len, 0, Smax) − T + t; its candidates are the blocks J ≤ pos / 64.
//  * s_g(J) = Σ_d max(q[g,d] · lo[J,d], q[g,d] · hi[J,d]) in fp32 — q, lo, hi widened exactly, every product exact — and
//    score(J) = max_g s_g(J) over the `group` query heads of the item (fmaxf: a NaN s_g is passed over while another head has
//    a number).  THE ORDER OF THE SUM over d, fixed: four lanes share a block; lane l adds its terms d = 32i + 8l + e in
//    ascending (i, e) — i < D / 32, e < 8 — into one fp32 accumulator that starts at +0, and the four partials p0 … p3 are
//    joined as (p0 + p1) + (p2 + p3).  The max of the two products is taken before the addition, so nothing contracts.
//  * Order: score descending, block index ascending; −0 counts as +0; a NaN score ranks below every number, −inf included.
//  * Forced blocks — the candidates among the first `sink` blocks and the `local` blocks ending at pos / 64 — are always
//    listed and count toward K; the other slots go to the unforced candidates first in that order.  count = min(K,
//    candidates); the list is written in ASCENDING BLOCK INDEX, slots at or beyond count as −1; pos < 0: count 0.
//  * scores (optional) [items][T][blocks] float32: score(J) of every candidate, −inf for every other block.
//  * Bounds of non-candidates are never read.  The bits of a token's outputs depend on its own item's q, bounds, pos, K, sink
//    and local only.  No atomics — in LDS neither —, no read-back, fixed shapes: graph-capturable.
//
// Kernel: one workgroup of 1024 threads per (item, token).  The scores' ordered bit patterns go into LDS (64 KiB for the
// cap of 16 384 blocks = 1 M keys; gfx950 gives a workgroup 160 KiB); the key of the last chosen unforced candidate is found
// by a threshold search over those bits, four bits a round: a wave counts the keys at or above each of 15 trial thresholds
// with ballots, the 16 waves' counts meet in LDS, one barrier a round.  Emission is a prefix-sum compaction over contiguous
// index ranges — ascending order for free —, in which the ties at the threshold are taken lowest index first.  The search and
// the emission are block_select_device.h's select_and_emit, shared with block_select_tiles.hip.
#include "block_select_device.h"

namespace {

constexpr int kB = 64;
constexpr int kMaxGroup = 16;
constexpr int kThreads = kSelectThreads, kWavesWg = kSelectWaves;
constexpr int kMaxBlocks = kSelectMaxBlocks;  // the scores of one token in LDS: 64 KiB

struct Args {
  int heads, group, T, blocks, K, sink, local;
  long smax;
  const uint16_t* q;  // query head g of item c, token t: q + (c / heads) · batchQ + ((c % heads) · group + g) · headQ + t · ldq
  long ldq, headQ, batchQ;
  const uint16_t* bounds;  // [items][blocks][2][D]
  const int32_t* k_lens;   // [items / lens_div]
  int lens_div;
  int32_t* ids;     // [items][T][K]
  int32_t* counts;  // [items][T]
  float* scores;    // [items][T][blocks] or null
};

template <class T, int D>
__global__ __launch_bounds__(kThreads) void block_select_kernel(Args a) {
  __shared__ unsigned keys[kMaxBlocks];
  __shared__ __attribute__((aligned(16))) float qs[kMaxGroup * D];
  __shared__ unsigned wcnt[2][kWavesWg][16];
  __shared__ unsigned wtot[kWavesWg];
  const int tid = threadIdx.x;
  const int t = blockIdx.x, c = blockIdx.y;
  const int G = a.group, K = a.K;
  int klen = a.k_lens[c / a.lens_div];
  klen = klen < 0 ? 0 : klen > a.smax ? (int)a.smax : klen;
  const int pos = klen - a.T + t;
  const long tok = (long)c * a.T + t;
  int32_t* ids = a.ids + tok * K;
  float* sc_out = a.scores ? a.scores + tok * a.blocks : nullptr;
  int n = pos < 0 ? 0 : pos / kB + 1;  // candidates
  n = n > a.blocks ? a.blocks : n;
  if (sc_out)
    for (int J = n + tid; J < a.blocks; J += kThreads) sc_out[J] = -INFINITY;
  const int count = K < n ? K : n;
  for (int s = count + tid; s < K; s += kThreads) ids[s] = -1;
  if (tid == 0) a.counts[tok] = count;
  if (n == 0) return;

  // ---- scores ------------------------------------------------------------------------------------------------------
  {
    const int b = c / a.heads, h = c - b * a.heads;
    const uint16_t* qrow = a.q + (long)b * a.batchQ + (long)h * G * a.headQ + (long)t * a.ldq;
    for (int e = tid; e < G * D; e += kThreads) {
      const int g = e / D, d = e - g * D;
      qs[e] = T::lo(qrow[(long)g * a.headQ + d]);
    }
  }
  __syncthreads();
  const int l4 = tid & 3;
  for (int J = tid >> 2; J < n; J += kThreads / 4) {
    const uint16_t* bj = a.bounds + ((long)c * a.blocks + J) * 2 * D;
    float lo[D / 4], hi[D / 4];  // the lane's elements d = 32i + 8l + e of the block's two rows, widened
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
      const uint4 x = *reinterpret_cast<const uint4*>(bj + 32 * i + 8 * l4);
      const uint4 y = *reinterpret_cast<const uint4*>(bj + D + 32 * i + 8 * l4);
      const unsigned xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        lo[8 * i + 2 * p] = T::lo(xw[p]), lo[8 * i + 2 * p + 1] = T::hi(xw[p]);
        hi[8 * i + 2 * p] = T::lo(yw[p]), hi[8 * i + 2 * p + 1] = T::hi(yw[p]);
      }
    }
    float best = 0.f;
    for (int g = 0; g < G; ++g) {
      const float* qg = qs + g * D + 8 * l4;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < D / 32; ++i) {
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(qg + 32 * i), q1 = *reinterpret_cast<const f32x4*>(qg + 32 * i + 4);
        const float qe[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += fmaxf(qe[e] * lo[8 * i + e], qe[e] * hi[8 * i + e]);
      }
      acc += __shfl_xor(acc, 1);  // (p0 + p1), (p2 + p3)
      acc += __shfl_xor(acc, 2);  // … and their sum, in all four lanes
      best = g == 0 ? acc : fmaxf(best, acc);
    }
    if (l4 == 0) {
      keys[J] = key_of(best);
      if (sc_out) sc_out[J] = best;
    }
  }
  __syncthreads();

  select_and_emit(keys, wcnt, wtot, n, count, a.sink, a.local, ids, tid);
}

template <class T, int D>
int launch(const Args& a, int items, hipStream_t s) {
  hipLaunchKernelGGL((block_select_kernel<T, D>), dim3((unsigned)a.T, (unsigned)items), dim3(kThreads), 0, s, a);
  return mi::check_launch();
}

// Every check comes before the first HIP call.
template <class T>
int select_entry(int32_t items, int32_t heads, int32_t T_, int32_t Smax, int32_t D, int32_t group, const uint16_t* q, int64_t ldq,
                 int64_t headQ, int64_t batchQ, const uint16_t* bounds, const int32_t* k_lens, int32_t lens_count, int32_t K,
                 int32_t sink, int32_t local, int32_t* ids, int32_t* counts, float* scores, hipStream_t s) {
  if (!takes_width(D) || group < 1 || group > kMaxGroup) return MI_EINVAL;
  if (K < 1 || sink < 0 || local < 1 || (int64_t)sink + local > K) return MI_EINVAL;
  if (items < 0 || heads < 0 || T_ < 0 || Smax < 0 || Smax % kB != 0 || Smax / kB > kMaxBlocks) return MI_EINVAL;
  if (items > 65535) return MI_EINVAL;  // the grid's y
  if (items == 0 || T_ == 0) return MI_OK;
  if (heads == 0 || items % heads != 0 || lens_count < 1 || items % lens_count != 0) return MI_EINVAL;
  if (!k_lens || !aligned4(k_lens) || !ids || !aligned4(ids) || !counts || !aligned4(counts) || !aligned4(scores)) return MI_EINVAL;
  if (!q || !mi::aligned16(q) || !stride_ok(ldq) || !stride_ok(headQ) || !stride_ok(batchQ)) return MI_EINVAL;
  if (Smax > 0 && (!bounds || !mi::aligned16(bounds))) return MI_EINVAL;
  Args a = {};
  a.heads = heads, a.group = group, a.T = T_, a.blocks = Smax / kB, a.K = K, a.sink = sink, a.local = local, a.smax = Smax;
  a.q = q, a.ldq = ldq, a.headQ = headQ, a.batchQ = batchQ, a.bounds = bounds;
  a.k_lens = k_lens, a.lens_div = items / lens_count;
  a.ids = ids, a.counts = counts, a.scores = scores;
  switch (D) {
    case 32: return launch<T, 32>(a, items, s);
    case 64: return launch<T, 64>(a, items, s);
    case 96: return launch<T, 96>(a, items, s);
    default: return launch<T, 128>(a, items, s);
  }
}

}  // namespace

extern "C" {

int32_t mi_block_select_max_blocks(void) { return kMaxBlocks; }

#define MI_SELECT_ARGS                                                                                                          \
  int32_t items, int32_t heads, int32_t T, int32_t Smax, int32_t D, int32_t group, const uint16_t *q, int64_t ldq, int64_t headQ, \
      int64_t batchQ, const uint16_t *bounds, const int32_t *k_lens, int32_t lens_count, int32_t K, int32_t sink, int32_t local,  \
      int32_t *block_ids, int32_t *block_counts, float *scores, mi_stream_t stream
#define MI_SELECT_PASS                                                                                                        \
  items, heads, T, Smax, D, group, q, ldq, headQ, batchQ, bounds, k_lens, lens_count, K, sink, local, block_ids, block_counts, \
      scores, static_cast<hipStream_t>(stream)

int mi_block_select_bf16(MI_SELECT_ARGS) { return select_entry<Bf16>(MI_SELECT_PASS); }
int mi_block_select_f16(MI_SELECT_ARGS) { return select_entry<F16>(MI_SELECT_PASS); }

}  // extern "C"
