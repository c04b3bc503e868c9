// Query-aware key-block selection for CHUNKED PREFILL: every 64-key block of an item's cache is scored against the queries of a
// whole 64-position tile of the chunk on the matrix cores, and the K best blocks of every tile are written as an ascending
// list — the list that block_attention_prefill.hip's list source walks.  block_select.hip (§3.29) gives one
// list per token; the prefill walk shares one walk among the 64 positions of a tile, and a per-token selection over a
// 2048-token chunk would cost about what the dense attention does.
//
// What it computes (contract of include/mi_spmm.h, mi_block_select_tiles_{bf16,f16}):
//  * Geometry: the prefill walk's Geom, word for word.  With klen = clamp(k_len, 0, Smax), n = clamp(new_len, 0, T) (T without
//    new_lens), start = klen − T and first = max(klen − n, 0), tile x of item c is layout row r = ⌊start / 64⌋ + x; its tokens
//    are the positions pos ∈ [64r, 64r + 64) with first ≤ pos < klen and slot t = pos − start ∈ [0, T).  A tile without a
//    token: count 0, a row of −1, scores −inf.  Else 0 ≤ r < blocks, and the candidates are the blocks J ≤ r.
//  * The Quest score Σ_d max(q_d · lo_d, q_d · hi_d) is q⁻ · lo + q⁺ · hi with q⁺ = max(q, 0), q⁻ = min(q, 0) (lo ≤ hi) — and a
//    row of bounds [c][J] is [lo | hi] already, 2·D contiguous elements.  So s_{t,g}(J) = [q⁻ | q⁺]_{t,g} · [lo | hi]_Jᵀ, fp32 on
//    the matrix cores: mfma<T> 16 × 16 × 32, the 2·D / 32 MFMAs of one accumulator issued in ascending k from +0.  (q⁻ keeps
//    the elements whose sign bit is set, q⁺ the others; the other half holds +0.)
//    score(J) = max over the tile's tokens and the `group` heads of s_{t,g}(J), by fmaxf from a NaN: a NaN term is passed over
//    while another is a number; a slot without a token takes no part — its zero row would give a 0.
//  * Order, forced blocks (the first `sink` and the `local` ending at r), count = min(K, candidates), the list in ASCENDING
//    BLOCK INDEX, −1 from count on: block_select.hip's, through block_select_device.h's select_and_emit.
//  * scores (optional) [items][X][blocks] float32: score(J) of every candidate, −inf elsewhere.  The selection is an exact
//    function of these.  Bounds of non-candidates are never read; q of a slot without a token is never read.
//  * With an inf or NaN in q or bounds the product form may give NaN (0 · inf) where the per-token kernel has a number: then
//    only the structure holds — the count, ascending distinct candidates, every forced block, no store outside the row.
//  * The bits of a tile's outputs depend on its own item's q, bounds, klen, new_len, its positions, K, sink and local only.
//    No atomics, no read-back, fixed shapes: graph-capturable.
//
// Kernel: one workgroup of 1024 threads per (tile, item).  Per head g of the group, the image [64 tokens][2·D + 8] of
// [q⁻ | q⁺] is staged in LDS (the staged-row stride: 16 rows of a fragment read on 16 different 16-byte bank slots); a wave
// takes 16 blocks at a time — 256 a pass of the 16 waves —, their [lo | hi] rows loaded straight from global memory as B
// fragments, 16 bytes a lane (the way the prefill walk loads qf); 4 token sub-tiles × 2·D / 32 MFMAs (a sub-tile without a
// token is skipped); acc[r] of lane (li, lg) is token 16f + 4lg + r against block li, so the max over the tokens is taken in
// registers and with two __shfl_xor.  The running max over the heads stands in keys[] as float bits — block J is always the
// same lane's — and becomes key_of(best) with the last head.
#include "block_select_device.h"
#include "mfma_device.h"

namespace {

constexpr int kB = 64;
constexpr int kMaxGroup = 16;
constexpr int kThreads = kSelectThreads, kWavesWg = kSelectWaves;
constexpr int kMaxBlocks = kSelectMaxBlocks;

struct Args {
  int heads, group, T, tiles, blocks, K, sink, local;
  long smax;
  const uint16_t* q;  // query head g of item c, token t: q + (c / heads) · batchQ + ((c % heads) · group + g) · headQ + t · ldq
  long ldq, headQ, batchQ;
  const uint16_t* bounds;  // [items][blocks][2][D]
  const int32_t* k_lens;   // [items / lens_div]
  int lens_div;
  const int32_t* new_lens;  // [B] or [1], clamped to [0, T] where read; null: T
  int new_lens_one;
  int32_t* ids;     // [items][tiles][K]
  int32_t* counts;  // [items][tiles]
  float* scores;    // [items][tiles][blocks] or null
};

// the halves of a word of two elements whose sign bit is set, as a mask
__device__ __forceinline__ unsigned negative_halves(unsigned w) { return ((w >> 15) & 0x00010001u) * 0xffffu; }

template <class T, int D>
__global__ __launch_bounds__(kThreads) void block_select_tiles_kernel(Args a) {
  constexpr int kRow = 2 * D + 8;  // elements of an image row
  __shared__ unsigned keys[kMaxBlocks];
  __shared__ __attribute__((aligned(16))) unsigned short img[kB * kRow];
  __shared__ unsigned wcnt[2][kWavesWg][16];
  __shared__ unsigned wtot[kWavesWg];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int x = blockIdx.x, c = blockIdx.y;
  const int G = a.group, K = a.K;
  const int bi = c / a.heads, h = c - bi * a.heads;
  // the prefill walk's geometry
  int klen = a.k_lens[c / a.lens_div];
  klen = klen < 0 ? 0 : klen > a.smax ? (int)a.smax : klen;
  int nn = a.T;
  if (a.new_lens) {
    nn = a.new_lens[a.new_lens_one ? 0 : bi];
    nn = nn < 0 ? 0 : nn > a.T ? a.T : nn;
  }
  const int start = klen - a.T;
  const int first = klen - nn < 0 ? 0 : klen - nn;
  const int r = (start >> 6) + x;
  const bool any = first < klen && r * kB + kB > first && r * kB < klen;  // then 0 ≤ r < blocks
  const long row = (long)c * a.tiles + x;
  int32_t* ids = a.ids + row * K;
  float* sc_out = a.scores ? a.scores + row * a.blocks : nullptr;
  int n = any ? r + 1 : 0;  // candidates
  n = n > a.blocks ? a.blocks : n;
  if (sc_out)
    for (int J = n + tid; J < a.blocks; J += kThreads) sc_out[J] = -INFINITY;
  const int count = K < n ? K : n;
  for (int s = count + tid; s < K; s += kThreads) ids[s] = -1;
  if (tid == 0) a.counts[row] = count;
  if (n == 0) return;

  // own row i of the tile stands at pos = 64r + i, slot pos − start; bit i: it holds a token
  const int lo_pos = first > r * kB ? first : r * kB, hi_pos = klen < r * kB + kB ? klen : r * kB + kB;  // tokens: [lo_pos, hi_pos)
  const int i0 = lo_pos - r * kB, i1 = hi_pos - r * kB;                                                   // 0 ≤ i0 < i1 ≤ 64
  const unsigned long long below1 = i1 >= 64 ? ~0ull : (1ull << i1) - 1ull;
  const unsigned long long tokens = below1 & ~((1ull << i0) - 1ull);

  const uint16_t* qhead = a.q + (long)bi * a.batchQ + (long)h * G * a.headQ;
  const uint16_t* brow = a.bounds + (long)c * a.blocks * 2 * D;
  for (int g = 0; g < G; ++g) {
    // ---- the image of head g: row i = [q⁻ | q⁺] of the token at pos 64r + i, zeros for a slot without one ------------------------
    if (g > 0) __syncthreads();  // the previous head's fragment reads are done
    for (int e = tid; e < kB * (D / 8); e += kThreads) {
      const int i = e / (D / 8), p = e - i * (D / 8);
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if ((tokens >> i) & 1ull) {
        const long t = (long)r * kB + i - start;  // in [0, T): first ≥ start and pos < klen
        v = *reinterpret_cast<const uint4*>(qhead + (long)g * a.headQ + t * a.ldq + 8 * p);
      }
      const uint4 m = uint4{negative_halves(v.x), negative_halves(v.y), negative_halves(v.z), negative_halves(v.w)};
      *reinterpret_cast<uint4*>(img + i * kRow + 8 * p) = uint4{v.x & m.x, v.y & m.y, v.z & m.z, v.w & m.w};
      *reinterpret_cast<uint4*>(img + i * kRow + D + 8 * p) = uint4{v.x & ~m.x, v.y & ~m.y, v.z & ~m.z, v.w & ~m.w};
    }
    __syncthreads();
    // ---- 16 blocks a wave and turn --------------------------------------------------------------------------------------------
    for (int J0 = wave * 16; J0 < n; J0 += kWavesWg * 16) {  // (wave-uniform)
      const int J = J0 + li;
      uint4 bf[2 * D / 32];  // block J's [lo | hi] row as B fragments: lane (li, lg) holds elements 32s + 8lg … + 7
#pragma unroll
      for (int s = 0; s < 2 * D / 32; ++s) bf[s] = uint4{0u, 0u, 0u, 0u};
      if (J < n) {
#pragma unroll
        for (int s = 0; s < 2 * D / 32; ++s) bf[s] = *reinterpret_cast<const uint4*>(brow + (long)J * 2 * D + 32 * s + 8 * lg);
      }
      float best = __builtin_nanf("");
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (((tokens >> (16 * f)) & 0xffffull) == 0ull) continue;  // (workgroup-uniform) no token in the sub-tile
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2 * D / 32; ++s) {
          const uint4 af = *reinterpret_cast<const uint4*>(img + (16 * f + li) * kRow + 32 * s + 8 * lg);
          acc = mfma<T>(af, bf[s], acc);
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          if ((tokens >> (16 * f + 4 * lg + rr)) & 1ull) best = fmaxf(best, acc[rr]);
      }
      best = fmaxf(best, __shfl_xor(best, 16));
      best = fmaxf(best, __shfl_xor(best, 32));
      if (lg == 0 && J < n) {
        if (g > 0) best = fmaxf(__uint_as_float(keys[J]), best);
        if (g + 1 < G) {
          keys[J] = __float_as_uint(best);
        } else {
          keys[J] = key_of(best);
          if (sc_out) sc_out[J] = best;
        }
      }
    }
  }
  __syncthreads();
  select_and_emit(keys, wcnt, wtot, n, count, a.sink, a.local, ids, tid);
}

template <class T, int D>
int launch(const Args& a, int items, hipStream_t s) {
  hipLaunchKernelGGL((block_select_tiles_kernel<T, D>), dim3((unsigned)a.tiles, (unsigned)items), dim3(kThreads), 0, s, a);
  return mi::check_launch();
}

// Every check comes before the first HIP call, in block_select.hip's select_entry's order; new_lens is this entry's own.
template <class T>
int select_tiles_entry(int32_t items, int32_t heads, int32_t T_, int32_t Smax, int32_t D, int32_t group, const uint16_t* q, int64_t ldq,
                       int64_t headQ, int64_t batchQ, const uint16_t* bounds, const int32_t* k_lens, int32_t lens_count,
                       const int32_t* new_lens, int32_t new_lens_count, int32_t K, int32_t sink, int32_t local, int32_t* ids,
                       int32_t* counts, float* scores, hipStream_t s) {
  if (!takes_width(D) || group < 1 || group > kMaxGroup) return MI_EINVAL;
  if (K < 1 || sink < 0 || local < 1 || (int64_t)sink + local > K) return MI_EINVAL;
  if (items < 0 || heads < 0 || T_ < 0 || Smax < 0 || Smax % kB != 0 || Smax / kB > kMaxBlocks) return MI_EINVAL;
  if (items > 65535) return MI_EINVAL;  // the grid's y
  if (items == 0 || T_ == 0) return MI_OK;
  if (heads == 0 || items % heads != 0 || lens_count < 1 || items % lens_count != 0) return MI_EINVAL;
  if (!k_lens || !aligned4(k_lens) || !ids || !aligned4(ids) || !counts || !aligned4(counts) || !aligned4(scores)) return MI_EINVAL;
  if (new_lens && (!aligned4(new_lens) || (new_lens_count != 1 && new_lens_count != items / heads))) return MI_EINVAL;
  if (!q || !mi::aligned16(q) || !stride_ok(ldq) || !stride_ok(headQ) || !stride_ok(batchQ)) return MI_EINVAL;
  if (Smax > 0 && (!bounds || !mi::aligned16(bounds))) return MI_EINVAL;
  Args a = {};
  a.heads = heads, a.group = group, a.T = T_, a.tiles = (int)(((long)T_ + kB - 1) / kB + 1), a.blocks = Smax / kB;
  a.K = K, a.sink = sink, a.local = local, a.smax = Smax;
  a.q = q, a.ldq = ldq, a.headQ = headQ, a.batchQ = batchQ, a.bounds = bounds;
  a.k_lens = k_lens, a.lens_div = items / lens_count;
  a.new_lens = new_lens, a.new_lens_one = new_lens_count == 1;
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

#define MI_SELECT_TILES_PASS                                                                                                   \
  items, heads, T, Smax, D, group, q, ldq, headQ, batchQ, bounds, k_lens, lens_count, new_lens, new_lens_count, K, sink, local, \
      block_ids, block_counts, scores, static_cast<hipStream_t>(stream)

int mi_block_select_tiles_bf16(MI_BLOCK_SELECT_TILES_OPERANDS) { return select_tiles_entry<Bf16>(MI_SELECT_TILES_PASS); }
int mi_block_select_tiles_f16(MI_BLOCK_SELECT_TILES_OPERANDS) { return select_tiles_entry<F16>(MI_SELECT_TILES_PASS); }

}  // extern "C"
