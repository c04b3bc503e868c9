// What the two key-block selection units — block_select.hip (one list per token) and block_select_tiles.hip (one
// list per position tile, §3.33) — say alike once the scores of a row's candidates stand in LDS as ordered keys: the key of a
// score, the threshold search for the key of the last chosen unforced candidate and the emission of the list in ascending block
// index.  A function of keys[], n, count, sink, local and the row pointer alone.  Not installed.  Everything here has internal
// linkage (an anonymous namespace per including unit).
#ifndef MI_BLOCK_SELECT_DEVICE_H_
#define MI_BLOCK_SELECT_DEVICE_H_

#include "kv_cache_device.h"

namespace {

constexpr int kSelectThreads = 1024, kSelectWaves = kSelectThreads / 64;
constexpr int kSelectMaxBlocks = 16384;  // the scores of one row in LDS: 64 KiB

// a score as an unsigned key of the selection's order: NaN lowest, −0 as +0
__device__ __forceinline__ unsigned key_of(float s) {
  if (s != s) return 0u;
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The list of one row from the keys of its n candidates (all of them written, a barrier passed): `count` ≤ n entries into ids[]
// in ascending block index.  Forced — always listed — are the candidates J < sink and J ≥ n − local; the other slots go to the
// rest in (key descending, index ascending).  The key of the last chosen unforced candidate is found by a threshold search over
// the keys' bits, four bits a round: a wave counts the keys at or above each of 15 trial thresholds with ballots, the 16
// waves' counts meet in wcnt, one barrier a round.  Emission is a prefix-sum compaction over contiguous index ranges —
// ascending order for free —, in which the ties at the threshold are taken lowest index first.  Called by all 1024 threads of
// the workgroup; wcnt and wtot are its scratch in LDS.
__device__ __forceinline__ void select_and_emit(const unsigned* keys, unsigned (&wcnt)[2][kSelectWaves][16], unsigned (&wtot)[kSelectWaves],
                                                int n, int count, int sink, int local, int32_t* ids, int tid) {
  constexpr int kThreads = kSelectThreads, kWavesWg = kSelectWaves;
  const int lane = tid & 63, wave = tid >> 6;
  // ---- the threshold: the key of the last chosen unforced candidate ------------------------------------------------------
  const int sinkN = sink < n ? sink : n;                        // forced: J < sinkN …
  const int localFrom = n - local > sinkN ? n - local : sinkN;  // … or J ≥ localFrom
  const int forced = sinkN + (n - localFrom);
  const int R = count - forced;  // slots of the unforced candidates (sink + local ≤ K: never negative)
  const int U = n - forced;      // unforced candidates
  unsigned th = 0u;              // chosen: key > th, and the lowest-index ties key == th that still fit
  const bool all = R >= U, none = R <= 0;
  if (!all && !none) {
    for (int round = 0; round < 8; ++round) {
      const int shift = 28 - 4 * round;
      unsigned cnt[15];
#pragma unroll
      for (int d = 0; d < 15; ++d) cnt[d] = 0u;
      for (int J0 = sinkN + wave * 64; J0 < localFrom; J0 += kThreads) {  // (a wave-uniform bound: every lane votes)
        const int J = J0 + lane;
        const bool in = J < localFrom;
        const unsigned key = in ? keys[J] : 0u;
#pragma unroll
        for (int d = 0; d < 15; ++d)
          cnt[d] += (unsigned)__popcll(__ballot(in && key >= (th | ((unsigned)(d + 1) << shift))));
      }
      unsigned(*buf)[16] = wcnt[round & 1];
      if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 15; ++d) buf[wave][d + 1] = cnt[d];
      }
      __syncthreads();
      // lane d of 1 … 15 adds the waves' counts of digit d; the counts fall with d, so the lanes that reach R are a prefix
      unsigned tot = 0u;
      const int d = lane & 15;
      if (d > 0)
        for (int w = 0; w < kWavesWg; ++w) tot += buf[w][d];
      const unsigned long long reach = __ballot(lane > 0 && lane < 16 && tot >= (unsigned)R);
      const int digit = reach ? 63 - __clzll(reach) : 0;
      th |= (unsigned)digit << shift;
    }
  }

  // ---- emission: a prefix sum over contiguous index ranges -------------------------------------------------------------------
  const int per = (n + kThreads - 1) / kThreads;
  const int beg = tid * per < n ? tid * per : n, end = beg + per < n ? beg + per : n;
  unsigned mine = 0u;  // chosen for certain (low half) and ties at the threshold (high half) of this thread's range
  for (int J = beg; J < end; ++J) {
    const bool f = J < sinkN || J >= localFrom;
    const unsigned key = keys[J];
    const bool sure = f || all || (!none && key > th);
    const bool tie = !f && !all && !none && key == th;
    mine += (sure ? 1u : 0u) + (tie ? 0x10000u : 0u);
  }
  unsigned incl = mine;  // (n ≤ 16 384: neither half overflows its 16 bits)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  unsigned before = incl - mine, total = 0u;
  for (int w = 0; w < kWavesWg; ++w) {
    const unsigned x = wtot[w];
    if (w < wave) before += x;
    total += x;
  }
  const int ties_taken = count - (int)(total & 0xffffu);  // ties that still fit, lowest index first
  int sure_before = (int)(before & 0xffffu), tie_before = (int)(before >> 16);
  for (int J = beg; J < end; ++J) {
    const bool f = J < sinkN || J >= localFrom;
    const unsigned key = keys[J];
    const bool sure = f || all || (!none && key > th);
    const bool tie = !f && !all && !none && key == th;
    if (sure || (tie && tie_before < ties_taken)) {
      const int slot = sure_before + (tie_before < ties_taken ? tie_before : ties_taken);
      // (always: the guard keeps a wrong count inside the row — on both sides: with more sure candidates than slots
      // ties_taken, and with it the slot, would be negative)
      if ((unsigned)slot < (unsigned)count) ids[slot] = J;
    }
    sure_before += sure ? 1 : 0;
    tie_before += tie ? 1 : 0;
  }
}

}  // namespace

#endif  // MI_BLOCK_SELECT_DEVICE_H_
