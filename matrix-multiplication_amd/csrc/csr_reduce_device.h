// Pieces shared by the amax / amin translation units (csr_reduce.hip: float32; csr_reduce_lowp.hip: bfloat16 / float16):
// the selection steps, the hub-row list and its workspace layout (one layout, fp32 / int32 partials, for every dtype).
// Not installed.  Everything here has internal linkage (an anonymous namespace per including unit).
#ifndef MI_CSR_REDUCE_DEVICE_H_
#define MI_CSR_REDUCE_DEVICE_H_

#include "mi_common.h"

namespace {

constexpr int kHubRow = 8192;     // rows with more entries are split when the caller gave a workspace
constexpr int kHubChunk = 16384;  // entries per workgroup of a split row (S = max(1, len / kHubChunk))
constexpr int kHubWaves = 16;
constexpr int kU = 8;             // gathers in flight per lane

// One step of the sequential scan.
template <bool MAX>
__device__ __forceinline__ void scan(float p, int e, float& cur, int& arg) {
  const bool take = (MAX ? p > cur : p < cur) || __builtin_isnan(p);
  cur = take ? p : cur;
  arg = take ? e : arg;
}

// (cur, arg) ← the selection over the union of two scans of disjoint entry sets (order-independent).
template <bool MAX>
__device__ __forceinline__ void pick(float v, int a, float& cur, int& arg) {
  const bool vn = __builtin_isnan(v), cn = __builtin_isnan(cur);
  const bool take = vn ? (!cn || a > arg) : (!cn && ((MAX ? v > cur : v < cur) || (v == cur && a < arg)));
  cur = take ? v : cur;
  arg = take ? a : arg;
}

template <bool MAX>
__device__ __forceinline__ float scan_start() {
  return MAX ? -__builtin_inff() : __builtin_inff();
}

// Workspace (ints): [0] rows listed, [1] chunk slots handed out, [2] partial rows handed out, [3] –; cap_e entries of
// {row, slot base, S, partial base}; cap_s slot → entry; then (16-B aligned) cap_p × N floats and cap_p × N ints.
struct HubArg {
  int* ws;  // nullptr: no row is split
  int cap_e, cap_s, cap_p;
};

__device__ __forceinline__ void hub_append(const HubArg& h, int row, int len) {
  int* ws = h.ws;
  const int S = len / kHubChunk < 1 ? 1 : len / kHubChunk;
  const int e = atomicAdd(&ws[0], 1);
  const int sb = atomicAdd(&ws[1], S);
  const int pb = S > 1 ? atomicAdd(&ws[2], S) : 0;
  // the caps hold for any rowptr consistent with nnz; a lying rowptr must not write out of bounds
  if (e >= h.cap_e) return;
  const bool fits = sb + S <= h.cap_s && (S <= 1 || pb + S <= h.cap_p);
  int* ent = ws + 4 + 4 * (long)e;
  ent[0] = row;
  ent[1] = sb;
  ent[2] = fits ? S : 0;
  ent[3] = pb;
  if (!fits) return;
  int* owner = ws + 4 + 4 * (long)h.cap_e;
  for (int g = 0; g < S; ++g) owner[sb + g] = e;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct HubWs {
  long cap_e, cap_s, cap_p;
  size_t part_val_off, part_arg_off, bytes;
};
inline HubWs hub_ws_layout(int64_t nnz, int32_t N) {
  HubWs w;
  w.cap_e = nnz / kHubRow + 1;
  w.cap_p = nnz / kHubChunk;
  w.cap_s = w.cap_e + w.cap_p;
  const size_t ints = 4 + 4 * (size_t)w.cap_e + (size_t)w.cap_s;
  w.part_val_off = (ints * sizeof(int) + 15) / 16 * 16;
  w.part_arg_off = w.part_val_off + (size_t)w.cap_p * (size_t)N * sizeof(float);
  w.bytes = w.part_arg_off + (size_t)w.cap_p * (size_t)N * sizeof(int);
  return w;
}

// lanes per row for a width: a power of two with G·W ≥ N, at most a wave
template <int W>
inline int lanes_for(int32_t N) {
  const int need = (N + W - 1) / W;
  return need >= 64 ? 64 : mi::pow2_ceil(need);
}

inline bool grid_fits(int64_t rows, int lanes) { return (rows * lanes + 255) / 256 <= 0x7fffffffLL; }

}  // namespace

#endif  // MI_CSR_REDUCE_DEVICE_H_
