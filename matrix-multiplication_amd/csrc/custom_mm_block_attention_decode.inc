// custom_mm — block-sparse attention for decoding: the newest tokens of every item against a key / value cache, in its four
// forms — contiguous or paged, 2-byte or FP8 (OCP e4m3fn)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands (DESIGN.md §3.23) and about a reading call (§3.31).  Not compiled on its
// own.  Contract: include/mi_spmm.h, "Block-sparse attention for decoding", "… over a paged cache", "… over an FP8 cache" (DESIGN.md §3.18–§3.20): q and out
// [B, Hq, T, D] contiguous, bfloat16 or float16; the cache of q's type or float8_e4m3fn; offsets int32 [layouts, Smax/64 + 1]
// with the layouts' bases, columns int32 layout-local, in 64-blocks; lse float32 [B, Hq, T].  The workspace of the chunks'
// partials comes from torch's allocator.

// all four forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D];
// `fp8`: a cache of e4m3fn bytes with the two scales.  Its own: chunk, the layout, q contiguous, the workspace, the C entry.
torch::Tensor block_attention_decode_impl(const char* what, const char* kname, const char* vname, bool fp8, const torch::Tensor& offsets,
                                          const torch::Tensor& columns, int64_t nnz, const torch::Tensor& q, const torch::Tensor& k,
                                          const torch::Tensor& v, const torch::Tensor* table, const torch::Tensor& k_lens, double scale,
                                          const c10::optional<torch::Tensor>& k_scale, const c10::optional<torch::Tensor>& v_scale,
                                          int64_t chunk, torch::Tensor out, const torch::Tensor& lse,
                                          const torch::Tensor* tree = nullptr, const WindowOperand* win = nullptr) {
  TORCH_CHECK(!(tree && win), what, ": a tree mask and a window do not go together");
  if (win) check_window(what, *win);
  const ReadShape s = read_shape(what, kname, vname, fp8, q, k, v, table, out);
  TORCH_CHECK(chunk >= 1 && chunk <= INT32_MAX, what, ": chunk must be a positive int32, got ", chunk);
  const int64_t Smax = read_smax(what, k, table, s.B);
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Smax, Smax);
  check_same_device(what, lay.list.device, {&q, &k, &v});
  check_read_operands(what, lay.list.device, true, q, table, k_lens, out, lse, s);
  const ReadCache r = read_cache(what, kname, vname, fp8, q, k, v, table, k_scale, v_scale, s);
  std::pair<const int64_t*, int32_t> tm = {nullptr, 0};
  if (tree) tm = tree_mask_operand(what, *tree, s.B, s.T, lay.list.device);
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)(s.B * s.Hkv), (int32_t)s.T, (int32_t)s.group, (int32_t)s.D,
                                                                    (int32_t)Smax, (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
// the argument lists of the eight C entries, in pieces: MI_READ_TABLE and MI_READ_SCALES are what the paged and the fp8 entries add
#define MI_DECODE_LIST lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, MI_READ_SIZES
#define MI_DECODE_OPERANDS(CT) (int32_t) s.D, bits16(q), s.D, s.T* s.D, MI_READ_CACHE(CT), (int32_t)s.group, (int32_t)chunk, (float)scale
#define MI_DECODE_OUT MI_READ_OUT, ws.data_ptr(), ws_bytes, stream_of(out)
#define MI_DECODE_TREE tm.first, tm.second
#define MI_DECODE_WINDOW (int32_t) win->window, (int32_t)win->sink
  int st;
  if (win && !fp8)
    st = table ? (s.bf ? mi_block_attention_window_decode_paged_bf16 : mi_block_attention_window_decode_paged_f16)(
                     MI_DECODE_LIST, MI_READ_TABLE, MI_DECODE_OPERANDS(uint16_t), MI_DECODE_WINDOW, MI_DECODE_OUT)
               : (s.bf ? mi_block_attention_window_decode_bf16 : mi_block_attention_window_decode_f16)(
                     MI_DECODE_LIST, MI_DECODE_OPERANDS(uint16_t), MI_DECODE_WINDOW, MI_DECODE_OUT);
  else if (win)
    st = table ? (s.bf ? mi_block_attention_window_decode_paged_fp8_bf16 : mi_block_attention_window_decode_paged_fp8_f16)(
                     MI_DECODE_LIST, MI_READ_TABLE, MI_DECODE_OPERANDS(uint8_t), MI_READ_SCALES, MI_DECODE_WINDOW, MI_DECODE_OUT)
               : (s.bf ? mi_block_attention_window_decode_fp8_bf16 : mi_block_attention_window_decode_fp8_f16)(
                     MI_DECODE_LIST, MI_DECODE_OPERANDS(uint8_t), MI_READ_SCALES, MI_DECODE_WINDOW, MI_DECODE_OUT);
  else if (tree && !fp8)
    st = table ? (s.bf ? mi_block_attention_tree_decode_paged_bf16 : mi_block_attention_tree_decode_paged_f16)(
                     MI_DECODE_LIST, MI_READ_TABLE, MI_DECODE_OPERANDS(uint16_t), MI_DECODE_TREE, MI_DECODE_OUT)
               : (s.bf ? mi_block_attention_tree_decode_bf16 : mi_block_attention_tree_decode_f16)(
                     MI_DECODE_LIST, MI_DECODE_OPERANDS(uint16_t), MI_DECODE_TREE, MI_DECODE_OUT);
  else if (tree)
    st = table ? (s.bf ? mi_block_attention_tree_decode_paged_fp8_bf16 : mi_block_attention_tree_decode_paged_fp8_f16)(
                     MI_DECODE_LIST, MI_READ_TABLE, MI_DECODE_OPERANDS(uint8_t), MI_READ_SCALES, MI_DECODE_TREE, MI_DECODE_OUT)
               : (s.bf ? mi_block_attention_tree_decode_fp8_bf16 : mi_block_attention_tree_decode_fp8_f16)(
                     MI_DECODE_LIST, MI_DECODE_OPERANDS(uint8_t), MI_READ_SCALES, MI_DECODE_TREE, MI_DECODE_OUT);
  else if (!fp8)
    st = table ? (s.bf ? mi_block_attention_decode_paged_bf16 : mi_block_attention_decode_paged_f16)(
                     MI_DECODE_LIST, MI_READ_TABLE, MI_DECODE_OPERANDS(uint16_t), MI_DECODE_OUT)
               : (s.bf ? mi_block_attention_decode_bf16 : mi_block_attention_decode_f16)(MI_DECODE_LIST, MI_DECODE_OPERANDS(uint16_t),
                                                                                       MI_DECODE_OUT);
  else
    st = table ? (s.bf ? mi_block_attention_decode_paged_fp8_bf16 : mi_block_attention_decode_paged_fp8_f16)(
                     MI_DECODE_LIST, MI_READ_TABLE, MI_DECODE_OPERANDS(uint8_t), MI_READ_SCALES, MI_DECODE_OUT)
               : (s.bf ? mi_block_attention_decode_fp8_bf16 : mi_block_attention_decode_fp8_f16)(
                     MI_DECODE_LIST, MI_DECODE_OPERANDS(uint8_t), MI_READ_SCALES, MI_DECODE_OUT);
#undef MI_DECODE_LIST
#undef MI_DECODE_OPERANDS
#undef MI_DECODE_OUT
#undef MI_DECODE_TREE
#undef MI_DECODE_WINDOW
  check_status(st, what);
  return out;
}

torch::Tensor block_attention_decode(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                     torch::Tensor v, torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out,
                                     torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_decode", "k", "v", false, offsets, columns, nnz, q, k, v, nullptr, k_lens, scale,
                                     c10::nullopt, c10::nullopt, chunk, out, lse);
}

torch::Tensor block_attention_decode_paged(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                           torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                           torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_decode_paged", "k_pages", "v_pages", false, offsets, columns, nnz, q, k_pages,
                                     v_pages, &block_table, k_lens, scale, c10::nullopt, c10::nullopt, chunk, out, lse);
}

torch::Tensor block_attention_decode_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                         torch::Tensor v, torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                         c10::optional<torch::Tensor> v_scale, int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_decode_fp8", "k", "v", true, offsets, columns, nnz, q, k, v, nullptr, k_lens,
                                     scale, k_scale, v_scale, chunk, out, lse);
}

torch::Tensor block_attention_decode_paged_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                               torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                               torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                               c10::optional<torch::Tensor> v_scale, int64_t chunk, torch::Tensor out,
                                               torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_decode_paged_fp8", "k_pages", "v_pages", true, offsets, columns, nnz, q, k_pages,
                                     v_pages, &block_table, k_lens, scale, k_scale, v_scale, chunk, out, lse);
}

// … with a tree mask (DESIGN.md §3.34): the four bindings above with `tree_mask` int64 [B, T] or [T] before chunk
torch::Tensor block_attention_tree_decode(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, torch::Tensor k_lens, double scale, torch::Tensor tree_mask, int64_t chunk,
                                          torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_tree_decode", "k", "v", false, offsets, columns, nnz, q, k, v, nullptr, k_lens,
                                     scale, c10::nullopt, c10::nullopt, chunk, out, lse, &tree_mask);
}

torch::Tensor block_attention_tree_decode_paged(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                torch::Tensor k_lens, double scale, torch::Tensor tree_mask, int64_t chunk,
                                                torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_tree_decode_paged", "k_pages", "v_pages", false, offsets, columns, nnz, q, k_pages,
                                     v_pages, &block_table, k_lens, scale, c10::nullopt, c10::nullopt, chunk, out, lse, &tree_mask);
}

torch::Tensor block_attention_tree_decode_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                              torch::Tensor v, torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                              c10::optional<torch::Tensor> v_scale, torch::Tensor tree_mask, int64_t chunk,
                                              torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_tree_decode_fp8", "k", "v", true, offsets, columns, nnz, q, k, v, nullptr, k_lens,
                                     scale, k_scale, v_scale, chunk, out, lse, &tree_mask);
}

torch::Tensor block_attention_tree_decode_paged_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                    torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                    torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                                    c10::optional<torch::Tensor> v_scale, torch::Tensor tree_mask, int64_t chunk,
                                                    torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_impl("block_attention_tree_decode_paged_fp8", "k_pages", "v_pages", true, offsets, columns, nnz, q,
                                     k_pages, v_pages, &block_table, k_lens, scale, k_scale, v_scale, chunk, out, lse, &tree_mask);
}

// … with a window (DESIGN.md §3.35): the four plain bindings with `window, sink` (ints, 1 ≤ window, 0 ≤ sink, both int32) before chunk
torch::Tensor block_attention_window_decode(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                            torch::Tensor v, torch::Tensor k_lens, double scale, int64_t window, int64_t sink,
                                            int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_impl("block_attention_window_decode", "k", "v", false, offsets, columns, nnz, q, k, v, nullptr, k_lens,
                                     scale, c10::nullopt, c10::nullopt, chunk, out, lse, nullptr, &win);
}

torch::Tensor block_attention_window_decode_paged(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                  torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                  torch::Tensor k_lens, double scale, int64_t window, int64_t sink, int64_t chunk,
                                                  torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_impl("block_attention_window_decode_paged", "k_pages", "v_pages", false, offsets, columns, nnz, q,
                                     k_pages, v_pages, &block_table, k_lens, scale, c10::nullopt, c10::nullopt, chunk, out, lse, nullptr,
                                     &win);
}

torch::Tensor block_attention_window_decode_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                torch::Tensor k, torch::Tensor v, torch::Tensor k_lens, double scale,
                                                c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                int64_t window, int64_t sink, int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_impl("block_attention_window_decode_fp8", "k", "v", true, offsets, columns, nnz, q, k, v, nullptr,
                                     k_lens, scale, k_scale, v_scale, chunk, out, lse, nullptr, &win);
}

torch::Tensor block_attention_window_decode_paged_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                      torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                      torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                                      c10::optional<torch::Tensor> v_scale, int64_t window, int64_t sink,
                                                      int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_impl("block_attention_window_decode_paged_fp8", "k_pages", "v_pages", true, offsets, columns, nnz, q,
                                     k_pages, v_pages, &block_table, k_lens, scale, k_scale, v_scale, chunk, out, lse, nullptr, &win);
}
