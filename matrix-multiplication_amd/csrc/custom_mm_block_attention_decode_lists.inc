// custom_mm — block-sparse attention for decoding over the caller's block lists: block_attention_decode{,_paged} with the list
// of every (k / v item, token) given as a row of block_ids, in the place of a CSR layout (DESIGN.md §3.29)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after
// custom_mm_kv_cache.inc, whose reading-call pieces it shares with the decode and the prefill bindings (§3.31).  Not compiled on
// its own.  Contract: include/mi_spmm.h, "Query-aware key-block selection": block_ids int32 [B, Hkv, T, K] and block_counts int32 [B, Hkv, T], contiguous, HANDED OVER AS THEY ARE; q and out
// [B, Hq, T, D] contiguous, bfloat16 or float16; the cache of q's type or (the *_fp8 forms, §3.32) float8_e4m3fn with the two
// scales, read through its own strides; lse float32 [B, Hq, T].

// all four forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D]; `fp8`: a
// cache of e4m3fn bytes with the two scales.  Its own:
// chunk, Smax % 64, the block_ids / block_counts rules, the workspace of a cache of K blocks, the C entry.
torch::Tensor block_attention_decode_lists_impl(const char* what, const char* kname, const char* vname, bool fp8,
                                                const torch::Tensor& block_ids, const torch::Tensor& block_counts, const torch::Tensor& q,
                                                const torch::Tensor& k, const torch::Tensor& v, const torch::Tensor* table,
                                                const torch::Tensor& k_lens, double scale, const c10::optional<torch::Tensor>& k_scale,
                                                const c10::optional<torch::Tensor>& v_scale, int64_t chunk, torch::Tensor out,
                                                const torch::Tensor& lse, const torch::Tensor* tree = nullptr,
                                                const WindowOperand* win = nullptr) {
  TORCH_CHECK(!(tree && win), what, ": a tree mask and a window do not go together");
  if (win) check_window(what, *win);
  const ReadShape s = read_shape(what, kname, vname, fp8, q, k, v, table, out);
  TORCH_CHECK(chunk >= 1 && chunk <= INT32_MAX, what, ": chunk must be a positive int32, got ", chunk);
  const int64_t Smax = read_smax(what, k, table, s.B);
  TORCH_CHECK(Smax % 64 == 0, what, ": Smax = ", Smax, " must be a multiple of 64");
  TORCH_CHECK(block_ids.dim() == 4 && block_ids.size(0) == s.B && block_ids.size(1) == s.Hkv && block_ids.size(2) == s.T &&
                  block_ids.size(3) >= 1 && block_ids.is_contiguous(),
              what, ": block_ids must be a contiguous [B, Hkv, T, K] = [", s.B, ", ", s.Hkv, ", ", s.T, ", K >= 1] tensor");
  const int64_t K = block_ids.size(3);
  TORCH_CHECK(block_counts.dim() == 3 && block_counts.size(0) == s.B && block_counts.size(1) == s.Hkv && block_counts.size(2) == s.T &&
                  block_counts.is_contiguous(),
              what, ": block_counts must be a contiguous [B, Hkv, T] = [", s.B, ", ", s.Hkv, ", ", s.T, "] tensor");
  check_device_i32(block_ids, "block_ids");
  check_device_i32(block_counts, "block_counts");
  check_same_device(what, q.device(), {&block_ids, &block_counts, &k, &v});
  check_read_operands(what, q.device(), true, q, table, k_lens, out, lse, s);
  const ReadCache r = read_cache(what, kname, vname, fp8, q, k, v, table, k_scale, v_scale, s);
  check_sizes(what, {64 * K, s.B * s.Hkv * s.T * K});
  std::pair<const int64_t*, int32_t> tm = {nullptr, 0};
  if (tree) tm = tree_mask_operand(what, *tree, s.B, s.T, q.device());
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  // a list has at most K entries: the chunks' partials are those of a cache of K blocks
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)(s.B * s.Hkv), (int32_t)s.T, (int32_t)s.group, (int32_t)s.D,
                                                                    (int32_t)(64 * K), (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
#define MI_LISTS_HEAD block_ids.data_ptr<int32_t>(), block_counts.data_ptr<int32_t>(), (int32_t)K, MI_READ_SIZES
#define MI_LISTS_OPERANDS(CT) (int32_t) s.D, bits16(q), s.D, s.T* s.D, MI_READ_CACHE(CT), (int32_t)s.group, (int32_t)chunk, (float)scale
#define MI_LISTS_OUT MI_READ_OUT, ws.data_ptr(), ws_bytes, stream_of(out)
#define MI_LISTS_TREE tm.first, tm.second
#define MI_LISTS_WINDOW (int32_t) win->window, (int32_t)win->sink
  int st;
  if (win && fp8)
    st = table ? (s.bf ? mi_block_attention_window_decode_lists_paged_fp8_bf16 : mi_block_attention_window_decode_lists_paged_fp8_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_WINDOW, MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_window_decode_lists_fp8_bf16 : mi_block_attention_window_decode_lists_fp8_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_WINDOW, MI_LISTS_OUT);
  else if (win)
    st = table ? (s.bf ? mi_block_attention_window_decode_lists_paged_bf16 : mi_block_attention_window_decode_lists_paged_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_WINDOW, MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_window_decode_lists_bf16 : mi_block_attention_window_decode_lists_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_WINDOW, MI_LISTS_OUT);
  else if (tree && fp8)
    st = table ? (s.bf ? mi_block_attention_tree_decode_lists_paged_fp8_bf16 : mi_block_attention_tree_decode_lists_paged_fp8_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_TREE, MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_tree_decode_lists_fp8_bf16 : mi_block_attention_tree_decode_lists_fp8_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_TREE, MI_LISTS_OUT);
  else if (tree)
    st = table ? (s.bf ? mi_block_attention_tree_decode_lists_paged_bf16 : mi_block_attention_tree_decode_lists_paged_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_TREE, MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_tree_decode_lists_bf16 : mi_block_attention_tree_decode_lists_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_TREE, MI_LISTS_OUT);
  else if (fp8)
    st = table ? (s.bf ? mi_block_attention_lists_decode_paged_fp8_bf16 : mi_block_attention_lists_decode_paged_fp8_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_lists_decode_fp8_bf16 : mi_block_attention_lists_decode_fp8_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_OUT);
  else
    st = table ? (s.bf ? mi_block_attention_decode_lists_paged_bf16 : mi_block_attention_decode_lists_paged_f16)(
                             MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_decode_lists_bf16 : mi_block_attention_decode_lists_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_OUT);
#undef MI_LISTS_HEAD
#undef MI_LISTS_OPERANDS
#undef MI_LISTS_OUT
#undef MI_LISTS_TREE
#undef MI_LISTS_WINDOW
  check_status(st, what);
  return out;
}

torch::Tensor block_attention_decode_lists(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                           torch::Tensor v, torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out,
                                           torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_decode_lists", "k", "v", false, block_ids, block_counts, q, k, v, nullptr,
                                           k_lens, scale, c10::nullopt, c10::nullopt, chunk, out, lse);
}

torch::Tensor block_attention_decode_lists_paged(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                 torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                 torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out,
                                                 torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_decode_lists_paged", "k_pages", "v_pages", false, block_ids, block_counts, q,
                                           k_pages, v_pages, &block_table, k_lens, scale, c10::nullopt, c10::nullopt, chunk, out, lse);
}

torch::Tensor block_attention_lists_decode_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                               torch::Tensor v, torch::Tensor k_lens, double scale,
                                               c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale, int64_t chunk,
                                               torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_lists_decode_fp8", "k", "v", true, block_ids, block_counts, q, k, v, nullptr,
                                           k_lens, scale, k_scale, v_scale, chunk, out, lse);
}

torch::Tensor block_attention_lists_decode_paged_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                     torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                     torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                                     c10::optional<torch::Tensor> v_scale, int64_t chunk, torch::Tensor out,
                                                     torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_lists_decode_paged_fp8", "k_pages", "v_pages", true, block_ids, block_counts,
                                           q, k_pages, v_pages, &block_table, k_lens, scale, k_scale, v_scale, chunk, out, lse);
}

// … with a tree mask (DESIGN.md §3.34): the four bindings above with `tree_mask` int64 [B, T] or [T] before chunk
torch::Tensor block_attention_tree_decode_lists(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                                torch::Tensor v, torch::Tensor k_lens, double scale, torch::Tensor tree_mask,
                                                int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_tree_decode_lists", "k", "v", false, block_ids, block_counts, q, k, v,
                                           nullptr, k_lens, scale, c10::nullopt, c10::nullopt, chunk, out, lse, &tree_mask);
}

torch::Tensor block_attention_tree_decode_lists_paged(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                      torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                      torch::Tensor k_lens, double scale, torch::Tensor tree_mask, int64_t chunk,
                                                      torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_tree_decode_lists_paged", "k_pages", "v_pages", false, block_ids,
                                           block_counts, q, k_pages, v_pages, &block_table, k_lens, scale, c10::nullopt, c10::nullopt,
                                           chunk, out, lse, &tree_mask);
}

torch::Tensor block_attention_tree_lists_decode_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                                    torch::Tensor v, torch::Tensor k_lens, double scale,
                                                    c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                    torch::Tensor tree_mask, int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_tree_lists_decode_fp8", "k", "v", true, block_ids, block_counts, q, k, v,
                                           nullptr, k_lens, scale, k_scale, v_scale, chunk, out, lse, &tree_mask);
}

torch::Tensor block_attention_tree_lists_decode_paged_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                          torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                          torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                                          c10::optional<torch::Tensor> v_scale, torch::Tensor tree_mask, int64_t chunk,
                                                          torch::Tensor out, torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_tree_lists_decode_paged_fp8", "k_pages", "v_pages", true, block_ids,
                                           block_counts, q, k_pages, v_pages, &block_table, k_lens, scale, k_scale, v_scale, chunk, out,
                                           lse, &tree_mask);
}

// … with a window (DESIGN.md §3.35): the four plain bindings with `window, sink` before chunk
torch::Tensor block_attention_window_decode_lists(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                                  torch::Tensor v, torch::Tensor k_lens, double scale, int64_t window, int64_t sink,
                                                  int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_lists_impl("block_attention_window_decode_lists", "k", "v", false, block_ids, block_counts, q, k, v,
                                           nullptr, k_lens, scale, c10::nullopt, c10::nullopt, chunk, out, lse, nullptr, &win);
}

torch::Tensor block_attention_window_decode_lists_paged(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                        torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                        torch::Tensor k_lens, double scale, int64_t window, int64_t sink, int64_t chunk,
                                                        torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_lists_impl("block_attention_window_decode_lists_paged", "k_pages", "v_pages", false, block_ids,
                                           block_counts, q, k_pages, v_pages, &block_table, k_lens, scale, c10::nullopt, c10::nullopt,
                                           chunk, out, lse, nullptr, &win);
}

torch::Tensor block_attention_window_lists_decode_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                      torch::Tensor k, torch::Tensor v, torch::Tensor k_lens, double scale,
                                                      c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                      int64_t window, int64_t sink, int64_t chunk, torch::Tensor out,
                                                      torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_lists_impl("block_attention_window_lists_decode_fp8", "k", "v", true, block_ids, block_counts, q, k, v,
                                           nullptr, k_lens, scale, k_scale, v_scale, chunk, out, lse, nullptr, &win);
}

torch::Tensor block_attention_window_lists_decode_paged_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                            torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                            torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                                            c10::optional<torch::Tensor> v_scale, int64_t window, int64_t sink,
                                                            int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_decode_lists_impl("block_attention_window_lists_decode_paged_fp8", "k_pages", "v_pages", true, block_ids,
                                           block_counts, q, k_pages, v_pages, &block_table, k_lens, scale, k_scale, v_scale, chunk, out,
                                           lse, nullptr, &win);
}
