// custom_mm — block-sparse prefill attention over the KV cache: the T newest tokens of every item (a whole prompt or a chunk of
// it) against a key / value cache, in its four forms — contiguous or paged, 2-byte or FP8 (OCP e4m3fn)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands (DESIGN.md §3.23) and about a reading call (§3.31): this file keeps what is the
// prefill calls' own.  Not compiled on its own.  Contract: include/mi_spmm.h, "Block-sparse prefill attention over the
// KV cache" (DESIGN.md §3.27): q [B, Hq, T, D] bfloat16 or float16 READ THROUGH ITS OWN STRIDES (check_source_strides: never
// copied), out [B, Hq, T, D] contiguous; the cache of q's type or float8_e4m3fn; offsets int32 [layouts, Smax/64 + 1] with the
// layouts' bases, columns int32 layout-local, in 64-blocks; new_lens None or int32 [B] / [1]; lse float32 [B, Hq, T].  No
// workspace — but for the four …_split bindings (DESIGN.md §3.28), which take `split` after the old argument list and get the
// workspace of the parts' partials from torch's allocator.

// all four forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D];
// `fp8`: a cache of e4m3fn bytes with the two scales; `split` 0: the unsplit entries, else the list entries of a part.  Its
// own: the layout, new_lens, q through its own strides, the split workspace, the C entry.
torch::Tensor block_attention_prefill_impl(const char* what, const char* kname, const char* vname, bool fp8, const torch::Tensor& offsets,
                                           const torch::Tensor& columns, int64_t nnz, const torch::Tensor& q, const torch::Tensor& k,
                                           const torch::Tensor& v, const torch::Tensor* table, const torch::Tensor& k_lens,
                                           const c10::optional<torch::Tensor>& new_lens, double scale,
                                           const c10::optional<torch::Tensor>& k_scale, const c10::optional<torch::Tensor>& v_scale,
                                           torch::Tensor out, const torch::Tensor& lse, int64_t split = 0,
                                           const WindowOperand* win = nullptr) {
  TORCH_CHECK(!(split != 0 && win), what, ": split and a window do not go together");
  if (win) check_window(what, *win);
  const ReadShape s = read_shape(what, kname, vname, fp8, q, k, v, table, out);
  const int64_t Smax = read_smax(what, k, table, s.B);
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Smax, Smax);
  check_same_device(what, lay.list.device, {&q, &k, &v});
  check_read_operands(what, lay.list.device, false, q, table, k_lens, out, lse, s);
  const int32_t* nl = nullptr;
  int32_t nl_count = 0;
  if (new_lens.has_value()) {
    check_same_device(what, lay.list.device, {&*new_lens});
    check_device_i32(*new_lens, "new_lens");
    TORCH_CHECK(new_lens->is_contiguous() && (new_lens->numel() == s.B || new_lens->numel() == 1), what,
                ": new_lens must be None or a contiguous int32 tensor of B = ", s.B, " entries or of one, got ", new_lens->numel());
    nl = new_lens->data_ptr<int32_t>(), nl_count = (int32_t)new_lens->numel();
  }
  check_source_strides(what, "q", q);
  const ReadCache r = read_cache(what, kname, vname, fp8, q, k, v, table, k_scale, v_scale, s);
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  torch::Tensor ws;  // the partials of a split call: alive until the launches are enqueued, then the allocator's on this stream
  int64_t ws_bytes = 0;
  if (split != 0) {
    ws_bytes = mi_block_attention_prefill_split_workspace_bytes((int32_t)(s.B * s.Hkv), (int32_t)s.group, (int32_t)s.T, (int32_t)s.D,
                                                                (int32_t)Smax, (int32_t)split);
    if (ws_bytes < 0) check_status((int)ws_bytes, what);
    ws = byte_workspace(out.device(), (size_t)ws_bytes, 16);
  }
// the argument lists of the sixteen C entries, in pieces: MI_READ_TABLE and MI_READ_SCALES are what the paged and the fp8 entries add
#define MI_PREFILL_LIST lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, MI_READ_SIZES
#define MI_PREFILL_OPERANDS(CT)                                                                                            \
  (int32_t) s.D, bits16(q), cache_stride(q, 2, s.D), cache_stride(q, 1, 0), cache_stride(q, 0, 0), MI_READ_CACHE(CT), nl, nl_count, \
      (int32_t)s.group, (float)scale
#define MI_PREFILL_OUT MI_READ_OUT, stream_of(out)
#define MI_PREFILL_SPLIT_OUT MI_READ_OUT, (int32_t)split, ws.data_ptr(), (size_t)ws_bytes, stream_of(out)
#define MI_PREFILL_WINDOW_OUT (int32_t) win->window, (int32_t)win->sink, MI_PREFILL_OUT
  int st;
  if (win && !fp8)
    st = table ? (s.bf ? mi_block_attention_window_prefill_paged_bf16 : mi_block_attention_window_prefill_paged_f16)(
                     MI_PREFILL_LIST, MI_READ_TABLE, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_WINDOW_OUT)
               : (s.bf ? mi_block_attention_window_prefill_bf16 : mi_block_attention_window_prefill_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_WINDOW_OUT);
  else if (win)
    st = table ? (s.bf ? mi_block_attention_window_prefill_paged_fp8_bf16 : mi_block_attention_window_prefill_paged_fp8_f16)(
                     MI_PREFILL_LIST, MI_READ_TABLE, MI_PREFILL_OPERANDS(uint8_t), MI_READ_SCALES, MI_PREFILL_WINDOW_OUT)
               : (s.bf ? mi_block_attention_window_prefill_fp8_bf16 : mi_block_attention_window_prefill_fp8_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint8_t), MI_READ_SCALES, MI_PREFILL_WINDOW_OUT);
  else if (split != 0 && !fp8)
    st = table ? (s.bf ? mi_block_attention_prefill_split_paged_bf16 : mi_block_attention_prefill_split_paged_f16)(
                     MI_PREFILL_LIST, MI_READ_TABLE, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_SPLIT_OUT)
               : (s.bf ? mi_block_attention_prefill_split_bf16 : mi_block_attention_prefill_split_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_SPLIT_OUT);
  else if (split != 0)
    st = table ? (s.bf ? mi_block_attention_prefill_split_paged_fp8_bf16 : mi_block_attention_prefill_split_paged_fp8_f16)(
                     MI_PREFILL_LIST, MI_READ_TABLE, MI_PREFILL_OPERANDS(uint8_t), MI_READ_SCALES, MI_PREFILL_SPLIT_OUT)
               : (s.bf ? mi_block_attention_prefill_split_fp8_bf16 : mi_block_attention_prefill_split_fp8_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint8_t), MI_READ_SCALES, MI_PREFILL_SPLIT_OUT);
  else if (!fp8)
    st = table ? (s.bf ? mi_block_attention_prefill_paged_bf16 : mi_block_attention_prefill_paged_f16)(
                     MI_PREFILL_LIST, MI_READ_TABLE, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_OUT)
               : (s.bf ? mi_block_attention_prefill_bf16 : mi_block_attention_prefill_f16)(MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint16_t),
                                                                                         MI_PREFILL_OUT);
  else
    st = table ? (s.bf ? mi_block_attention_prefill_paged_fp8_bf16 : mi_block_attention_prefill_paged_fp8_f16)(
                     MI_PREFILL_LIST, MI_READ_TABLE, MI_PREFILL_OPERANDS(uint8_t), MI_READ_SCALES, MI_PREFILL_OUT)
               : (s.bf ? mi_block_attention_prefill_fp8_bf16 : mi_block_attention_prefill_fp8_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint8_t), MI_READ_SCALES, MI_PREFILL_OUT);
#undef MI_PREFILL_LIST
#undef MI_PREFILL_OPERANDS
#undef MI_PREFILL_OUT
#undef MI_PREFILL_SPLIT_OUT
#undef MI_PREFILL_WINDOW_OUT
  check_status(st, what);
  return out;
}

torch::Tensor block_attention_prefill(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                      torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                      torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_impl("block_attention_prefill", "k", "v", false, offsets, columns, nnz, q, k, v, nullptr, k_lens,
                                      new_lens, scale, c10::nullopt, c10::nullopt, out, lse);
}

torch::Tensor block_attention_prefill_paged(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                            torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                            torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                            torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_impl("block_attention_prefill_paged", "k_pages", "v_pages", false, offsets, columns, nnz, q, k_pages,
                                      v_pages, &block_table, k_lens, new_lens, scale, c10::nullopt, c10::nullopt, out, lse);
}

torch::Tensor block_attention_prefill_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                          c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                          torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_impl("block_attention_prefill_fp8", "k", "v", true, offsets, columns, nnz, q, k, v, nullptr, k_lens,
                                      new_lens, scale, k_scale, v_scale, out, lse);
}

torch::Tensor block_attention_prefill_paged_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                                c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_impl("block_attention_prefill_paged_fp8", "k_pages", "v_pages", true, offsets, columns, nnz, q,
                                      k_pages, v_pages, &block_table, k_lens, new_lens, scale, k_scale, v_scale, out, lse);
}

// the four split forms: the old argument lists with `split` at the end
void check_split(const char* what, int64_t split) {
  TORCH_CHECK(split >= 1 && split <= INT32_MAX, what, ": split must be a positive int32, got ", split);
}

torch::Tensor block_attention_prefill_split(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                            torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                            torch::Tensor out, torch::Tensor lse, int64_t split) {
  check_split("block_attention_prefill_split", split);
  return block_attention_prefill_impl("block_attention_prefill_split", "k", "v", false, offsets, columns, nnz, q, k, v, nullptr, k_lens,
                                      new_lens, scale, c10::nullopt, c10::nullopt, out, lse, split);
}

torch::Tensor block_attention_prefill_split_paged(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                  torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                  torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                                  torch::Tensor out, torch::Tensor lse, int64_t split) {
  check_split("block_attention_prefill_split_paged", split);
  return block_attention_prefill_impl("block_attention_prefill_split_paged", "k_pages", "v_pages", false, offsets, columns, nnz, q,
                                      k_pages, v_pages, &block_table, k_lens, new_lens, scale, c10::nullopt, c10::nullopt, out, lse,
                                      split);
}

torch::Tensor block_attention_prefill_split_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                torch::Tensor k, torch::Tensor v, torch::Tensor k_lens,
                                                c10::optional<torch::Tensor> new_lens, double scale,
                                                c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                torch::Tensor out, torch::Tensor lse, int64_t split) {
  check_split("block_attention_prefill_split_fp8", split);
  return block_attention_prefill_impl("block_attention_prefill_split_fp8", "k", "v", true, offsets, columns, nnz, q, k, v, nullptr,
                                      k_lens, new_lens, scale, k_scale, v_scale, out, lse, split);
}

torch::Tensor block_attention_prefill_split_paged_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                                      torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                      torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                                      c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                      torch::Tensor out, torch::Tensor lse, int64_t split) {
  check_split("block_attention_prefill_split_paged_fp8", split);
  return block_attention_prefill_impl("block_attention_prefill_split_paged_fp8", "k_pages", "v_pages", true, offsets, columns, nnz, q,
                                      k_pages, v_pages, &block_table, k_lens, new_lens, scale, k_scale, v_scale, out, lse, split);
}

// … with a window (DESIGN.md §3.35): the four unsplit bindings with `window, sink` (ints, 1 ≤ window, 0 ≤ sink, both int32) before out
torch::Tensor block_attention_window_prefill(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale, int64_t window, int64_t sink,
    torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_impl("block_attention_window_prefill", "k", "v", false, offsets, columns, nnz, q, k, v, nullptr, k_lens,
      new_lens, scale, c10::nullopt, c10::nullopt, out, lse, 0, &win);
}

torch::Tensor block_attention_window_prefill_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
    torch::Tensor k, torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
    c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale, int64_t window, int64_t sink,
    torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_impl("block_attention_window_prefill_fp8", "k", "v", true, offsets, columns, nnz, q, k, v, nullptr,
      k_lens, new_lens, scale, k_scale, v_scale, out, lse, 0, &win);
}

torch::Tensor block_attention_window_prefill_paged(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
    torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens,
    double scale, int64_t window, int64_t sink, torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_impl("block_attention_window_prefill_paged", "k_pages", "v_pages", false, offsets, columns, nnz, q,
      k_pages, v_pages, &block_table, k_lens, new_lens, scale, c10::nullopt, c10::nullopt, out, lse, 0, &win);
}

torch::Tensor block_attention_window_prefill_paged_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
    torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens,
    double scale, c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale, int64_t window, int64_t sink,
    torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_impl("block_attention_window_prefill_paged_fp8", "k_pages", "v_pages", true, offsets, columns, nnz, q,
      k_pages, v_pages, &block_table, k_lens, new_lens, scale, k_scale, v_scale, out, lse, 0, &win);
}
