// custom_mm — block-sparse prefill attention over the caller's block lists: block_attention_prefill{,_paged}{,_fp8} with the list
// of every (k / v item, position tile) given as a row of block_ids, in the place of a CSR layout (DESIGN.md §3.33)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after
// custom_mm_kv_cache.inc, whose reading-call pieces it shares with the decode and the prefill bindings (§3.31).  Not compiled on
// its own.  Contract: include/mi_spmm.h, "Prefill over the caller's lists": block_ids int32 [B, Hkv, X, K] and block_counts int32
// [B, Hkv, X] with X = ⌈T / 64⌉ + 1, contiguous, HANDED OVER AS THEY ARE; q [B, Hq, T, D] bfloat16 or float16 READ THROUGH ITS OWN
// STRIDES, out [B, Hq, T, D] contiguous; the cache of q's type or float8_e4m3fn with the two scales; new_lens None or int32 [B] /
// [1]; lse float32 [B, Hq, T].  No workspace.
// The four bindings are named block_attention_lists_prefill[_paged][_fp8] — `lists` before `prefill`, as §3.32 names its
// decode bindings: the bindings `block_attention_prefill…` are the closed family of eight layout bindings.

// all four forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D]; `fp8`: a
// cache of e4m3fn bytes with the two scales.  Its own: Smax % 64, the block_ids / block_counts rules, new_lens, q through its own
// strides, the C entry.
torch::Tensor block_attention_prefill_lists_impl(const char* what, const char* kname, const char* vname, bool fp8,
                                                 const torch::Tensor& block_ids, const torch::Tensor& block_counts, const torch::Tensor& q,
                                                 const torch::Tensor& k, const torch::Tensor& v, const torch::Tensor* table,
                                                 const torch::Tensor& k_lens, const c10::optional<torch::Tensor>& new_lens, double scale,
                                                 const c10::optional<torch::Tensor>& k_scale, const c10::optional<torch::Tensor>& v_scale,
                                                 torch::Tensor out, const torch::Tensor& lse, const WindowOperand* win = nullptr) {
  if (win) check_window(what, *win);
  const ReadShape s = read_shape(what, kname, vname, fp8, q, k, v, table, out);
  const int64_t Smax = read_smax(what, k, table, s.B);
  TORCH_CHECK(Smax % 64 == 0, what, ": Smax = ", Smax, " must be a multiple of 64");
  const int64_t X = (s.T + 63) / 64 + 1;  // position tiles per item, from the shape alone
  TORCH_CHECK(block_ids.dim() == 4 && block_ids.size(0) == s.B && block_ids.size(1) == s.Hkv && block_ids.size(2) == X &&
                  block_ids.size(3) >= 1 && block_ids.is_contiguous(),
              what, ": block_ids must be a contiguous [B, Hkv, ceil(T/64) + 1, K] = [", s.B, ", ", s.Hkv, ", ", X, ", K >= 1] tensor");
  const int64_t K = block_ids.size(3);
  TORCH_CHECK(block_counts.dim() == 3 && block_counts.size(0) == s.B && block_counts.size(1) == s.Hkv && block_counts.size(2) == X &&
                  block_counts.is_contiguous(),
              what, ": block_counts must be a contiguous [B, Hkv, ceil(T/64) + 1] = [", s.B, ", ", s.Hkv, ", ", X, "] tensor");
  check_device_i32(block_ids, "block_ids");
  check_device_i32(block_counts, "block_counts");
  check_same_device(what, q.device(), {&block_ids, &block_counts, &k, &v});
  check_read_operands(what, q.device(), false, q, table, k_lens, out, lse, s);
  const int32_t* nl = nullptr;
  int32_t nl_count = 0;
  if (new_lens.has_value()) {
    check_same_device(what, q.device(), {&*new_lens});
    check_device_i32(*new_lens, "new_lens");
    TORCH_CHECK(new_lens->is_contiguous() && (new_lens->numel() == s.B || new_lens->numel() == 1), what,
                ": new_lens must be None or a contiguous int32 tensor of B = ", s.B, " entries or of one, got ", new_lens->numel());
    nl = new_lens->data_ptr<int32_t>(), nl_count = (int32_t)new_lens->numel();
  }
  check_source_strides(what, "q", q);
  const ReadCache r = read_cache(what, kname, vname, fp8, q, k, v, table, k_scale, v_scale, s);
  check_sizes(what, {K, s.B * s.Hkv * X * K});
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
#define MI_LISTS_HEAD block_ids.data_ptr<int32_t>(), block_counts.data_ptr<int32_t>(), (int32_t)K, MI_READ_SIZES
#define MI_LISTS_OPERANDS(CT)                                                                                              \
  (int32_t) s.D, bits16(q), cache_stride(q, 2, s.D), cache_stride(q, 1, 0), cache_stride(q, 0, 0), MI_READ_CACHE(CT), nl, nl_count, \
      (int32_t)s.group, (float)scale
#define MI_LISTS_OUT MI_READ_OUT, stream_of(out)
#define MI_LISTS_WINDOW_OUT (int32_t) win->window, (int32_t)win->sink, MI_LISTS_OUT
  int st;
  if (win && fp8)
    st = table ? (s.bf ? mi_block_attention_window_prefill_lists_paged_fp8_bf16 : mi_block_attention_window_prefill_lists_paged_fp8_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_WINDOW_OUT)
               : (s.bf ? mi_block_attention_window_prefill_lists_fp8_bf16 : mi_block_attention_window_prefill_lists_fp8_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_WINDOW_OUT);
  else if (win)
    st = table ? (s.bf ? mi_block_attention_window_prefill_lists_paged_bf16 : mi_block_attention_window_prefill_lists_paged_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_WINDOW_OUT)
               : (s.bf ? mi_block_attention_window_prefill_lists_bf16 : mi_block_attention_window_prefill_lists_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_WINDOW_OUT);
  else if (fp8)
    st = table ? (s.bf ? mi_block_attention_lists_prefill_paged_fp8_bf16 : mi_block_attention_lists_prefill_paged_fp8_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_lists_prefill_fp8_bf16 : mi_block_attention_lists_prefill_fp8_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint8_t), MI_READ_SCALES, MI_LISTS_OUT);
  else
    st = table ? (s.bf ? mi_block_attention_lists_prefill_paged_bf16 : mi_block_attention_lists_prefill_paged_f16)(
                     MI_LISTS_HEAD, MI_READ_TABLE, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_OUT)
               : (s.bf ? mi_block_attention_lists_prefill_bf16 : mi_block_attention_lists_prefill_f16)(
                     MI_LISTS_HEAD, MI_LISTS_OPERANDS(uint16_t), MI_LISTS_OUT);
#undef MI_LISTS_HEAD
#undef MI_LISTS_OPERANDS
#undef MI_LISTS_OUT
#undef MI_LISTS_WINDOW_OUT
  check_status(st, what);
  return out;
}

torch::Tensor block_attention_prefill_lists(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                            torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                            torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_lists_impl("block_attention_lists_prefill", "k", "v", false, block_ids, block_counts, q, k, v, nullptr,
                                            k_lens, new_lens, scale, c10::nullopt, c10::nullopt, out, lse);
}

torch::Tensor block_attention_prefill_lists_paged(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                  torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                  torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                                  torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_lists_impl("block_attention_lists_prefill_paged", "k_pages", "v_pages", false, block_ids, block_counts,
                                            q, k_pages, v_pages, &block_table, k_lens, new_lens, scale, c10::nullopt, c10::nullopt, out,
                                            lse);
}

torch::Tensor block_attention_prefill_lists_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                                torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                                c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_lists_impl("block_attention_lists_prefill_fp8", "k", "v", true, block_ids, block_counts, q, k, v,
                                            nullptr, k_lens, new_lens, scale, k_scale, v_scale, out, lse);
}

torch::Tensor block_attention_prefill_lists_paged_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                      torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                      torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
                                                      c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale,
                                                      torch::Tensor out, torch::Tensor lse) {
  return block_attention_prefill_lists_impl("block_attention_lists_prefill_paged_fp8", "k_pages", "v_pages", true, block_ids,
                                            block_counts, q, k_pages, v_pages, &block_table, k_lens, new_lens, scale, k_scale, v_scale,
                                            out, lse);
}

// … with a window (DESIGN.md §3.35): the four bindings with `window, sink` before out, named block_attention_window_lists_prefill…
torch::Tensor block_attention_window_prefill_lists(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale, int64_t window, int64_t sink,
    torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_lists_impl("block_attention_window_lists_prefill", "k", "v", false, block_ids, block_counts, q, k, v,
      nullptr, k_lens, new_lens, scale, c10::nullopt, c10::nullopt, out, lse, &win);
}

torch::Tensor block_attention_window_prefill_lists_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
    torch::Tensor k, torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens, double scale,
    c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale, int64_t window, int64_t sink,
    torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_lists_impl("block_attention_window_lists_prefill_fp8", "k", "v", true, block_ids, block_counts, q, k, v,
      nullptr, k_lens, new_lens, scale, k_scale, v_scale, out, lse, &win);
}

torch::Tensor block_attention_window_prefill_lists_paged(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
    torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens,
    double scale, int64_t window, int64_t sink, torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_lists_impl("block_attention_window_lists_prefill_paged", "k_pages", "v_pages", false, block_ids,
      block_counts, q, k_pages, v_pages, &block_table, k_lens, new_lens, scale, c10::nullopt, c10::nullopt, out, lse, &win);
}

torch::Tensor block_attention_window_prefill_lists_paged_fp8(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
    torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens,
    double scale, c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale, int64_t window, int64_t sink,
    torch::Tensor out, torch::Tensor lse) {
  const WindowOperand win = {window, sink};
  return block_attention_prefill_lists_impl("block_attention_window_lists_prefill_paged_fp8", "k_pages", "v_pages", true, block_ids,
      block_counts, q, k_pages, v_pages, &block_table, k_lens, new_lens, scale, k_scale, v_scale, out, lse, &win);
}
