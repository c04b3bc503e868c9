// custom_mm — block-sparse prefill attention over the KV cache: the T newest tokens of every item (a whole prompt or a chunk of
// it) against a key / value cache, in its four forms — contiguous or paged, 2-byte or FP8 (OCP e4m3fn)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands (DESIGN.md §3.23), and after custom_mm_block_attention_decode.inc, whose
// fp8_decode_dtypes it shares.  Not compiled on its own.  Contract: include/mi_spmm.h, "Block-sparse prefill attention over the
// KV cache" (DESIGN.md §3.27): q [B, Hq, T, D] bfloat16 or float16 READ THROUGH ITS OWN STRIDES (check_source_strides: never
// copied), out [B, Hq, T, D] contiguous; the cache of q's type or float8_e4m3fn; offsets int32 [layouts, Smax/64 + 1] with the
// layouts' bases, columns int32 layout-local, in 64-blocks; new_lens None or int32 [B] / [1]; lse float32 [B, Hq, T].  No
// workspace — but for the four …_split bindings (DESIGN.md §3.28), which take `split` after the old argument list and get the
// workspace of the parts' partials from torch's allocator.

// all four forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D];
// `fp8`: a cache of e4m3fn bytes with the two scales; `split` 0: the unsplit entries, else the list entries of a part
torch::Tensor block_attention_prefill_impl(const char* what, const char* kname, const char* vname, bool fp8, const torch::Tensor& offsets,
                                           const torch::Tensor& columns, int64_t nnz, const torch::Tensor& q, const torch::Tensor& k,
                                           const torch::Tensor& v, const torch::Tensor* table, const torch::Tensor& k_lens,
                                           const c10::optional<torch::Tensor>& new_lens, double scale,
                                           const c10::optional<torch::Tensor>& k_scale, const c10::optional<torch::Tensor>& v_scale,
                                           torch::Tensor out, const torch::Tensor& lse, int64_t split = 0) {
  const bool bf = fp8 ? fp8_decode_dtypes(what, q, out, kname, k, vname, v)
                      : is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {kname, &k}, {vname, &v}, {"out", &out}}, true));
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, what, ": q must be [B, Hq, T, D], ", kname, " and ", vname,
              table ? " [P, Hkv, page, D]" : " [B, Hkv, Smax, D]");
  const int64_t B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3), Hkv = k.size(1);
  if (table) {
    TORCH_CHECK(k.size(3) == D && v.sizes() == k.sizes(), what, ": ", kname, " and ", vname,
                " must be [P, Hkv, page, D] = [P, Hkv, page, ", D, "]");
    check_page(what, "keys", k.size(2));
  } else {
    TORCH_CHECK(k.size(0) == B && k.size(3) == D && v.sizes() == k.sizes(), what, ": k and v must be [B, Hkv, Smax, D] = [", B,
                ", Hkv, Smax, ", D, "]");
  }
  TORCH_CHECK(Hkv > 0 ? Hq % Hkv == 0 : Hq == 0, what, ": ", Hq, " query heads are not a multiple of ", Hkv, " k / v heads");
  const int64_t group = Hkv > 0 ? std::max<int64_t>(Hq / Hkv, 1) : 1;
  const int64_t Smax = table ? table_width(what, *table, B) * k.size(2) : k.size(2);
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Smax, Smax);
  check_same_device(what, lay.list.device, {&q, &k, &v});
  if (table) check_same_device(what, lay.list.device, {table});
  check_same_device(what, lay.list.device, {&out, &lse, &k_lens});
  check_device_f32(lse, "lse");
  check_device_i32(k_lens, "k_lens");
  if (table) check_table(what, *table);
  TORCH_CHECK(out.is_contiguous() && out.sizes() == q.sizes(), what, ": out must be a contiguous [B, Hq, T, D] tensor of q's shape");
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == B * Hq * T, what, ": lse must be a contiguous [B, Hq, T] tensor");
  check_k_lens(what, k_lens, B);
  const int32_t* nl = nullptr;
  int32_t nl_count = 0;
  if (new_lens.has_value()) {
    check_same_device(what, lay.list.device, {&*new_lens});
    check_device_i32(*new_lens, "new_lens");
    TORCH_CHECK(new_lens->is_contiguous() && (new_lens->numel() == B || new_lens->numel() == 1), what,
                ": new_lens must be None or a contiguous int32 tensor of B = ", B, " entries or of one, got ", new_lens->numel());
    nl = new_lens->data_ptr<int32_t>(), nl_count = (int32_t)new_lens->numel();
  }
  check_source_strides(what, "q", q);
  const char* outer = table ? "page" : "batch";
  check_cache_strides(what, kname, k, D, outer, fp8 ? 16 : 8);
  check_cache_strides(what, vname, v, D, outer, fp8 ? 16 : 8);
  std::pair<const float*, int32_t> ks = {nullptr, 1}, vs = ks;
  if (fp8) ks = fp8_scale(what, "k_scale", k_scale, Hkv, q), vs = fp8_scale(what, "v_scale", v_scale, Hkv, q);
  const CacheOperands c = cache_operands(k, v, table, D);
  if (table)
    check_sizes(what, {B * Hkv, B * Hq, T, Smax, D, c.P});
  else
    check_sizes(what, {B * Hkv, B * Hq, T, Smax, D});
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  const int64_t items = B * Hkv;
  torch::Tensor ws;  // the partials of a split call: alive until the launches are enqueued, then the allocator's on this stream
  int64_t ws_bytes = 0;
  if (split != 0) {
    ws_bytes = mi_block_attention_prefill_split_workspace_bytes((int32_t)items, (int32_t)group, (int32_t)T, (int32_t)D, (int32_t)Smax,
                                                                (int32_t)split);
    if (ws_bytes < 0) check_status((int)ws_bytes, what);
    ws = byte_workspace(out.device(), (size_t)ws_bytes, 16);
  }
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
// the argument lists of the eight C entries, in pieces: [table] and [scales] are what the paged and the fp8 entries add
#define MI_PREFILL_LIST \
  lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax
#define MI_PREFILL_TABLE c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page
#define MI_PREFILL_OPERANDS(CT)                                                                                               \
  (int32_t) D, p(q), cache_stride(q, 2, D), cache_stride(q, 1, 0), cache_stride(q, 0, 0), static_cast<const CT*>(c.k), c.ldk,  \
      c.headK, c.outerK, static_cast<const CT*>(c.v), c.ldv, c.headV, c.outerV, k_lens.data_ptr<int32_t>(),                   \
      (int32_t)k_lens.numel(), nl, nl_count, (int32_t)group, (float)scale
#define MI_PREFILL_SCALES ks.first, ks.second, vs.first, vs.second
#define MI_PREFILL_OUT p(out), D, T* D, lse.data_ptr<float>(), stream_of(out)
#define MI_PREFILL_SPLIT_OUT p(out), D, T* D, lse.data_ptr<float>(), (int32_t)split, ws.data_ptr(), (size_t)ws_bytes, stream_of(out)
  int st;
  if (split != 0 && !fp8)
    st = table ? (bf ? mi_block_attention_prefill_split_paged_bf16 : mi_block_attention_prefill_split_paged_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_TABLE, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_SPLIT_OUT)
               : (bf ? mi_block_attention_prefill_split_bf16 : mi_block_attention_prefill_split_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_SPLIT_OUT);
  else if (split != 0)
    st = table ? (bf ? mi_block_attention_prefill_split_paged_fp8_bf16 : mi_block_attention_prefill_split_paged_fp8_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_TABLE, MI_PREFILL_OPERANDS(uint8_t), MI_PREFILL_SCALES, MI_PREFILL_SPLIT_OUT)
               : (bf ? mi_block_attention_prefill_split_fp8_bf16 : mi_block_attention_prefill_split_fp8_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint8_t), MI_PREFILL_SCALES, MI_PREFILL_SPLIT_OUT);
  else if (!fp8)
    st = table ? (bf ? mi_block_attention_prefill_paged_bf16 : mi_block_attention_prefill_paged_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_TABLE, MI_PREFILL_OPERANDS(uint16_t), MI_PREFILL_OUT)
               : (bf ? mi_block_attention_prefill_bf16 : mi_block_attention_prefill_f16)(MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint16_t),
                                                                                       MI_PREFILL_OUT);
  else
    st = table ? (bf ? mi_block_attention_prefill_paged_fp8_bf16 : mi_block_attention_prefill_paged_fp8_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_TABLE, MI_PREFILL_OPERANDS(uint8_t), MI_PREFILL_SCALES, MI_PREFILL_OUT)
               : (bf ? mi_block_attention_prefill_fp8_bf16 : mi_block_attention_prefill_fp8_f16)(
                     MI_PREFILL_LIST, MI_PREFILL_OPERANDS(uint8_t), MI_PREFILL_SCALES, MI_PREFILL_OUT);
#undef MI_PREFILL_LIST
#undef MI_PREFILL_TABLE
#undef MI_PREFILL_OPERANDS
#undef MI_PREFILL_SCALES
#undef MI_PREFILL_OUT
#undef MI_PREFILL_SPLIT_OUT
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
