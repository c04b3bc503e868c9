// custom_mm — block-sparse attention for decoding: the newest tokens of every item against a key / value cache, in its four
// forms — contiguous or paged, 2-byte or FP8 (OCP e4m3fn)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands (DESIGN.md §3.23).  Not compiled on its own.  Contract: include/mi_spmm.h,
// "Block-sparse attention for decoding", "… over a paged cache", "… over an FP8 cache" (DESIGN.md §3.18–§3.20): q and out
// [B, Hq, T, D] contiguous, bfloat16 or float16; the cache of q's type or float8_e4m3fn; offsets int32 [layouts, Smax/64 + 1]
// with the layouts' bases, columns int32 layout-local, in 64-blocks; lse float32 [B, Hq, T].  The workspace of the chunks'
// partials comes from torch's allocator.

// q's and out's type of an fp8 call, the cache's checked on the way
bool fp8_decode_dtypes(const char* what, const torch::Tensor& q, const torch::Tensor& out, const char* kname, const torch::Tensor& k,
                       const char* vname, const torch::Tensor& v) {
  TORCH_CHECK(k.scalar_type() == torch::kFloat8_e4m3fn && v.scalar_type() == torch::kFloat8_e4m3fn, what, ": ", kname, " and ", vname,
              " must be float8_e4m3fn (the OCP e4m3fn encoding is what is read), got ", k.scalar_type(), " and ", v.scalar_type());
  return is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {"out", &out}}, true));
}

// all four forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D];
// `fp8`: a cache of e4m3fn bytes with the two scales
torch::Tensor block_attention_decode_impl(const char* what, const char* kname, const char* vname, bool fp8, const torch::Tensor& offsets,
                                          const torch::Tensor& columns, int64_t nnz, const torch::Tensor& q, const torch::Tensor& k,
                                          const torch::Tensor& v, const torch::Tensor* table, const torch::Tensor& k_lens, double scale,
                                          const c10::optional<torch::Tensor>& k_scale, const c10::optional<torch::Tensor>& v_scale,
                                          int64_t chunk, torch::Tensor out, const torch::Tensor& lse) {
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
  TORCH_CHECK(chunk >= 1 && chunk <= INT32_MAX, what, ": chunk must be a positive int32, got ", chunk);
  const int64_t Smax = table ? table_width(what, *table, B) * k.size(2) : k.size(2);
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Smax, Smax);
  check_same_device(what, lay.list.device, {&q, &k, &v});
  if (table) check_same_device(what, lay.list.device, {table});
  check_same_device(what, lay.list.device, {&out, &lse, &k_lens});
  check_device_f32(lse, "lse");
  check_device_i32(k_lens, "k_lens");
  if (table) check_table(what, *table);
  TORCH_CHECK(q.is_contiguous() && out.is_contiguous() && out.sizes() == q.sizes(), what,
              ": q and out must be contiguous [B, Hq, T, D] tensors of one shape");
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == B * Hq * T, what, ": lse must be a contiguous [B, Hq, T] tensor");
  check_k_lens(what, k_lens, B);
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
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)items, (int32_t)T, (int32_t)group, (int32_t)D,
                                                                    (int32_t)Smax, (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
// the argument lists of the eight C entries, in pieces: [table] and [scales] are what the paged and the fp8 entries add
#define MI_DECODE_LIST \
  lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax
#define MI_DECODE_TABLE c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page
#define MI_DECODE_OPERANDS(CT)                                                                                             \
  (int32_t) D, p(q), D, T* D, static_cast<const CT*>(c.k), c.ldk, c.headK, c.outerK, static_cast<const CT*>(c.v), c.ldv, c.headV, \
      c.outerV, k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel(), (int32_t)group, (int32_t)chunk, (float)scale
#define MI_DECODE_SCALES ks.first, ks.second, vs.first, vs.second
#define MI_DECODE_OUT p(out), D, T* D, lse.data_ptr<float>(), ws.data_ptr(), ws_bytes, stream_of(out)
  int st;
  if (!fp8)
    st = table ? (bf ? mi_block_attention_decode_paged_bf16 : mi_block_attention_decode_paged_f16)(
                     MI_DECODE_LIST, MI_DECODE_TABLE, MI_DECODE_OPERANDS(uint16_t), MI_DECODE_OUT)
               : (bf ? mi_block_attention_decode_bf16 : mi_block_attention_decode_f16)(MI_DECODE_LIST, MI_DECODE_OPERANDS(uint16_t),
                                                                                     MI_DECODE_OUT);
  else
    st = table ? (bf ? mi_block_attention_decode_paged_fp8_bf16 : mi_block_attention_decode_paged_fp8_f16)(
                     MI_DECODE_LIST, MI_DECODE_TABLE, MI_DECODE_OPERANDS(uint8_t), MI_DECODE_SCALES, MI_DECODE_OUT)
               : (bf ? mi_block_attention_decode_fp8_bf16 : mi_block_attention_decode_fp8_f16)(
                     MI_DECODE_LIST, MI_DECODE_OPERANDS(uint8_t), MI_DECODE_SCALES, MI_DECODE_OUT);
#undef MI_DECODE_LIST
#undef MI_DECODE_TABLE
#undef MI_DECODE_OPERANDS
#undef MI_DECODE_SCALES
#undef MI_DECODE_OUT
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
