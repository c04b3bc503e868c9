// custom_mm — block-sparse attention for decoding over the caller's block lists: block_attention_decode{,_paged} with the list
// of every (k / v item, token) given as a row of block_ids, in the place of a CSR layout (DESIGN.md §3.29)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after
// custom_mm_block_attention_decode.inc.  Not compiled on its own.  Contract: include/mi_spmm.h, "Query-aware key-block
// selection": block_ids int32 [B, Hkv, T, K] and block_counts int32 [B, Hkv, T], contiguous, HANDED OVER AS THEY ARE; q and out
// [B, Hq, T, D] contiguous, bfloat16 or float16; the cache of q's type, read through its own strides; lse float32 [B, Hq, T].

// both forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D]
torch::Tensor block_attention_decode_lists_impl(const char* what, const char* kname, const char* vname, const torch::Tensor& block_ids,
                                                const torch::Tensor& block_counts, const torch::Tensor& q, const torch::Tensor& k,
                                                const torch::Tensor& v, const torch::Tensor* table, const torch::Tensor& k_lens,
                                                double scale, int64_t chunk, torch::Tensor out, const torch::Tensor& lse) {
  const bool bf = is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {kname, &k}, {vname, &v}, {"out", &out}}, true));
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
  TORCH_CHECK(Smax % 64 == 0, what, ": Smax = ", Smax, " must be a multiple of 64");
  TORCH_CHECK(block_ids.dim() == 4 && block_ids.size(0) == B && block_ids.size(1) == Hkv && block_ids.size(2) == T &&
                  block_ids.size(3) >= 1 && block_ids.is_contiguous(),
              what, ": block_ids must be a contiguous [B, Hkv, T, K] = [", B, ", ", Hkv, ", ", T, ", K >= 1] tensor");
  const int64_t K = block_ids.size(3);
  TORCH_CHECK(block_counts.dim() == 3 && block_counts.size(0) == B && block_counts.size(1) == Hkv && block_counts.size(2) == T &&
                  block_counts.is_contiguous(),
              what, ": block_counts must be a contiguous [B, Hkv, T] = [", B, ", ", Hkv, ", ", T, "] tensor");
  check_device_i32(block_ids, "block_ids");
  check_device_i32(block_counts, "block_counts");
  check_same_device(what, q.device(), {&block_ids, &block_counts, &k, &v});
  if (table) check_same_device(what, q.device(), {table});
  check_same_device(what, q.device(), {&out, &lse, &k_lens});
  check_device_f32(lse, "lse");
  check_device_i32(k_lens, "k_lens");
  if (table) check_table(what, *table);
  TORCH_CHECK(q.is_contiguous() && out.is_contiguous() && out.sizes() == q.sizes(), what,
              ": q and out must be contiguous [B, Hq, T, D] tensors of one shape");
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == B * Hq * T, what, ": lse must be a contiguous [B, Hq, T] tensor");
  check_k_lens(what, k_lens, B);
  const char* outer = table ? "page" : "batch";
  check_cache_strides(what, kname, k, D, outer);
  check_cache_strides(what, vname, v, D, outer);
  const CacheOperands c = cache_operands(k, v, table, D);
  check_sizes(what, {B * Hkv, B * Hq, T, Smax, D, c.P, 64 * K, B * Hkv * T * K});
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  const int64_t items = B * Hkv;
  // a list has at most K entries: the chunks' partials are those of a cache of K blocks
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)items, (int32_t)T, (int32_t)group, (int32_t)D,
                                                                    (int32_t)(64 * K), (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
#define MI_LISTS_HEAD block_ids.data_ptr<int32_t>(), block_counts.data_ptr<int32_t>(), (int32_t)K, (int32_t)items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax
#define MI_LISTS_OPERANDS                                                                                                        \
  (int32_t) D, p(q), D, T* D, static_cast<const uint16_t*>(c.k), c.ldk, c.headK, c.outerK, static_cast<const uint16_t*>(c.v), c.ldv,   \
      c.headV, c.outerV, k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel(), (int32_t)group, (int32_t)chunk, (float)scale, p(out), D, \
      T* D, lse.data_ptr<float>(), ws.data_ptr(), ws_bytes, stream_of(out)
  const int st = table ? (bf ? mi_block_attention_decode_lists_paged_bf16 : mi_block_attention_decode_lists_paged_f16)(
                             MI_LISTS_HEAD, c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page, MI_LISTS_OPERANDS)
                       : (bf ? mi_block_attention_decode_lists_bf16 : mi_block_attention_decode_lists_f16)(MI_LISTS_HEAD, MI_LISTS_OPERANDS);
#undef MI_LISTS_HEAD
#undef MI_LISTS_OPERANDS
  check_status(st, what);
  return out;
}

torch::Tensor block_attention_decode_lists(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q, torch::Tensor k,
                                           torch::Tensor v, torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out,
                                           torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_decode_lists", "k", "v", block_ids, block_counts, q, k, v, nullptr, k_lens,
                                           scale, chunk, out, lse);
}

torch::Tensor block_attention_decode_lists_paged(torch::Tensor block_ids, torch::Tensor block_counts, torch::Tensor q,
                                                 torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                                 torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out,
                                                 torch::Tensor lse) {
  return block_attention_decode_lists_impl("block_attention_decode_lists_paged", "k_pages", "v_pages", block_ids, block_counts, q,
                                           k_pages, v_pages, &block_table, k_lens, scale, chunk, out, lse);
}
