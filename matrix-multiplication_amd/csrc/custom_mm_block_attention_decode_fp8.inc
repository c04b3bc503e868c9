// custom_mm — block-sparse attention for decoding over an FP8 (OCP e4m3fn) key / value cache, contiguous and paged
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after
// custom_mm_block_attention_decode.inc, whose stride checks it shares.  Not compiled on its own.  Contract: include/mi_spmm.h,
// "… over an FP8 cache" (DESIGN.md §3.20): the operands of block_attention_decode / block_attention_decode_paged with q and
// out bfloat16 or float16 and the cache (k, v [B, Hkv, Smax, D] or k_pages, v_pages [P, Hkv, page, D]) float8_e4m3fn, READ
// THROUGH ITS OWN STRIDES (last stride 1, the others multiples of 16 elements, a 16-byte aligned data pointer — never copied);
// k_scale, v_scale: None (= 1) or float32 device tensors of 1 or Hkv entries, handed over as pointers and never read back.

// q's and out's type of an fp8 call, the cache's checked on the way
bool fp8_decode_dtypes(const char* what, const torch::Tensor& q, const torch::Tensor& out, const char* kname, const torch::Tensor& k,
                       const char* vname, const torch::Tensor& v) {
  TORCH_CHECK(k.scalar_type() == torch::kFloat8_e4m3fn && v.scalar_type() == torch::kFloat8_e4m3fn, what, ": ", kname, " and ", vname,
              " must be float8_e4m3fn (the OCP e4m3fn encoding is what is read), got ", k.scalar_type(), " and ", v.scalar_type());
  return is_lowp_dtype(what, value_dtype(what, {{"q", &q}, {"out", &out}}, true));
}

// a scale operand as the C ABI takes it: (pointer or null, count)
std::pair<const float*, int32_t> fp8_scale(const char* what, const char* name, const c10::optional<torch::Tensor>& s, int64_t Hkv,
                                           const torch::Tensor& q) {
  if (!s.has_value()) return {nullptr, 1};
  const torch::Tensor& t = *s;
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.device() == q.device() && t.is_contiguous() && t.dim() <= 1 &&
                  (t.numel() == 1 || t.numel() == Hkv),
              what, ": ", name, " must be None or a contiguous float32 tensor on q's device of 1 or Hkv = ", Hkv, " entries");
  return {t.data_ptr<float>(), (int32_t)t.numel()};
}

torch::Tensor block_attention_decode_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                         torch::Tensor v, torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                         c10::optional<torch::Tensor> v_scale, int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  const char* what = "block_attention_decode_fp8";
  const bool bf = fp8_decode_dtypes(what, q, out, "k", k, "v", v);
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, what, ": q must be [B, Hq, T, D], k and v [B, Hkv, Smax, D]");
  const int64_t B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3), Hkv = k.size(1), Smax = k.size(2);
  TORCH_CHECK(k.size(0) == B && k.size(3) == D && v.sizes() == k.sizes(), what, ": k and v must be [B, Hkv, Smax, D] = [", B,
              ", Hkv, Smax, ", D, "]");
  TORCH_CHECK(Hkv > 0 ? Hq % Hkv == 0 : Hq == 0, what, ": ", Hq, " query heads are not a multiple of ", Hkv, " k / v heads");
  const int64_t group = Hkv > 0 ? std::max<int64_t>(Hq / Hkv, 1) : 1;
  TORCH_CHECK(chunk >= 1 && chunk <= INT32_MAX, what, ": chunk must be a positive int32, got ", chunk);
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Smax, Smax);
  check_same_device(what, lay.list.device, {&q, &k, &v, &out, &lse, &k_lens});
  check_device_f32(lse, "lse");
  check_device_i32(k_lens, "k_lens");
  TORCH_CHECK(q.is_contiguous() && out.is_contiguous() && out.sizes() == q.sizes(), what,
              ": q and out must be contiguous [B, Hq, T, D] tensors of one shape");
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == B * Hq * T, what, ": lse must be a contiguous [B, Hq, T] tensor");
  TORCH_CHECK(k_lens.is_contiguous() && (k_lens.numel() == B || k_lens.numel() == 1), what,
              ": k_lens must be a contiguous int32 tensor of B = ", B, " entries or of one, got ", k_lens.numel());
  check_cache_strides(what, "k", k, D, "batch", 16);
  check_cache_strides(what, "v", v, D, "batch", 16);
  const auto ks = fp8_scale(what, "k_scale", k_scale, Hkv, q), vs = fp8_scale(what, "v_scale", v_scale, Hkv, q);
  check_sizes(what, {B * Hkv, B * Hq, T, Smax, D});
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  const int64_t items = B * Hkv;
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)items, (int32_t)T, (int32_t)group, (int32_t)D,
                                                                    (int32_t)Smax, (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  auto p8 = [](const torch::Tensor& t) { return static_cast<const uint8_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_decode_fp8_bf16 : mi_block_attention_decode_fp8_f16)(
      lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax,
      (int32_t)D, p(q), D, T * D, p8(k), cache_stride(k, 2, D), cache_stride(k, 1, 0), cache_stride(k, 0, 0), p8(v),
      cache_stride(v, 2, D), cache_stride(v, 1, 0), cache_stride(v, 0, 0), k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel(),
      (int32_t)group, (int32_t)chunk, (float)scale, ks.first, ks.second, vs.first, vs.second, p(out), D, T * D,
      lse.data_ptr<float>(), ws.data_ptr(), ws_bytes, stream_of(out));
  check_status(st, what);
  return out;
}

torch::Tensor block_attention_decode_paged_fp8(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                               torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                               torch::Tensor k_lens, double scale, c10::optional<torch::Tensor> k_scale,
                                               c10::optional<torch::Tensor> v_scale, int64_t chunk, torch::Tensor out,
                                               torch::Tensor lse) {
  const char* what = "block_attention_decode_paged_fp8";
  const bool bf = fp8_decode_dtypes(what, q, out, "k_pages", k_pages, "v_pages", v_pages);
  TORCH_CHECK(q.dim() == 4 && k_pages.dim() == 4 && v_pages.dim() == 4, what,
              ": q must be [B, Hq, T, D], k_pages and v_pages [P, Hkv, page, D]");
  const int64_t B = q.size(0), Hq = q.size(1), T = q.size(2), D = q.size(3);
  const int64_t P = k_pages.size(0), Hkv = k_pages.size(1), page = k_pages.size(2);
  TORCH_CHECK(k_pages.size(3) == D && v_pages.sizes() == k_pages.sizes(), what,
              ": k_pages and v_pages must be [P, Hkv, page, D] = [P, Hkv, page, ", D, "]");
  TORCH_CHECK(page >= 16 && (page & (page - 1)) == 0, what, ": a page must hold a power of two >= 16 keys, got ", page);
  TORCH_CHECK(Hkv > 0 ? Hq % Hkv == 0 : Hq == 0, what, ": ", Hq, " query heads are not a multiple of ", Hkv, " k / v heads");
  const int64_t group = Hkv > 0 ? std::max<int64_t>(Hq / Hkv, 1) : 1;
  TORCH_CHECK(chunk >= 1 && chunk <= INT32_MAX, what, ": chunk must be a positive int32, got ", chunk);
  TORCH_CHECK(block_table.dim() == 2 && block_table.size(0) == B, what, ": block_table must be [B, W] = [", B, ", W]");
  const int64_t W = block_table.size(1), Smax = W * page;
  const BlockLayout lay = block_layout(what, offsets, columns, nnz, Smax, Smax);
  check_same_device(what, lay.list.device, {&q, &k_pages, &v_pages, &block_table, &out, &lse, &k_lens});
  check_device_f32(lse, "lse");
  check_device_i32(k_lens, "k_lens");
  check_device_i32(block_table, "block_table");
  TORCH_CHECK((W <= 1 || block_table.stride(1) == 1) && (B <= 1 || block_table.stride(0) >= W), what,
              ": block_table must have a last stride of 1 and a row stride of at least W = ", W, ", got strides (",
              block_table.stride(0), ", ", block_table.stride(1), ")");
  TORCH_CHECK(q.is_contiguous() && out.is_contiguous() && out.sizes() == q.sizes(), what,
              ": q and out must be contiguous [B, Hq, T, D] tensors of one shape");
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == B * Hq * T, what, ": lse must be a contiguous [B, Hq, T] tensor");
  TORCH_CHECK(k_lens.is_contiguous() && (k_lens.numel() == B || k_lens.numel() == 1), what,
              ": k_lens must be a contiguous int32 tensor of B = ", B, " entries or of one, got ", k_lens.numel());
  check_cache_strides(what, "k_pages", k_pages, D, "page", 16);
  check_cache_strides(what, "v_pages", v_pages, D, "page", 16);
  const auto ks = fp8_scale(what, "k_scale", k_scale, Hkv, q), vs = fp8_scale(what, "v_scale", v_scale, Hkv, q);
  check_sizes(what, {B * Hkv, B * Hq, T, Smax, D, P});
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  const int64_t items = B * Hkv;
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)items, (int32_t)T, (int32_t)group, (int32_t)D,
                                                                    (int32_t)Smax, (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  auto p8 = [](const torch::Tensor& t) { return static_cast<const uint8_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_decode_paged_fp8_bf16 : mi_block_attention_decode_paged_fp8_f16)(
      lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax,
      block_table.data_ptr<int32_t>(), B > 1 ? block_table.stride(0) : W, (int32_t)P, (int32_t)page, (int32_t)D, p(q), D, T * D,
      p8(k_pages), cache_stride(k_pages, 2, D), cache_stride(k_pages, 1, 0), cache_stride(k_pages, 0, 0), p8(v_pages),
      cache_stride(v_pages, 2, D), cache_stride(v_pages, 1, 0), cache_stride(v_pages, 0, 0), k_lens.data_ptr<int32_t>(),
      (int32_t)k_lens.numel(), (int32_t)group, (int32_t)chunk, (float)scale, ks.first, ks.second, vs.first, vs.second, p(out), D,
      T * D, lse.data_ptr<float>(), ws.data_ptr(), ws_bytes, stream_of(out));
  check_status(st, what);
  return out;
}
