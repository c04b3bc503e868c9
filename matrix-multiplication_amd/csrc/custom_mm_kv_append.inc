// custom_mm — the fused KV-cache append: the keys and values of the newest tokens written into the decode calls' cache
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after
// custom_mm_block_attention_decode_fp8.inc, whose cache-stride and scale checks it shares.  Not compiled on its own.  Contract:
// include/mi_spmm.h, "The fused KV-cache append" (DESIGN.md §3.21): k_new and v_new [B, Hkv, T, D] bfloat16 or float16 READ
// THROUGH THEIR OWN STRIDES (last stride 1, the others multiples of 8 elements, a 16-byte aligned data pointer — never copied);
// the cache k, v [B, Hkv, Smax, D] or k_pages, v_pages [P, Hkv, page, D] with block_table int32 [B, W], as the decode entries
// take them, of the source's dtype (a bit copy) or float8_e4m3fn (quantised with k_scale, v_scale: None or float32 device
// tensors of 1 or Hkv entries); k_lens int32 [B] or [1] on the device, the lengths AFTER the append.  Nothing is returned.

// a source operand's strides as the kernel takes them; the message names the stride that does not fit
void check_source_strides(const char* what, const char* name, const torch::Tensor& t) {
  static const char* const dims[] = {"batch", "head", "token"};
  TORCH_CHECK(t.stride(3) == 1 || t.size(3) <= 1, what, ": ", name, " must have a last stride of 1, got ", t.stride(3));
  for (int d = 2; d >= 0; --d)
    TORCH_CHECK(t.size(d) <= 1 || (t.stride(d) >= 0 && t.stride(d) % 8 == 0), what, ": ", name, "'s ", dims[d],
                " stride must be a multiple of 8 elements, got ", t.stride(d));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what, ": ", name, "'s data pointer must be 16-byte aligned");
}

// both forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D]
void kv_append_impl(const char* what, const char* kname, const char* vname, const char* outer, const torch::Tensor& k_new,
                    const torch::Tensor& v_new, const torch::Tensor& k, const torch::Tensor& v, const torch::Tensor* table,
                    const torch::Tensor& k_lens, const c10::optional<torch::Tensor>& k_scale,
                    const c10::optional<torch::Tensor>& v_scale) {
  const torch::ScalarType dt = value_dtype(what, {{"k_new", &k_new}, {"v_new", &v_new}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": k_new must be bfloat16 or float16, got ", dt);
  const bool fp8 = k.scalar_type() != dt || v.scalar_type() != dt;
  TORCH_CHECK(!fp8 || (k.scalar_type() == torch::kFloat8_e4m3fn && v.scalar_type() == torch::kFloat8_e4m3fn), what, ": ", kname,
              " and ", vname, " must have k_new's dtype ", dt, " or be float8_e4m3fn (the OCP e4m3fn encoding is what is written), got ",
              k.scalar_type(), " and ", v.scalar_type());
  TORCH_CHECK(fp8 || (!k_scale.has_value() && !v_scale.has_value()), what, ": k_scale and v_scale go with a float8_e4m3fn cache only");
  TORCH_CHECK(k_new.dim() == 4 && v_new.dim() == 4 && k.dim() == 4 && v.dim() == 4, what,
              ": k_new and v_new must be [B, Hkv, T, D], ", kname, " and ", vname, table ? " [P, Hkv, page, D]" : " [B, Hkv, Smax, D]");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), T = k_new.size(2), D = k_new.size(3);
  TORCH_CHECK(v_new.sizes() == k_new.sizes(), what, ": k_new and v_new must have one shape");
  TORCH_CHECK((table || k.size(0) == B) && k.size(1) == Hkv && k.size(3) == D && v.sizes() == k.sizes(), what, ": ", kname, " and ",
              vname, " must be ", table ? "[P, Hkv, page, D]" : "[B, Hkv, Smax, D]", " with k_new's B = ", B, ", Hkv = ", Hkv,
              " and D = ", D);
  int64_t Smax = k.size(2), P = 0, page = 0, W = 0;
  if (table) {
    P = k.size(0), page = k.size(2);
    TORCH_CHECK(page >= 16 && (page & (page - 1)) == 0, what, ": a page must hold a power of two >= 16 rows, got ", page);
    TORCH_CHECK(table->dim() == 2 && table->size(0) == B, what, ": block_table must be [B, W] = [", B, ", W]");
    W = table->size(1), Smax = W * page;
    check_device_i32(*table, "block_table");
    TORCH_CHECK((W <= 1 || table->stride(1) == 1) && (B <= 1 || table->stride(0) >= W), what,
                ": block_table must have a last stride of 1 and a row stride of at least W = ", W, ", got strides (",
                table->stride(0), ", ", table->stride(1), ")");
    check_same_device(what, k_new.device(), {table});
  }
  check_same_device(what, k_new.device(), {&v_new, &k, &v, &k_lens});
  check_device_i32(k_lens, "k_lens");
  TORCH_CHECK(k_lens.is_contiguous() && (k_lens.numel() == B || k_lens.numel() == 1), what,
              ": k_lens must be a contiguous int32 tensor of B = ", B, " entries or of one, got ", k_lens.numel());
  check_source_strides(what, "k_new", k_new);
  check_source_strides(what, "v_new", v_new);
  check_cache_strides(what, kname, k, D, outer, fp8 ? 16 : 8);
  check_cache_strides(what, vname, v, D, outer, fp8 ? 16 : 8);
  const auto ks = fp8_scale(what, "k_scale", k_scale, Hkv, k_new), vs = fp8_scale(what, "v_scale", v_scale, Hkv, k_new);
  check_sizes(what, {B * Hkv, T, Smax, D, P});
  if (k_new.numel() == 0 || k.numel() == 0) return;
  c10::hip::HIPGuard guard(k_new.device().index());
  const int32_t items = (int32_t)(B * Hkv), lens_count = (int32_t)k_lens.numel();
  auto src = [](const torch::Tensor& t) { return static_cast<const uint16_t*>(t.data_ptr()); };
  const int64_t ldkn = cache_stride(k_new, 2, D), headKn = cache_stride(k_new, 1, 0), batchKn = cache_stride(k_new, 0, 0);
  const int64_t ldvn = cache_stride(v_new, 2, D), headVn = cache_stride(v_new, 1, 0), batchVn = cache_stride(v_new, 0, 0);
  const int64_t ldk = cache_stride(k, 2, D), headK = cache_stride(k, 1, 0), outerK = cache_stride(k, 0, 0);
  const int64_t ldv = cache_stride(v, 2, D), headV = cache_stride(v, 1, 0), outerV = cache_stride(v, 0, 0);
  const int32_t* lens = k_lens.data_ptr<int32_t>();
  const int32_t* tab = table ? table->data_ptr<int32_t>() : nullptr;
  const int64_t table_ld = table ? (B > 1 ? table->stride(0) : W) : 0;
  mi_stream_t stream = stream_of(k_new);
  int st;
  if (!fp8) {
    auto dst = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
    st = table ? mi_kv_append_paged_b16(items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax, tab, table_ld, (int32_t)P, (int32_t)page,
                                        (int32_t)D, src(k_new), ldkn, headKn, batchKn, src(v_new), ldvn, headVn, batchVn, dst(k), ldk,
                                        headK, outerK, dst(v), ldv, headV, outerV, lens, lens_count, stream)
               : mi_kv_append_b16(items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax, (int32_t)D, src(k_new), ldkn, headKn, batchKn,
                                  src(v_new), ldvn, headVn, batchVn, dst(k), ldk, headK, outerK, dst(v), ldv, headV, outerV, lens,
                                  lens_count, stream);
  } else {
    auto dst = [](const torch::Tensor& t) { return static_cast<uint8_t*>(t.data_ptr()); };
    const bool bf = dt == torch::kBFloat16;
    st = table ? (bf ? mi_kv_append_paged_fp8_bf16 : mi_kv_append_paged_fp8_f16)(
                     items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax, tab, table_ld, (int32_t)P, (int32_t)page, (int32_t)D, src(k_new),
                     ldkn, headKn, batchKn, src(v_new), ldvn, headVn, batchVn, dst(k), ldk, headK, outerK, dst(v), ldv, headV, outerV,
                     lens, lens_count, ks.first, ks.second, vs.first, vs.second, stream)
               : (bf ? mi_kv_append_fp8_bf16 : mi_kv_append_fp8_f16)(
                     items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax, (int32_t)D, src(k_new), ldkn, headKn, batchKn, src(v_new), ldvn,
                     headVn, batchVn, dst(k), ldk, headK, outerK, dst(v), ldv, headV, outerV, lens, lens_count, ks.first, ks.second,
                     vs.first, vs.second, stream);
  }
  check_status(st, what);
}

void kv_append(torch::Tensor k_new, torch::Tensor v_new, torch::Tensor k, torch::Tensor v, torch::Tensor k_lens,
               c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale) {
  kv_append_impl("kv_append", "k", "v", "batch", k_new, v_new, k, v, nullptr, k_lens, k_scale, v_scale);
}

void kv_append_paged(torch::Tensor k_new, torch::Tensor v_new, torch::Tensor k_pages, torch::Tensor v_pages,
                     torch::Tensor block_table, torch::Tensor k_lens, c10::optional<torch::Tensor> k_scale,
                     c10::optional<torch::Tensor> v_scale) {
  kv_append_impl("kv_append_paged", "k_pages", "v_pages", "page", k_new, v_new, k_pages, v_pages, &block_table, k_lens, k_scale,
                 v_scale);
}
