// custom_mm — the fused KV-cache append: the keys and values of the newest tokens written into the decode calls' cache
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands, the sources' strides and the scales (DESIGN.md §3.23).  Not compiled on
// its own.  Contract: include/mi_spmm.h, "The fused KV-cache append" (DESIGN.md §3.21): k_new and v_new [B, Hkv, T, D]
// bfloat16 or float16 READ THROUGH THEIR OWN STRIDES; the cache of the source's dtype (a bit copy) or float8_e4m3fn (quantised
// with k_scale, v_scale); k_lens the lengths AFTER the append.  Nothing is returned.

// both forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D]
void kv_append_impl(const char* what, const char* kname, const char* vname, const char* outer, const torch::Tensor& k_new,
                    const torch::Tensor& v_new, const torch::Tensor& k, const torch::Tensor& v, const torch::Tensor* table,
                    const torch::Tensor& k_lens, const c10::optional<torch::Tensor>& k_scale,
                    const c10::optional<torch::Tensor>& v_scale) {
  const torch::ScalarType dt = value_dtype(what, {{"k_new", &k_new}, {"v_new", &v_new}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": k_new must be bfloat16 or float16, got ", dt);
  const bool fp8 = written_cache_is_fp8(what, kname, vname, dt, k, v, k_scale, v_scale);
  TORCH_CHECK(k_new.dim() == 4 && v_new.dim() == 4 && k.dim() == 4 && v.dim() == 4, what,
              ": k_new and v_new must be [B, Hkv, T, D], ", kname, " and ", vname, table ? " [P, Hkv, page, D]" : " [B, Hkv, Smax, D]");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), T = k_new.size(2), D = k_new.size(3);
  TORCH_CHECK(v_new.sizes() == k_new.sizes(), what, ": k_new and v_new must have one shape");
  check_written_cache_shape(what, kname, vname, k, v, table != nullptr, B, Hkv, D);
  check_written_cache_table(what, k, table, B, k_new.device());
  check_same_device(what, k_new.device(), {&v_new, &k, &v, &k_lens});
  check_device_i32(k_lens, "k_lens");
  check_k_lens(what, k_lens, B);
  check_source_strides(what, "k_new", k_new);
  check_source_strides(what, "v_new", v_new);
  check_cache_strides(what, kname, k, D, outer, fp8 ? 16 : 8);
  check_cache_strides(what, vname, v, D, outer, fp8 ? 16 : 8);
  const auto ks = fp8_scale(what, "k_scale", k_scale, Hkv, k_new), vs = fp8_scale(what, "v_scale", v_scale, Hkv, k_new);
  const CacheOperands c = cache_operands(k, v, table, D);
  check_sizes(what, {B * Hkv, T, c.Smax, D, c.P});
  if (k_new.numel() == 0 || k.numel() == 0) return;
  c10::hip::HIPGuard guard(k_new.device().index());
  auto src = [](const torch::Tensor& t) { return static_cast<const uint16_t*>(t.data_ptr()); };
// the argument lists of the six C entries, in pieces: [table] and [scales] are what the paged and the fp8 entries add
#define MI_APPEND_SIZES (int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax
#define MI_APPEND_TABLE c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page
#define MI_APPEND_OPERANDS(CT)                                                                                               \
  (int32_t) D, src(k_new), cache_stride(k_new, 2, D), cache_stride(k_new, 1, 0), cache_stride(k_new, 0, 0), src(v_new),       \
      cache_stride(v_new, 2, D), cache_stride(v_new, 1, 0), cache_stride(v_new, 0, 0), static_cast<CT*>(c.k), c.ldk, c.headK, \
      c.outerK, static_cast<CT*>(c.v), c.ldv, c.headV, c.outerV, k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel()
#define MI_APPEND_SCALES ks.first, ks.second, vs.first, vs.second
  mi_stream_t stream = stream_of(k_new);
  const bool bf = dt == torch::kBFloat16;
  int st;
  if (!fp8)
    st = table ? mi_kv_append_paged_b16(MI_APPEND_SIZES, MI_APPEND_TABLE, MI_APPEND_OPERANDS(uint16_t), stream)
               : mi_kv_append_b16(MI_APPEND_SIZES, MI_APPEND_OPERANDS(uint16_t), stream);
  else
    st = table ? (bf ? mi_kv_append_paged_fp8_bf16 : mi_kv_append_paged_fp8_f16)(MI_APPEND_SIZES, MI_APPEND_TABLE,
                                                                                 MI_APPEND_OPERANDS(uint8_t), MI_APPEND_SCALES, stream)
               : (bf ? mi_kv_append_fp8_bf16 : mi_kv_append_fp8_f16)(MI_APPEND_SIZES, MI_APPEND_OPERANDS(uint8_t), MI_APPEND_SCALES,
                                                                     stream);
#undef MI_APPEND_SIZES
#undef MI_APPEND_TABLE
#undef MI_APPEND_OPERANDS
#undef MI_APPEND_SCALES
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
