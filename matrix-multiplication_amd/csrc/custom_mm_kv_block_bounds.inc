// custom_mm — per-block key bounds of a key cache: the minimum and maximum of the keys of every 64-key block, kept next to the
// cache for block_select (DESIGN.md §3.29)
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands (DESIGN.md §3.23).  Not compiled on its own.  Contract: include/mi_spmm.h,
// "Query-aware key-block selection": k [B, Hkv, Smax, D] or the pool [P, Hkv, page, D] with block_table int32 [B, W], bfloat16
// or float16, READ THROUGH ITS OWN STRIDES; bounds [B, Hkv, Smax/64, 2, D] contiguous, of k's dtype, written in place; last: 0
// refreshes every block that holds a key, n ≥ 1 the blocks of the n newest positions.  Nothing is returned.  The *_fp8 forms
// (§3.32): k float8_e4m3fn with strides multiples of 16 bytes, bounds bfloat16 or float16 — its dtype names the C entry.

// all four forms: `table` null — the contiguous cache — or the block table of a pool; `fp8`: a cache of e4m3fn bytes
void kv_block_bounds_impl(const char* what, const char* kname, const char* outer, bool fp8, const torch::Tensor& k,
                          const torch::Tensor* table, const torch::Tensor& k_lens, int64_t last, const torch::Tensor& bounds) {
  TORCH_CHECK(!fp8 || k.scalar_type() == torch::kFloat8_e4m3fn, what, ": ", kname,
              " must be float8_e4m3fn (the OCP e4m3fn encoding is what is read), got ", k.scalar_type());
  const torch::ScalarType dt = fp8 ? value_dtype(what, {{"bounds", &bounds}}, true) : value_dtype(what, {{kname, &k}, {"bounds", &bounds}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": ", fp8 ? "bounds" : kname, " must be bfloat16 or float16, got ", dt);
  TORCH_CHECK(k.dim() == 4 && bounds.dim() == 5, what, ": ", kname, " must be ", table ? "[P, Hkv, page, D]" : "[B, Hkv, Smax, D]",
              " and bounds [B, Hkv, Smax/64, 2, D]");
  const int64_t B = bounds.size(0), Hkv = k.size(1), D = k.size(3);
  TORCH_CHECK(table || k.size(0) == B, what, ": k and bounds must have one batch size");
  if (table) {
    check_page(what, "keys", k.size(2));
    table_width(what, *table, B);
    check_table(what, *table);
    check_same_device(what, k.device(), {table});
  }
  check_same_device(what, k.device(), {&bounds, &k_lens});
  check_device_i32(k_lens, "k_lens");
  check_k_lens(what, k_lens, B);
  check_cache_strides(what, kname, k, D, outer, fp8 ? 16 : 8);
  const CacheOperands c = cache_operands(k, k, table, D);
  TORCH_CHECK(c.Smax % 64 == 0, what, ": Smax = ", c.Smax, " must be a multiple of 64");
  TORCH_CHECK(bounds.is_contiguous() && bounds.size(1) == Hkv && bounds.size(2) == c.Smax / 64 && bounds.size(3) == 2 &&
                  bounds.size(4) == D,
              what, ": bounds must be a contiguous [B, Hkv, Smax/64, 2, D] = [", B, ", ", Hkv, ", ", c.Smax / 64, ", 2, ", D, "] tensor");
  TORCH_CHECK(last >= 0 && last <= INT32_MAX, what, ": last must be 0 (every block) or a positive int32, got ", last);
  check_sizes(what, {B * Hkv, c.Smax, D, c.P});
  if (bounds.numel() == 0 || k.numel() == 0) return;
  c10::hip::HIPGuard guard(k.device().index());
  mi_stream_t stream = stream_of(k);
  const bool bf = dt == torch::kBFloat16;
#define MI_BOUNDS_OPERANDS(CT)                                                                                        \
  (int32_t) D, static_cast<const CT*>(c.k), c.ldk, c.headK, c.outerK, k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel(), \
      (int32_t)last, bits16(bounds), stream
#define MI_BOUNDS_PAGED_HEAD (int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)c.Smax, c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page
  int st;
  if (fp8)
    st = table ? (bf ? mi_kv_block_bounds_paged_fp8_bf16 : mi_kv_block_bounds_paged_fp8_f16)(MI_BOUNDS_PAGED_HEAD, MI_BOUNDS_OPERANDS(uint8_t))
               : (bf ? mi_kv_block_bounds_fp8_bf16 : mi_kv_block_bounds_fp8_f16)((int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)c.Smax,
                                                                                 MI_BOUNDS_OPERANDS(uint8_t));
  else
    st = table ? (bf ? mi_kv_block_bounds_paged_bf16 : mi_kv_block_bounds_paged_f16)(
                             MI_BOUNDS_PAGED_HEAD, MI_BOUNDS_OPERANDS(uint16_t))
                       : (bf ? mi_kv_block_bounds_bf16 : mi_kv_block_bounds_f16)((int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)c.Smax,
                                                                                 MI_BOUNDS_OPERANDS(uint16_t));
#undef MI_BOUNDS_OPERANDS
#undef MI_BOUNDS_PAGED_HEAD
  check_status(st, what);
}

void kv_block_bounds(torch::Tensor k, torch::Tensor k_lens, int64_t last, torch::Tensor bounds) {
  kv_block_bounds_impl("kv_block_bounds", "k", "batch", false, k, nullptr, k_lens, last, bounds);
}

void kv_block_bounds_paged(torch::Tensor k_pages, torch::Tensor block_table, torch::Tensor k_lens, int64_t last, torch::Tensor bounds) {
  kv_block_bounds_impl("kv_block_bounds_paged", "k_pages", "page", false, k_pages, &block_table, k_lens, last, bounds);
}

void kv_block_bounds_fp8(torch::Tensor k, torch::Tensor k_lens, int64_t last, torch::Tensor bounds) {
  kv_block_bounds_impl("kv_block_bounds_fp8", "k", "batch", true, k, nullptr, k_lens, last, bounds);
}

void kv_block_bounds_paged_fp8(torch::Tensor k_pages, torch::Tensor block_table, torch::Tensor k_lens, int64_t last,
                               torch::Tensor bounds) {
  kv_block_bounds_impl("kv_block_bounds_paged_fp8", "k_pages", "page", true, k_pages, &block_table, k_lens, last, bounds);
}
