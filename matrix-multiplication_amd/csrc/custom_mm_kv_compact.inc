// custom_mm — compaction after a speculative step: the accepted path's k / v rows moved to the front of the drafted window
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands (DESIGN.md §3.23).  Not compiled on its own.  Contract: include/mi_spmm.h,
// "Compaction after a speculative step" (DESIGN.md §3.34): the cache of kv_append — bfloat16, float16 or float8_e4m3fn, rows are
// bit copies —, k_lens int32 [B] or [1] still counting the T drafted slots, accept int32 [B, T], accept_counts int32 [B].

// both forms: `table` null — the contiguous cache [B, Hkv, Smax, D] — or the block table of a pool [P, Hkv, page, D]
void kv_compact_impl(const char* what, const char* kname, const char* vname, const char* outer, const torch::Tensor& k,
                     const torch::Tensor& v, const torch::Tensor* table, const torch::Tensor& k_lens, const torch::Tensor& accept,
                     const torch::Tensor& accept_counts, int64_t T) {
  TORCH_CHECK(k.is_cuda() && v.is_cuda(), kname, " and ", vname, " must be device (HIP) tensors; custom_mm has no CPU path");
  const torch::ScalarType dt = k.scalar_type();
  TORCH_CHECK((is_lowp(dt) || dt == torch::kFloat8_e4m3fn) && v.scalar_type() == dt, what, ": ", kname, " and ", vname,
              " must share one dtype — bfloat16, float16 or float8_e4m3fn —, got ", dt, " and ", v.scalar_type());
  const bool fp8 = dt == torch::kFloat8_e4m3fn;
  TORCH_CHECK(k.dim() == 4 && v.dim() == 4 && accept.dim() == 2, what, ": ", kname, " and ", vname, " must be ",
              table ? "[P, Hkv, page, D]" : "[B, Hkv, Smax, D]", ", accept [B, T]");
  const int64_t B = accept.size(0), Hkv = k.size(1), D = k.size(3);
  TORCH_CHECK(T >= 0 && T <= 64 && accept.size(1) == T && accept.is_contiguous(), what, ": accept must be a contiguous [B, T] tensor with "
              "T = ", T, " <= 64");
  TORCH_CHECK(accept_counts.dim() == 1 && accept_counts.size(0) == B && accept_counts.is_contiguous(), what,
              ": accept_counts must be a contiguous [B] = [", B, "] tensor");
  check_written_cache_shape(what, kname, vname, k, v, table != nullptr, B, Hkv, D);
  check_written_cache_table(what, k, table, B, k.device());
  check_same_device(what, k.device(), {&v, &k_lens, &accept, &accept_counts});
  check_device_i32(k_lens, "k_lens");
  check_device_i32(accept, "accept");
  check_device_i32(accept_counts, "accept_counts");
  check_k_lens(what, k_lens, B);
  check_cache_strides(what, kname, k, D, outer, fp8 ? 16 : 8);
  check_cache_strides(what, vname, v, D, outer, fp8 ? 16 : 8);
  const CacheOperands c = cache_operands(k, v, table, D);
  check_sizes(what, {B * Hkv, T, c.Smax, D, c.P});
  if (B * Hkv == 0 || T == 0 || k.numel() == 0) return;
  c10::hip::HIPGuard guard(k.device().index());
#define MI_COMPACT_OPERANDS                                                                                                      \
  (int32_t) D, fp8 ? 1 : 2, c.k, c.ldk, c.headK, c.outerK, c.v, c.ldv, c.headV, c.outerV, k_lens.data_ptr<int32_t>(),          \
      (int32_t)k_lens.numel(), accept.data_ptr<int32_t>(), accept_counts.data_ptr<int32_t>(), stream_of(k)
  const int st = table ? mi_kv_compact_paged((int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, c.table, c.table_ld,
                                             (int32_t)c.P, (int32_t)c.page, MI_COMPACT_OPERANDS)
                       : mi_kv_compact((int32_t)(B * Hkv), (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, MI_COMPACT_OPERANDS);
#undef MI_COMPACT_OPERANDS
  check_status(st, what);
}

void kv_compact(torch::Tensor k, torch::Tensor v, torch::Tensor k_lens, torch::Tensor accept, torch::Tensor accept_counts, int64_t T) {
  kv_compact_impl("kv_compact", "k", "v", "batch", k, v, nullptr, k_lens, accept, accept_counts, T);
}

void kv_compact_paged(torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table, torch::Tensor k_lens,
                      torch::Tensor accept, torch::Tensor accept_counts, int64_t T) {
  kv_compact_impl("kv_compact_paged", "k_pages", "v_pages", "page", k_pages, v_pages, &block_table, k_lens, accept, accept_counts, T);
}
