// custom_mm — block-sparse attention for decoding over a paged key / value cache: a pool of pages and a block table
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after
// custom_mm_block_attention_decode.inc, whose stride checks it shares.  Not compiled on its own.  Contract: include/mi_spmm.h,
// "… over a paged cache" (DESIGN.md §3.19): q and out [B, Hq, T, D] contiguous, k_pages and v_pages [P, Hkv, page, D] READ
// THROUGH THEIR OWN STRIDES (last stride 1, the others multiples of 8 elements, a 16-byte aligned data pointer — never
// copied), all bfloat16 or all float16; page a power of two ≥ 16; block_table int32 [B, W] with a last stride of 1 and a row
// stride ≥ W, handed over as it is; Smax = W · page; offsets int32 [layouts, Smax/64 + 1], columns int32 layout-local, in
// 64-blocks; k_lens int32 [B] or [1] on the device; lse float32 [B, Hq, T].  The workspace comes from torch's allocator.

torch::Tensor block_attention_decode_paged(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q,
                                           torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table,
                                           torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out, torch::Tensor lse) {
  const char* what = "block_attention_decode_paged";
  const torch::ScalarType dt = value_dtype(what, {{"q", &q}, {"k_pages", &k_pages}, {"v_pages", &v_pages}, {"out", &out}}, true);
  const bool bf = is_lowp_dtype(what, dt);
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
  check_cache_strides(what, "k_pages", k_pages, D, "page");
  check_cache_strides(what, "v_pages", v_pages, D, "page");
  check_sizes(what, {B * Hkv, B * Hq, T, Smax, D, P});
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  const int64_t items = B * Hkv;
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)items, (int32_t)T, (int32_t)group, (int32_t)D,
                                                                    (int32_t)Smax, (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_decode_paged_bf16 : mi_block_attention_decode_paged_f16)(
      lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax,
      block_table.data_ptr<int32_t>(), B > 1 ? block_table.stride(0) : W, (int32_t)P, (int32_t)page, (int32_t)D, p(q), D, T * D,
      p(k_pages), cache_stride(k_pages, 2, D), cache_stride(k_pages, 1, 0), cache_stride(k_pages, 0, 0), p(v_pages),
      cache_stride(v_pages, 2, D), cache_stride(v_pages, 1, 0), cache_stride(v_pages, 0, 0), k_lens.data_ptr<int32_t>(),
      (int32_t)k_lens.numel(), (int32_t)group, (int32_t)chunk, (float)scale, p(out), D, T * D, lse.data_ptr<float>(), ws.data_ptr(),
      ws_bytes, stream_of(out));
  check_status(st, what);
  return out;
}
