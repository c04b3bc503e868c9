// custom_mm — block-sparse attention for decoding: the newest tokens of every item against a key / value cache
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace (one translation unit; the
// split is for readers).  Not compiled on its own.  Contract: include/mi_spmm.h, "Block-sparse attention for decoding"
// (DESIGN.md §3.18): q and out [B, Hq, T, D] contiguous, k and v [B, Hkv, Smax, D] READ THROUGH THEIR OWN STRIDES (last
// stride 1, the others multiples of 8 elements, a 16-byte aligned data pointer — never copied), all bfloat16 or all float16;
// offsets int32 [layouts, Smax/64 + 1] with the layouts' bases, columns int32 layout-local, in 64-blocks; k_lens int32 [B]
// or [1] on the device; lse float32 [B, Hq, T].  The workspace of the chunks' partials comes from torch's allocator.

// a cache operand's strides as the kernel takes them; the message names the stride that does not fit (`outer`: the first
// one, the batch stride of a cache or the page stride of a pool; `unit`: the elements of 16 bytes — 8, or 16 of an fp8 cache)
void check_cache_strides(const char* what, const char* name, const torch::Tensor& t, int64_t D, const char* outer = "batch",
                         int64_t unit = 8) {
  TORCH_CHECK(t.stride(3) == 1 || D == 1, what, ": ", name, " must have a last stride of 1, got ", t.stride(3));
  TORCH_CHECK(t.size(2) <= 1 || (t.stride(2) >= D && t.stride(2) % unit == 0), what, ": ", name,
              "'s row stride must be a multiple of ", unit, " elements and at least D = ", D, ", got ", t.stride(2));
  TORCH_CHECK(t.size(1) <= 1 || (t.stride(1) >= 0 && t.stride(1) % unit == 0), what, ": ", name,
              "'s head stride must be a multiple of ", unit, " elements, got ", t.stride(1));
  TORCH_CHECK(t.size(0) <= 1 || (t.stride(0) >= 0 && t.stride(0) % unit == 0), what, ": ", name,
              "'s ", outer, " stride must be a multiple of ", unit, " elements, got ", t.stride(0));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, what, ": ", name, "'s data pointer must be 16-byte aligned");
}

// a stride the kernel never multiplies by anything but 0 (a dimension of one entry) is handed over as a harmless 0 / D
int64_t cache_stride(const torch::Tensor& t, int dim, int64_t fallback) { return t.size(dim) > 1 ? t.stride(dim) : fallback; }

torch::Tensor block_attention_decode(torch::Tensor offsets, torch::Tensor columns, int64_t nnz, torch::Tensor q, torch::Tensor k,
                                     torch::Tensor v, torch::Tensor k_lens, double scale, int64_t chunk, torch::Tensor out,
                                     torch::Tensor lse) {
  const char* what = "block_attention_decode";
  const torch::ScalarType dt = value_dtype(what, {{"q", &q}, {"k", &k}, {"v", &v}, {"out", &out}}, true);
  const bool bf = is_lowp_dtype(what, dt);
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
  check_cache_strides(what, "k", k, D);
  check_cache_strides(what, "v", v, D);
  check_sizes(what, {B * Hkv, B * Hq, T, Smax, D});
  if (out.numel() == 0) return out;
  c10::hip::HIPGuard guard(out.device().index());
  const int64_t items = B * Hkv;
  const size_t ws_bytes = mi_block_attention_decode_workspace_bytes((int32_t)items, (int32_t)T, (int32_t)group, (int32_t)D,
                                                                    (int32_t)Smax, (int32_t)chunk);
  torch::Tensor ws = byte_workspace(out.device(), ws_bytes, 16);
  auto p = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  const int st = (bf ? mi_block_attention_decode_bf16 : mi_block_attention_decode_f16)(
      lay.list.offsets, lay.list.columns, nnz, (int32_t)lay.layouts, (int32_t)items, (int32_t)Hkv, (int32_t)T, (int32_t)Smax,
      (int32_t)D, p(q), D, T * D, p(k), cache_stride(k, 2, D), cache_stride(k, 1, 0), cache_stride(k, 0, 0), p(v),
      cache_stride(v, 2, D), cache_stride(v, 1, 0), cache_stride(v, 0, 0), k_lens.data_ptr<int32_t>(), (int32_t)k_lens.numel(),
      (int32_t)group, (int32_t)chunk, (float)scale, p(out), D, T * D, lse.data_ptr<float>(), ws.data_ptr(), ws_bytes,
      stream_of(out));
  check_status(st, what);
  return out;
}
