// custom_mm — the fused rotary embedding + KV-cache append: q and the new keys rotated by position, the rotated keys and the
// values written into the decode calls' cache, the rotated q into q_out, in one launch
// Part of the `custom_mm` extension: included by custom_mm.cpp inside its anonymous namespace, after custom_mm_kv_cache.inc,
// which owns what is said about the cache operands, the sources' strides and the scales (DESIGN.md §3.23).  Not compiled on
// its own.
// Contract: include/mi_spmm.h, "The fused rotary embedding + KV-cache append" (DESIGN.md §3.22): q [B, Hq, T, D], k_new and
// v_new [B, Hkv, T, D] bfloat16 or float16 READ THROUGH THEIR OWN STRIDES; cos, sin float32 [Pmax, R/2] (last stride 1, one
// row stride ≥ R/2 that is a multiple of 4, 16-byte aligned); the cache, block_table, k_lens and the scales as kv_append takes
// them; new_lens None or int32 [B]; q_out [B, Hq, T, D] and k_out None or [B, Hkv, T, D] under the source's stride rules.
// Returns q_out.

torch::Tensor rope_kv_append_impl(const char* what, const char* kname, const char* vname, const char* outer, const torch::Tensor& q,
                                  const torch::Tensor& k_new, const torch::Tensor& v_new, const torch::Tensor& cos,
                                  const torch::Tensor& sin, const torch::Tensor& k, const torch::Tensor& v, const torch::Tensor* table,
                                  const torch::Tensor& k_lens, const c10::optional<torch::Tensor>& new_lens, torch::Tensor q_out,
                                  const c10::optional<torch::Tensor>& k_out, int64_t R, bool interleaved,
                                  const c10::optional<torch::Tensor>& k_scale, const c10::optional<torch::Tensor>& v_scale,
                                  const torch::Tensor* positions = nullptr) {
  const torch::ScalarType dt = value_dtype(what, {{"q", &q}, {"k_new", &k_new}, {"v_new", &v_new}, {"q_out", &q_out}}, true);
  TORCH_CHECK(is_lowp(dt), what, ": q must be bfloat16 or float16, got ", dt);
  TORCH_CHECK(!k_out.has_value() || k_out->scalar_type() == dt, what, ": k_out must have q's dtype ", dt, ", got ",
              k_out.has_value() ? k_out->scalar_type() : dt);
  const bool fp8 = written_cache_is_fp8(what, kname, vname, dt, k, v, k_scale, v_scale);
  TORCH_CHECK(q.dim() == 4 && k_new.dim() == 4 && v_new.dim() == 4 && k.dim() == 4 && v.dim() == 4, what,
              ": q must be [B, Hq, T, D], k_new and v_new [B, Hkv, T, D], ", kname, " and ", vname,
              table ? " [P, Hkv, page, D]" : " [B, Hkv, Smax, D]");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), T = k_new.size(2), D = k_new.size(3), Hq = q.size(1);
  TORCH_CHECK(v_new.sizes() == k_new.sizes(), what, ": k_new and v_new must have one shape");
  TORCH_CHECK(q.size(0) == B && q.size(2) == T && q.size(3) == D && Hq >= 1, what, ": q must be [B, Hq, T, D] with k_new's B = ", B,
              ", T = ", T, " and D = ", D, " and Hq >= 1");
  TORCH_CHECK(q_out.sizes() == q.sizes(), what, ": q_out must have q's shape");
  TORCH_CHECK(!k_out.has_value() || k_out->sizes() == k_new.sizes(), what, ": k_out must have k_new's shape");
  check_written_cache_shape(what, kname, vname, k, v, table != nullptr, B, Hkv, D);
  TORCH_CHECK(R >= 16 && R <= D && R % 16 == 0, what, ": rotary_dim must be a multiple of 16 in [16, D = ", D, "], got ", R);
  check_device_f32(cos, "cos");
  check_device_f32(sin, "sin");
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == R / 2 && sin.sizes() == cos.sizes(), what,
              ": cos and sin must be float32 [Pmax, rotary_dim / 2 = ", R / 2, "] tensors of one shape");
  const int64_t Pmax = cos.size(0);
  const int64_t ld = Pmax > 1 ? cos.stride(0) : (R / 2 + 3) / 4 * 4;
  TORCH_CHECK(cos.stride(1) == 1 && sin.stride(1) == 1 && (Pmax <= 1 || (ld >= R / 2 && ld % 4 == 0 && sin.stride(0) == ld)), what,
              ": cos and sin must have a last stride of 1 and one row stride that is a multiple of 4 and at least rotary_dim / 2, got (",
              cos.stride(0), ", ", cos.stride(1), ") and (", sin.stride(0), ", ", sin.stride(1), ")");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(cos.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(sin.data_ptr()) % 16 == 0, what,
              ": the data pointers of cos and sin must be 16-byte aligned");
  check_written_cache_table(what, k, table, B, q.device());
  check_same_device(what, q.device(), {&k_new, &v_new, &cos, &sin, &k, &v, &k_lens, &q_out});
  check_device_i32(k_lens, "k_lens");
  check_k_lens(what, k_lens, B);
  if (new_lens.has_value()) {
    check_same_device(what, q.device(), {&*new_lens});
    check_device_i32(*new_lens, "new_lens");
    TORCH_CHECK(new_lens->is_contiguous() && new_lens->dim() == 1 && new_lens->numel() == B, what,
                ": new_lens must be a contiguous int32 tensor of B = ", B, " entries");
  }
  if (positions) {  // the *_pos bindings (DESIGN.md §3.34): the table row of every slot's rotation, handed over as it is
    check_same_device(what, q.device(), {positions});
    check_device_i32(*positions, "positions");
    TORCH_CHECK(positions->is_contiguous() && positions->dim() == 2 && positions->size(0) == B && positions->size(1) == T, what,
                ": positions must be a contiguous int32 [B, T] = [", B, ", ", T, "] tensor");
  }
  check_source_strides(what, "q", q);
  check_source_strides(what, "k_new", k_new);
  check_source_strides(what, "v_new", v_new);
  check_source_strides(what, "q_out", q_out);
  if (k_out.has_value()) {
    check_same_device(what, q.device(), {&*k_out});
    check_source_strides(what, "k_out", *k_out);
  }
  check_cache_strides(what, kname, k, D, outer, fp8 ? 16 : 8);
  check_cache_strides(what, vname, v, D, outer, fp8 ? 16 : 8);
  const auto ks = fp8_scale(what, "k_scale", k_scale, Hkv, q), vs = fp8_scale(what, "v_scale", v_scale, Hkv, q);
  const CacheOperands c = cache_operands(k, v, table, D);
  check_sizes(what, {B * Hkv, B * Hq, T, c.Smax, D, c.P, Pmax});
  if (q.numel() == 0) return q_out;
  c10::hip::HIPGuard guard(q.device().index());
  const int32_t items = (int32_t)(B * Hkv), lens_count = (int32_t)k_lens.numel();
  auto src = [](const torch::Tensor& t) { return static_cast<const uint16_t*>(t.data_ptr()); };
  auto dst16 = [](const torch::Tensor& t) { return static_cast<uint16_t*>(t.data_ptr()); };
  auto st3 = [D](const torch::Tensor& t) {
    return std::array<int64_t, 3>{cache_stride(t, 2, D), cache_stride(t, 1, 0), cache_stride(t, 0, 0)};
  };
  const auto sq = st3(q), sqo = st3(q_out), skn = st3(k_new), svn = st3(v_new);
  const auto sko = k_out.has_value() ? st3(*k_out) : std::array<int64_t, 3>{D, 0, 0};
  uint16_t* ko = k_out.has_value() ? dst16(*k_out) : nullptr;
  const int32_t* lens = k_lens.data_ptr<int32_t>();
  const int32_t* nl = new_lens.has_value() ? new_lens->data_ptr<int32_t>() : nullptr;
  const float *cp = Pmax > 0 ? cos.data_ptr<float>() : nullptr, *sp = Pmax > 0 ? sin.data_ptr<float>() : nullptr;
  const bool bf = dt == torch::kBFloat16;
  mi_stream_t stream = stream_of(q);
  int st;
// the operand list of MI_ROPE_KV_APPEND_OPERANDS, with the cache pointers of type CT
#define MI_ROPE_CALL_OPERANDS(CT)                                                                                                   \
  (int32_t) Hq, src(q), sq[0], sq[1], sq[2], dst16(q_out), sqo[0], sqo[1], sqo[2], src(k_new), skn[0], skn[1], skn[2], src(v_new),  \
      svn[0], svn[1], svn[2], ko, sko[0], sko[1], sko[2], cp, sp, (int32_t)Pmax, ld, (int32_t)R, (int32_t)interleaved,              \
      static_cast<CT*>(c.k), c.ldk, c.headK, c.outerK, static_cast<CT*>(c.v), c.ldv, c.headV, c.outerV, lens, lens_count, nl
  if (positions) {
    const int32_t* pp = positions->data_ptr<int32_t>();
    if (!fp8)
      st = table ? (bf ? mi_rope_pos_kv_append_paged_bf16 : mi_rope_pos_kv_append_paged_f16)(
                       items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page, (int32_t)D,
                       MI_ROPE_CALL_OPERANDS(uint16_t), pp, stream)
                 : (bf ? mi_rope_pos_kv_append_bf16 : mi_rope_pos_kv_append_f16)(items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax,
                                                                                 (int32_t)D, MI_ROPE_CALL_OPERANDS(uint16_t), pp, stream);
    else
      st = table ? (bf ? mi_rope_pos_kv_append_paged_fp8_bf16 : mi_rope_pos_kv_append_paged_fp8_f16)(
                       items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page, (int32_t)D,
                       MI_ROPE_CALL_OPERANDS(uint8_t), pp, ks.first, ks.second, vs.first, vs.second, stream)
                 : (bf ? mi_rope_pos_kv_append_fp8_bf16 : mi_rope_pos_kv_append_fp8_f16)(
                       items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, (int32_t)D, MI_ROPE_CALL_OPERANDS(uint8_t), pp, ks.first,
                       ks.second, vs.first, vs.second, stream);
  } else if (!fp8) {
    st = table ? (bf ? mi_rope_kv_append_paged_bf16 : mi_rope_kv_append_paged_f16)(
                     items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page, (int32_t)D,
                     MI_ROPE_CALL_OPERANDS(uint16_t), stream)
               : (bf ? mi_rope_kv_append_bf16 : mi_rope_kv_append_f16)(items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, (int32_t)D,
                                                                       MI_ROPE_CALL_OPERANDS(uint16_t), stream);
  } else {
    st = table ? (bf ? mi_rope_kv_append_paged_fp8_bf16 : mi_rope_kv_append_paged_fp8_f16)(
                     items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, c.table, c.table_ld, (int32_t)c.P, (int32_t)c.page, (int32_t)D,
                     MI_ROPE_CALL_OPERANDS(uint8_t), ks.first, ks.second, vs.first, vs.second, stream)
               : (bf ? mi_rope_kv_append_fp8_bf16 : mi_rope_kv_append_fp8_f16)(
                     items, (int32_t)Hkv, (int32_t)T, (int32_t)c.Smax, (int32_t)D, MI_ROPE_CALL_OPERANDS(uint8_t), ks.first, ks.second,
                     vs.first, vs.second, stream);
  }
#undef MI_ROPE_CALL_OPERANDS
  check_status(st, what);
  return q_out;
}

torch::Tensor rope_kv_append(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor cos, torch::Tensor sin,
                             torch::Tensor k, torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens,
                             torch::Tensor q_out, c10::optional<torch::Tensor> k_out, int64_t rotary_dim, bool interleaved,
                             c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale) {
  return rope_kv_append_impl("rope_kv_append", "k", "v", "batch", q, k_new, v_new, cos, sin, k, v, nullptr, k_lens, new_lens, q_out,
                             k_out, rotary_dim, interleaved, k_scale, v_scale);
}

torch::Tensor rope_kv_append_paged(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor cos, torch::Tensor sin,
                                   torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table, torch::Tensor k_lens,
                                   c10::optional<torch::Tensor> new_lens, torch::Tensor q_out, c10::optional<torch::Tensor> k_out,
                                   int64_t rotary_dim, bool interleaved, c10::optional<torch::Tensor> k_scale,
                                   c10::optional<torch::Tensor> v_scale) {
  return rope_kv_append_impl("rope_kv_append_paged", "k_pages", "v_pages", "page", q, k_new, v_new, cos, sin, k_pages, v_pages,
                             &block_table, k_lens, new_lens, q_out, k_out, rotary_dim, interleaved, k_scale, v_scale);
}

// … with explicit positions (DESIGN.md §3.34): `positions` int32 [B, T] after v_scale
torch::Tensor rope_kv_append_pos(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor cos, torch::Tensor sin,
                                 torch::Tensor k, torch::Tensor v, torch::Tensor k_lens, c10::optional<torch::Tensor> new_lens,
                                 torch::Tensor q_out, c10::optional<torch::Tensor> k_out, int64_t rotary_dim, bool interleaved,
                                 c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale, torch::Tensor positions) {
  return rope_kv_append_impl("rope_kv_append_pos", "k", "v", "batch", q, k_new, v_new, cos, sin, k, v, nullptr, k_lens, new_lens, q_out,
                             k_out, rotary_dim, interleaved, k_scale, v_scale, &positions);
}

torch::Tensor rope_kv_append_paged_pos(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor cos, torch::Tensor sin,
                                       torch::Tensor k_pages, torch::Tensor v_pages, torch::Tensor block_table, torch::Tensor k_lens,
                                       c10::optional<torch::Tensor> new_lens, torch::Tensor q_out, c10::optional<torch::Tensor> k_out,
                                       int64_t rotary_dim, bool interleaved, c10::optional<torch::Tensor> k_scale,
                                       c10::optional<torch::Tensor> v_scale, torch::Tensor positions) {
  return rope_kv_append_impl("rope_kv_append_paged_pos", "k_pages", "v_pages", "page", q, k_new, v_new, cos, sin, k_pages, v_pages,
                             &block_table, k_lens, new_lens, q_out, k_out, rotary_dim, interleaved, k_scale, v_scale, &positions);
}
