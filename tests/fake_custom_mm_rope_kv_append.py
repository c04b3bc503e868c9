"""fake_custom_mm_kv_append plus the two fused rotary + append entries — TEST ONLY.

Re-exports tests/fake_custom_mm_kv_append.py and adds stand-ins for custom_mm.rope_kv_append (q, k_new, v_new, cos, sin, k, v,
k_lens, new_lens, q_out, k_out, rotary_dim, interleaved, k_scale, v_scale) and custom_mm.rope_kv_append_paged (…, k_pages,
v_pages, block_table, k_lens, …) with the real entries' argument lists.  Every operand arrives AS IT IS: the call is recorded
with data pointers, strides and dtypes, so a test sees that nothing was copied or read back.  The work is done with torch on
the CPU by the rule of DESIGN.md §3.22: tests/rope_reference.py rotates, the append's stand-in writes the cache.  A plain
Python module.
"""
import torch

import rope_reference as ref
from fake_custom_mm_kv_append import *  # noqa: F401,F403
from fake_custom_mm_kv_append import _converted, _scale_record, _tensor_record, calls  # noqa: F401

F8 = torch.float8_e4m3fn


def _rope_append(name, q, k_new, v_new, cos, sin, k, v, table, k_lens, new_lens, q_out, k_out, R, interleaved, k_scale, v_scale):
    B, Hkv, T, D = k_new.shape
    dtype = q.dtype
    assert dtype in (torch.bfloat16, torch.float16) and k_new.dtype == dtype and v_new.dtype == dtype and q_out.dtype == dtype
    assert q.shape[0] == B and q.shape[2:] == k_new.shape[2:] and q_out.shape == q.shape and v_new.shape == k_new.shape
    assert k.dtype == v.dtype and k.dtype in (dtype, F8) and (k.dtype == F8 or (k_scale is None and v_scale is None))
    assert k_lens.dtype == torch.int32 and k_lens.is_contiguous() and k_lens.numel() in (1, B)
    assert new_lens is None or (new_lens.dtype == torch.int32 and new_lens.is_contiguous() and tuple(new_lens.shape) == (B,))
    assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.shape == sin.shape and cos.shape[1] == R // 2
    assert isinstance(R, int) and isinstance(interleaved, bool) and 16 <= R <= D and R % 16 == 0
    assert k_out is None or (k_out.dtype == dtype and k_out.shape == k_new.shape)
    rec = {"rotary_dim": R, "interleaved": interleaved}
    for n, t in (("q", q), ("k_new", k_new), ("v_new", v_new), ("cos", cos), ("sin", sin), ("k", k), ("v", v), ("k_lens", k_lens),
                 ("q_out", q_out)):
        rec.update(_tensor_record(n, t))
    for n, t in (("new_lens", new_lens), ("k_out", k_out)):
        rec[n] = None if t is None else _tensor_record(n, t)
    if table is not None:
        assert table.dtype == torch.int32
        rec.update(_tensor_record("table", table))
    rec["k_scale"], rec["v_scale"] = _scale_record(k_scale, Hkv), _scale_record(v_scale, Hkv)
    calls.append((name, rec))
    lens = k_lens.reshape(-1).expand(B).tolist()
    pos, token = ref.token_slots(B, T, lens, cos.shape[0], None if new_lens is None else new_lens.tolist())
    q_rot = ref.rotated(q.contiguous().view(torch.int16), dtype, cos, sin, pos, token, R, interleaved)
    k_rot = ref.rotated(k_new.contiguous().view(torch.int16), dtype, cos, sin, pos, token, R, interleaved)
    q_out.copy_(q_rot.view(dtype))
    if k_out is not None:
        k_out.copy_(k_rot.view(dtype))
    raw = torch.int16 if k.dtype == dtype else torch.uint8
    page = k.shape[2]
    smax = page if table is None else table.shape[1] * page
    for b in range(B):
        for t in range(T):
            p = int(pos[b, t])
            if not token[b, t] or not 0 <= p < smax:
                continue
            outer, row = b, p
            if table is not None:
                outer, row = int(table[b, p // page]), p % page
                if not 0 <= outer < k.shape[0]:
                    continue
            k.view(raw)[outer, :, row] = _converted(k_rot[b, :, t].view(dtype), k.dtype, k_scale)
            v.view(raw)[outer, :, row] = _converted(v_new[b, :, t], v.dtype, v_scale)
    return q_out


def rope_kv_append(q, k_new, v_new, cos, sin, k, v, k_lens, new_lens, q_out, k_out, rotary_dim, interleaved, k_scale, v_scale):
    return _rope_append("rope_kv_append", q, k_new, v_new, cos, sin, k, v, None, k_lens, new_lens, q_out, k_out, rotary_dim,
                        interleaved, k_scale, v_scale)


def rope_kv_append_paged(q, k_new, v_new, cos, sin, k_pages, v_pages, block_table, k_lens, new_lens, q_out, k_out, rotary_dim,
                         interleaved, k_scale, v_scale):
    return _rope_append("rope_kv_append_paged", q, k_new, v_new, cos, sin, k_pages, v_pages, block_table, k_lens, new_lens, q_out,
                        k_out, rotary_dim, interleaved, k_scale, v_scale)
