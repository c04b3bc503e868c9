"""fake_custom_mm_block_attention_decode_fp8 plus the two append entries — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention_decode_fp8.py and adds stand-ins for custom_mm.kv_append (k_new, v_new, k, v,
k_lens, k_scale, v_scale) and custom_mm.kv_append_paged (k_new, v_new, k_pages, v_pages, block_table, k_lens, k_scale,
v_scale) with the real entries' argument lists.  Every operand arrives AS IT IS: the call is recorded with data pointers,
strides and dtypes — the scales as None or (data_ptr, shape, a clone) — so a test sees that nothing was copied or read back.
The write is done with torch on the CPU, token by token, by the rule of DESIGN.md §3.21: token t of item b goes to
k_lens[b] − T + t, or nowhere.  A plain Python module.
"""
import torch

from fake_custom_mm_block_attention_decode_fp8 import *  # noqa: F401,F403
from fake_custom_mm_block_attention_decode_fp8 import _scale_record, calls  # noqa: F401

F8 = torch.float8_e4m3fn


def _tensor_record(name, t):
    return {f"{name}_ptr": t.data_ptr(), f"{name}_stride": tuple(t.stride()), f"{name}_dtype": t.dtype, f"{name}_shape": tuple(t.shape)}


def _converted(x, cache_dtype, s):
    """The rows x [Hkv, D] as the cache stores them, as raw integers: a bit copy, or torch's CPU fp8 cast of x / s clamped."""
    if cache_dtype == x.dtype:
        return x.contiguous().view(torch.int16)
    Hkv = x.shape[0]
    scale = torch.ones(Hkv) if s is None else s.reshape(-1).expand(Hkv)
    return (x.float() / scale.reshape(Hkv, 1)).clamp(-448.0, 448.0).to(F8).view(torch.uint8)


def _append(name, k_new, v_new, k, v, table, k_lens, k_scale, v_scale):
    B, Hkv, T, D = k_new.shape
    assert k_new.dtype in (torch.bfloat16, torch.float16) and v_new.dtype == k_new.dtype
    assert k.dtype == v.dtype and k.dtype in (k_new.dtype, F8)
    assert k_lens.dtype == torch.int32 and k_lens.is_contiguous() and k_lens.numel() in (1, B)
    assert k.dtype == F8 or (k_scale is None and v_scale is None)
    rec = {}
    for n, t in (("k_new", k_new), ("v_new", v_new), ("k", k), ("v", v), ("k_lens", k_lens)):
        rec.update(_tensor_record(n, t))
    if table is not None:
        assert table.dtype == torch.int32
        rec.update(_tensor_record("table", table))
    rec["k_scale"], rec["v_scale"] = _scale_record(k_scale, Hkv), _scale_record(v_scale, Hkv)
    calls.append((name, rec))
    raw = torch.int16 if k.dtype == k_new.dtype else torch.uint8
    page = k.shape[2]
    smax = page if table is None else table.shape[1] * page
    lens = k_lens.reshape(-1).expand(B).tolist()
    for b in range(B):
        for t in range(T):
            pos = lens[b] - T + t
            if not 0 <= pos < smax:
                continue
            outer, row = b, pos
            if table is not None:
                outer, row = int(table[b, pos // page]), pos % page
                if not 0 <= outer < k.shape[0]:
                    continue
            k.view(raw)[outer, :, row] = _converted(k_new[b, :, t], k.dtype, k_scale)
            v.view(raw)[outer, :, row] = _converted(v_new[b, :, t], v.dtype, v_scale)


def kv_append(k_new, v_new, k, v, k_lens, k_scale, v_scale):
    _append("kv_append", k_new, v_new, k, v, None, k_lens, k_scale, v_scale)


def kv_append_paged(k_new, v_new, k_pages, v_pages, block_table, k_lens, k_scale, v_scale):
    _append("kv_append_paged", k_new, v_new, k_pages, v_pages, block_table, k_lens, k_scale, v_scale)
