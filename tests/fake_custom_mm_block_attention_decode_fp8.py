"""fake_custom_mm_block_attention_decode_paged plus the two fp8 decode entries — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention_decode_paged.py and adds float64 forms of
custom_mm.block_attention_decode_fp8 (offsets, columns, nnz, q, k, v, k_lens, scale, k_scale, v_scale, chunk, out, lse) and
custom_mm.block_attention_decode_paged_fp8 (offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, scale, k_scale,
v_scale, chunk, out, lse) with the real entries' argument lists.  The cache arrives as float8_e4m3fn AS IT IS: the call is
recorded with its data_ptr, strides and dtype and with the scales as they were handed over (None, or a contiguous float32
tensor of 1 or Hkv entries: its data_ptr and a clone), so a test sees that nothing was copied or read back.  The arithmetic
is the stand-in's of the 2-byte entries on the dequantised cache k8 · k_scale[h], v8 · v_scale[h] in float64; what those
never touch (unseen keys, unreferenced pages) is never touched here either.  A plain Python module.
"""
import torch

import fake_custom_mm_block_attention_decode_paged as _base
from fake_custom_mm_block_attention_decode_paged import *  # noqa: F401,F403
from fake_custom_mm_block_attention_decode_paged import TILE, calls  # noqa: F401


def _scale_record(s, Hkv):
    if s is None:
        return None
    assert isinstance(s, torch.Tensor) and s.dtype == torch.float32 and s.is_contiguous() and s.dim() <= 1
    assert s.numel() in (1, Hkv)
    return {"ptr": s.data_ptr(), "shape": tuple(s.shape), "value": s.clone()}


def _dequantised(x8, s, Hkv):
    """float64 x8 · s[h] with the heads in dim 1; NaN bytes stay NaN where they are."""
    assert x8.dtype == torch.float8_e4m3fn and x8.stride(3) == 1 and x8.data_ptr() % 16 == 0
    assert all(st % 16 == 0 for n, st in zip(x8.shape[:3], x8.stride()[:3]) if n > 1)
    x = x8.to(torch.float32).double()
    if s is None:
        return x
    return x * s.double().reshape(-1).expand(Hkv).reshape(1, Hkv, 1, 1)


def _record(name, q, k, v, k_lens, scale, k_scale, v_scale, chunk, offsets, nnz, **more):
    Hkv = k.shape[1]
    calls.append((name, {
        "q": tuple(q.shape), "k": tuple(k.shape), "layouts": offsets.shape[0], "nnz": nnz, "chunk": chunk, "scale": scale,
        "k_ptr": k.data_ptr(), "k_stride": tuple(k.stride()), "k_dtype": k.dtype, "v_ptr": v.data_ptr(),
        "v_stride": tuple(v.stride()), "v_dtype": v.dtype, "k_scale": _scale_record(k_scale, Hkv),
        "v_scale": _scale_record(v_scale, Hkv), "k_lens": k_lens.clone(), "offsets_ptr": offsets.data_ptr(), **more}))


def block_attention_decode_fp8(offsets, columns, nnz, q, k, v, k_lens, scale, k_scale, v_scale, chunk, out, lse):
    _record("block_attention_decode_fp8", q, k, v, k_lens, scale, k_scale, v_scale, chunk, offsets, nnz)
    Hkv = k.shape[1]
    _base.block_attention_decode(offsets, columns, nnz, q, _dequantised(k, k_scale, Hkv), _dequantised(v, v_scale, Hkv), k_lens,
                                 scale, chunk, out, lse)
    calls.pop()  # (the 2-byte stand-in's own record of the inner call)
    return out


def block_attention_decode_paged_fp8(offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, scale, k_scale, v_scale,
                                     chunk, out, lse):
    _record("block_attention_decode_paged_fp8", q, k_pages, v_pages, k_lens, scale, k_scale, v_scale, chunk, offsets, nnz,
            table_ptr=block_table.data_ptr(), table_stride=tuple(block_table.stride()), table_dtype=block_table.dtype,
            table_shape=tuple(block_table.shape))
    Hkv = k_pages.shape[1]
    _base.block_attention_decode_paged(offsets, columns, nnz, q, _dequantised(k_pages, k_scale, Hkv),
                                       _dequantised(v_pages, v_scale, Hkv), block_table, k_lens, scale, chunk, out, lse)
    calls.pop()
    return out
