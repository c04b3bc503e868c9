"""fake_custom_mm_block_select plus the four entries of the selection over an fp8 cache — TEST ONLY.

Re-exports tests/fake_custom_mm_block_select.py and tests/fake_custom_mm_block_attention_decode_fp8.py (both stand on the
paged stand-in and share its `calls`) and adds custom_mm.kv_block_bounds_fp8, kv_block_bounds_paged_fp8,
block_attention_lists_decode_fp8 and block_attention_lists_decode_paged_fp8 with the real entries' argument lists.  The
cache arrives as float8_e4m3fn AS IT IS: every call is recorded with the data_ptr, strides and dtype of the operands as they
arrive and with the scales as they were handed over, so a test sees that nothing was copied or read back.  The arithmetic
is the 2-byte stand-ins' on the widened (bounds) or dequantised (decode) cache.  A plain Python module.
"""
import torch

import fake_custom_mm_block_select as _sel
from fake_custom_mm_block_select import *  # noqa: F401,F403
from fake_custom_mm_block_attention_decode_fp8 import *  # noqa: F401,F403
from fake_custom_mm_block_attention_decode_fp8 import _dequantised, _scale_record
from fake_custom_mm_block_select import TILE, calls  # noqa: F401


def _fp8_cache(x):
    assert x.dtype == torch.float8_e4m3fn and x.dim() == 4 and x.stride(3) == 1 and x.data_ptr() % 16 == 0
    assert all(st % 16 == 0 for n, st in zip(x.shape[:3], x.stride()[:3]) if n > 1)


def _bounds_fp8(name, k, table, k_lens, last, bounds):
    _fp8_cache(k)
    assert bounds.dtype in (torch.bfloat16, torch.float16)
    wide = torch.empty(k.shape, dtype=bounds.dtype)  # (contiguous: the 2-byte stand-in asks for strides of 8 elements)
    wide.copy_(k.to(torch.float32))
    _sel._bounds(name, wide, table, k_lens, last, bounds)
    record = calls.pop()[1]  # the 2-byte stand-in's record of the inner call, with the cache as it arrived here
    record.update(k_ptr=k.data_ptr(), k_stride=tuple(k.stride()), k_dtype=k.dtype, bounds_dtype=bounds.dtype)
    calls.append((name, record))


def kv_block_bounds_fp8(k, k_lens, last, bounds):
    _bounds_fp8("kv_block_bounds_fp8", k, None, k_lens, last, bounds)


def kv_block_bounds_paged_fp8(k_pages, block_table, k_lens, last, bounds):
    _bounds_fp8("kv_block_bounds_paged_fp8", k_pages, block_table, k_lens, last, bounds)


def _lists_fp8(name, block_ids, block_counts, q, k, v, table, k_lens, scale, k_scale, v_scale, chunk, out, lse):
    _fp8_cache(k)
    _fp8_cache(v)
    Hkv = k.shape[1]
    kd, vd = (torch.empty(x.shape, dtype=torch.float64).copy_(_dequantised(x, s, Hkv)) for x, s in ((k, k_scale), (v, v_scale)))
    _sel._lists(name, block_ids, block_counts, q, kd, vd, table, k_lens, scale, chunk, out, lse)
    record = calls.pop()[1]
    record.update(k_ptr=k.data_ptr(), k_stride=tuple(k.stride()), k_dtype=k.dtype, v_ptr=v.data_ptr(), v_stride=tuple(v.stride()),
                  v_dtype=v.dtype, k_scale=_scale_record(k_scale, Hkv), v_scale=_scale_record(v_scale, Hkv))
    calls.append((name, record))
    return out


def block_attention_lists_decode_fp8(block_ids, block_counts, q, k, v, k_lens, scale, k_scale, v_scale, chunk, out, lse):
    return _lists_fp8("block_attention_lists_decode_fp8", block_ids, block_counts, q, k, v, None, k_lens, scale, k_scale, v_scale,
                      chunk, out, lse)


def block_attention_lists_decode_paged_fp8(block_ids, block_counts, q, k_pages, v_pages, block_table, k_lens, scale, k_scale,
                                           v_scale, chunk, out, lse):
    return _lists_fp8("block_attention_lists_decode_paged_fp8", block_ids, block_counts, q, k_pages, v_pages, block_table, k_lens,
                      scale, k_scale, v_scale, chunk, out, lse)
