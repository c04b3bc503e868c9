"""Shared by tests/test_gpu_block_attention_gqa.py: the mi_block_attention_{fwd,bwd}_ex_T entries of the C ABI through
ctypes on gpu_helpers.Padded operands (a leading dimension and an item stride of their own), and the masks, poison and
references of the grouped / lengths cases."""
import ctypes

import torch

_SUFFIX = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _ex_entry(capi, name):
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    dense, ex = [vp, i64, i64], [i32, vp, vp, i32, vp]
    fn = getattr(capi, name)
    if "_fwd_" in name:
        fn.argtypes = [vp, vp, i64] + 6 * [i32] + 3 * dense + [f32] + dense + [vp] + ex
    else:
        fn.argtypes = [vp, vp, vp, vp, i64] + 6 * [i32] + 5 * dense + [vp, f32] + 3 * dense + [vp, sz] + ex
    fn.restype = ctypes.c_int
    return fn


def _ptr(t):
    return None if t is None else t.data_ptr()


def fwd_ex_through_the_c_abi(capi, dtype, offsets, columns, nnz, layouts, batch, Sq, Sk, D, causal, q, k, v, scale, out, lse, group,
                             q_lens, k_lens, lens_count):
    """mi_block_attention_fwd_ex_T on Padded operands; returns the status."""
    fn = _ex_entry(capi, f"mi_block_attention_fwd_ex_{_SUFFIX[dtype]}")
    return fn(offsets.data_ptr(), columns.data_ptr(), nnz, layouts, batch, Sq, Sk, D, causal, *q.args(), *k.args(), *v.args(), scale,
              *out.args(), lse.data_ptr(), group, _ptr(q_lens), _ptr(k_lens), lens_count, torch.cuda.current_stream().cuda_stream)


def bwd_ex_through_the_c_abi(capi, dtype, offsets, columns, t_offsets, t_columns, nnz, layouts, batch, Sq, Sk, D, causal, q, k, v,
                             out, dout, lse, scale, dq, dk, dv, group, q_lens, k_lens, lens_count):
    """mi_block_attention_bwd_ex_T on Padded operands, with a workspace of mi_block_attention_workspace_bytes (query
    items); returns the status."""
    fn = _ex_entry(capi, f"mi_block_attention_bwd_ex_{_SUFFIX[dtype]}")
    capi.mi_block_attention_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
    capi.mi_block_attention_workspace_bytes.restype = ctypes.c_size_t
    ws_bytes = capi.mi_block_attention_workspace_bytes(batch, Sq)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=lse.device)
    return fn(offsets.data_ptr(), columns.data_ptr(), t_offsets.data_ptr(), t_columns.data_ptr(), nnz, layouts, batch, Sq, Sk, D,
              causal, *q.args(), *k.args(), *v.args(), *out.args(), *dout.args(), lse.data_ptr(), scale, *dq.args(), *dk.args(),
              *dv.args(), ws.data_ptr(), ws_bytes, group, _ptr(q_lens), _ptr(k_lens), lens_count,
              torch.cuda.current_stream().cuda_stream)


def length_mask(mask, q_lens, k_lens):
    """mask [B, …, Sq, Sk] (CPU, bool) and-ed with i < q_lens[b] and j < k_lens[b] (lists of B lengths or None)."""
    Sq, Sk = mask.shape[-2:]
    m = mask.clone()
    for b in range(m.shape[0]):
        if q_lens is not None:
            m[b, ..., max(min(q_lens[b], Sq), 0):, :] = False
        if k_lens is not None:
            m[b, ..., :, max(min(k_lens[b], Sk), 0):] = False
    return m


def fill_padding(x, lens, value):
    """A copy of x [B, …, S, D] with the rows at or beyond lens[b] of item b set to `value` (lens None: x itself)."""
    if lens is None:
        return x
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, ..., max(min(n, x.shape[-2]), 0):, :] = value
    return x
