"""fake_custom_mm_fused_attention plus the two block attention entries — TEST ONLY.

Re-exports tests/fake_custom_mm_fused_attention.py and adds float64 numpy forms of custom_mm.block_attention_forward /
block_attention_backward with the real entries' argument lists, so that the wiring of matmuls.blockSparseAttention (what
is saved, the expanded and the transposed block lists, which layout an item uses) can be checked on CPU tensors against
torch autograd of the dense masked attention.  The backward takes dq from the forward lists and dk, dv from the TRANSPOSED
lists alone, as the kernels do.  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_fused_attention import *  # noqa: F401,F403
from fake_custom_mm_fused_attention import _np, calls  # noqa: F401

TILE = 64


def _masks(offsets, columns, rows, cols, causal, transposed=False):
    """Boolean [layouts, rows·64, cols·64] masks of block lists (offsets [layouts, rows + 1] with the layouts' bases)."""
    off = _np(offsets).astype(np.int64).reshape(-1, rows + 1)
    col = _np(columns).astype(np.int64)
    out = np.zeros((off.shape[0], rows * TILE, cols * TILE), bool)
    for lay, o in enumerate(off):
        for r in range(rows):
            for c in col[o[r]:o[r + 1]]:
                assert 0 <= c < cols
                assert not out[lay, r * TILE, c * TILE], "a block stored twice"
                out[lay, r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE] = True
    if causal:
        i, j = np.arange(rows * TILE)[:, None], np.arange(cols * TILE)[None, :]
        out &= (i <= j) if transposed else (j <= i)
    return out


def _check(offsets, columns, nnz, q, k):
    assert offsets.dtype == torch.int32 and columns.dtype == torch.int32 and columns.numel() == nnz
    assert q.dim() == 3 and k.dim() == 3 and q.shape[1] % TILE == 0 and k.shape[1] % TILE == 0
    assert offsets.dim() == 2 and offsets.shape[1] == q.shape[1] // TILE + 1
    assert int(offsets[-1, -1]) == nnz


def block_attention_forward(offsets, columns, nnz, q, k, v, scale, causal, out, lse):
    calls.append(("block_attention_forward", (tuple(q.shape), tuple(k.shape), offsets.shape[0], nnz, causal)))
    _check(offsets, columns, nnz, q, k)
    assert lse.shape == q.shape[:2] and lse.dtype == torch.float32 and out.shape == q.shape
    masks = _masks(offsets, columns, q.shape[1] // TILE, k.shape[1] // TILE, causal)
    qn, kn, vn = (_np(t).astype(np.float64) for t in (q, k, v))
    res, ls = np.zeros(qn.shape), np.full(qn.shape[:2], -np.inf)
    for i in range(qn.shape[0]):
        mask = masks[i % len(masks)]
        s = np.where(mask, float(scale) * (qn[i] @ kn[i].T), -np.inf)
        seen = mask.any(1)
        m = s[seen].max(1, keepdims=True)
        e = np.exp(s[seen] - m)
        res[i][seen] = (e / e.sum(1, keepdims=True)) @ vn[i]
        ls[i][seen] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
    out.copy_(torch.from_numpy(res).to(out.dtype))
    lse.copy_(torch.from_numpy(ls).to(lse.dtype))
    return out


def block_attention_backward(offsets, columns, t_offsets, t_columns, nnz, q, k, v, out, dout, lse, scale, causal, dq, dk, dv):
    calls.append(("block_attention_backward", (tuple(q.shape), tuple(k.shape), offsets.shape[0], nnz, causal)))
    _check(offsets, columns, nnz, q, k)
    _check(t_offsets, t_columns, nnz, k, q)
    assert t_offsets.shape[0] == offsets.shape[0]
    rows, cols = q.shape[1] // TILE, k.shape[1] // TILE
    masks = _masks(offsets, columns, rows, cols, causal)
    t_masks = _masks(t_offsets, t_columns, cols, rows, causal, transposed=True)
    qn, kn, vn, on, gn = (_np(t).astype(np.float64) for t in (q, k, v, out, dout))
    ls = _np(lse).astype(np.float64)
    rq, rk, rv = np.zeros(qn.shape), np.zeros(kn.shape), np.zeros(vn.shape)
    for i in range(qn.shape[0]):
        s = float(scale) * (qn[i] @ kn[i].T)
        with np.errstate(over="ignore", invalid="ignore"):
            p_all = np.where(np.isinf(ls[i])[:, None], 0.0, np.exp(s - ls[i][:, None]))
        delta = (gn[i] * on[i]).sum(1, keepdims=True)
        ds_all = p_all * (gn[i] @ vn[i].T - delta)
        mask, t_mask = masks[i % len(masks)], t_masks[i % len(masks)].T
        rq[i] = float(scale) * (np.where(mask, ds_all, 0.0) @ kn[i])
        rk[i] = float(scale) * (np.where(t_mask, ds_all, 0.0).T @ qn[i])
        rv[i] = np.where(t_mask, p_all, 0.0).T @ gn[i]
    for t, r in ((dq, rq), (dk, rk), (dv, rv)):
        t.copy_(torch.from_numpy(r).to(t.dtype))
    return dq, dk, dv
