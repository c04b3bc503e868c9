"""fake_custom_mm_block_attention plus the two grouped / lengths entries — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention.py and adds float64 numpy forms of custom_mm.block_attention_forward_ex /
block_attention_backward_ex with the real entries' argument lists: k and v carry one item per `group` query items (query
item i reads item i // group), q_lens / k_lens are None or contiguous int32 tensors of one count (query item i reads entry
i // (batch / count)), clamped to [0, S] as the kernels clamp them.  dk and dv are the group's sums.  Every call is recorded
in `calls` under its own name, so a test sees WHICH binding matmuls chose.  A plain Python module: matmuls takes it for
the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_attention import *  # noqa: F401,F403
from fake_custom_mm_block_attention import TILE, _check, _masks, _np, calls  # noqa: F401


def _lens(t, name, batch, group, rows):
    """Per query item lengths [batch] of a lens argument (None: `rows` everywhere), after the checks the binding makes."""
    if t is None:
        return np.full(batch, rows, np.int64)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous(), name
    n = t.numel()
    assert n > 0 and batch % n == 0 and (batch // n) % group == 0, (name, n, batch, group)
    return np.clip(_np(t).astype(np.int64), 0, rows).repeat(batch // n)


def _item_masks(offsets, columns, q, k, causal, q_lens, k_lens, group, transposed=False):
    """Per query item the boolean [Sq, Sk] mask: its layout's blocks (from the lists, or from the TRANSPOSED lists), causal,
    and the positions that exist."""
    batch, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    if transposed:
        masks = _masks(offsets, columns, Sk // TILE, Sq // TILE, causal, transposed=True).transpose(0, 2, 1)
    else:
        masks = _masks(offsets, columns, Sq // TILE, Sk // TILE, causal)
    ql, kl = _lens(q_lens, "q_lens", batch, group, Sq), _lens(k_lens, "k_lens", batch, group, Sk)
    i, j = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
    return [masks[b % len(masks)] & (i < ql[b]) & (j < kl[b]) for b in range(batch)]


def _group(q, k):
    assert q.dim() == 3 and k.dim() == 3 and k.shape[0] > 0 and q.shape[0] % k.shape[0] == 0
    return q.shape[0] // k.shape[0]


def _clean(x, rows_alive):
    """x [rows, D] in float64 with the rows that do not exist zeroed (their NaN must not reach a product)."""
    x = _np(x).astype(np.float64).copy()
    x[~rows_alive] = 0.0
    return x


def block_attention_forward_ex(offsets, columns, nnz, q, k, v, scale, causal, out, lse, q_lens, k_lens):
    group = _group(q, k)
    calls.append(("block_attention_forward_ex", (tuple(q.shape), tuple(k.shape), offsets.shape[0], nnz, causal, group,
                                                 None if q_lens is None else q_lens.clone(),
                                                 None if k_lens is None else k_lens.clone())))
    _check(offsets, columns, nnz, q, k)
    assert v.shape == k.shape and lse.shape == q.shape[:2] and lse.dtype == torch.float32 and out.shape == q.shape
    masks = _item_masks(offsets, columns, q, k, causal, q_lens, k_lens, group)
    res, ls = np.zeros(tuple(q.shape)), np.full(tuple(q.shape[:2]), -np.inf)
    for i, mask in enumerate(masks):
        qn, kn, vn = _clean(q[i], mask.any(1)), _clean(k[i // group], mask.any(0)), _clean(v[i // group], mask.any(0))
        s = np.where(mask, float(scale) * (qn @ kn.T), -np.inf)
        seen = mask.any(1)
        if seen.any():
            m = s[seen].max(1, keepdims=True)
            e = np.exp(s[seen] - m)
            res[i][seen] = (e / e.sum(1, keepdims=True)) @ vn
            ls[i][seen] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
    out.copy_(torch.from_numpy(res).to(out.dtype))
    lse.copy_(torch.from_numpy(ls).to(lse.dtype))
    return out


def block_attention_backward_ex(offsets, columns, t_offsets, t_columns, nnz, q, k, v, out, dout, lse, scale, causal, dq, dk, dv,
                                q_lens, k_lens):
    group = _group(q, k)
    calls.append(("block_attention_backward_ex", (tuple(q.shape), tuple(k.shape), offsets.shape[0], nnz, causal, group,
                                                  None if q_lens is None else q_lens.clone(),
                                                  None if k_lens is None else k_lens.clone())))
    _check(offsets, columns, nnz, q, k)
    _check(t_offsets, t_columns, nnz, k, q)
    assert t_offsets.shape[0] == offsets.shape[0] and dk.shape == k.shape and dv.shape == k.shape and dq.shape == q.shape
    masks = _item_masks(offsets, columns, q, k, causal, q_lens, k_lens, group)
    # dk, dv from the TRANSPOSED lists alone, as the kernels take them
    t_masks = _item_masks(t_offsets, t_columns, q, k, causal, q_lens, k_lens, group, transposed=True)
    rq, rk, rv = np.zeros(tuple(q.shape)), np.zeros(tuple(k.shape)), np.zeros(tuple(v.shape))
    ls = _np(lse).astype(np.float64)
    for i, mask in enumerate(masks):
        rows, cols = mask.any(1), mask.any(0)
        qn, gn, on = _clean(q[i], rows), _clean(dout[i], rows), _clean(out[i], rows)
        kn, vn = _clean(k[i // group], cols), _clean(v[i // group], cols)
        s = float(scale) * (qn @ kn.T)
        with np.errstate(over="ignore", invalid="ignore"):
            p_all = np.where(np.isinf(ls[i])[:, None] | ~(rows[:, None] & cols[None, :]), 0.0, np.exp(s - ls[i][:, None]))
        delta = (gn * on).sum(1, keepdims=True)
        ds_all = p_all * (gn @ vn.T - delta)
        t_mask = t_masks[i]
        rq[i] = float(scale) * (np.where(mask, ds_all, 0.0) @ kn)
        rk[i // group] += float(scale) * (np.where(t_mask, ds_all, 0.0).T @ qn)
        rv[i // group] += np.where(t_mask, p_all, 0.0).T @ gn
    for t, r in ((dq, rq), (dk, rk), (dv, rv)):
        t.copy_(torch.from_numpy(r).to(t.dtype))
    return dq, dk, dv
