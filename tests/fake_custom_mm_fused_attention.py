"""fake_custom_mm_attention plus the two fused attention entries — TEST ONLY.

Re-exports tests/fake_custom_mm_attention.py and adds float64 numpy forms of custom_mm.sparse_attention_fwd /
sparse_attention_bwd with the real entries' argument lists, so that the wiring of matmuls.fusedSparseAttention (what is
saved, which array goes to which product, the transposed patterns) can be checked against torch autograd in float64.  A
plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_attention import *  # noqa: F401,F403
from fake_custom_mm_attention import _np, _rows_of, calls  # noqa: F401


def _rows(offsets, columns, batch, rows):
    """(global row, item, start, end, columns of the row) for every row with entries."""
    starts, ends = _rows_of(offsets, batch, rows)
    col = _np(columns).astype(np.int64)
    for g, (s, e) in enumerate(zip(starts, ends)):
        if e > s:
            yield g, g // rows, g % rows, int(s), int(e), col[s:e]


def _probabilities(qrow, kitem, c, scale):
    t = float(scale) * (kitem[c] @ qrow)
    m = t.max()
    e = np.exp(t - m)
    return e / e.sum(), m, 1.0 / e.sum()


def sparse_attention_fwd(offsets, columns, nnz, batch, rows, cols, q, k, v, scale, out, stats):
    calls.append(("sparse_attention_fwd", (batch, rows, cols)))
    assert offsets.dtype == torch.int32 and offsets.numel() == batch * (rows + 1) and columns.dtype == torch.int32
    assert q.shape == out.shape == (batch, rows, q.shape[-1]) and k.shape == v.shape == (batch, cols, q.shape[-1])
    assert stats.shape == (batch * rows, 2) and stats.dtype == torch.float32
    qn, kn, vn = (_np(t).astype(np.float64) for t in (q, k, v))
    res, st = np.zeros(qn.shape), np.zeros((batch * rows, 2))
    for g, i, r, s, e, c in _rows(offsets, columns, batch, rows):
        y, m, inv = _probabilities(qn[i, r], kn[i], c, scale)
        res[i, r] = y @ vn[i][c]
        st[g] = (m, inv)
    out.copy_(torch.from_numpy(res).to(out.dtype))
    stats.copy_(torch.from_numpy(st).to(stats.dtype))
    return out


def sparse_attention_bwd(offsets, columns, nnz, batch, rows, cols, q, k, v, dout, stats, scale, dq, y, ds):
    calls.append(("sparse_attention_bwd", (batch, rows, cols)))
    assert offsets.dtype == torch.int32 and columns.dtype == torch.int32 and stats.shape == (batch * rows, 2)
    assert y.numel() == ds.numel() == nnz and q.dtype == dout.dtype == dq.dtype == y.dtype == ds.dtype
    qn, kn, vn, gn = (_np(t).astype(np.float64) for t in (q, k, v, dout))
    res, yn, dsn = np.zeros(qn.shape), np.zeros(nnz), np.zeros(nnz)
    for g, i, r, s, e, c in _rows(offsets, columns, batch, rows):
        p = _probabilities(qn[i, r], kn[i], c, scale)[0]  # (float32 stats would cost the float64 check its tolerance)
        dp = vn[i][c] @ gn[i, r]
        d = float(scale) * p * (dp - np.dot(dp, p))
        yn[s:e], dsn[s:e] = p, d
        res[i, r] = d @ kn[i][c]
    dq.copy_(torch.from_numpy(res).to(dq.dtype))
    y.copy_(torch.from_numpy(yn).to(y.dtype))
    ds.copy_(torch.from_numpy(dsn).to(ds.dtype))
    return dq
