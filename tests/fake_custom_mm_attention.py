"""fake_custom_mm plus what sparse attention needs — TEST ONLY.

Re-exports tests/fake_custom_mm.py (the oracle behind the custom_mm names) and adds numpy forms of the CSR row softmax and
its backward; the CSR products and sampled products are replaced by forms that compute in float64 whatever the operands'
dtype (the oracle is float32), so that the autograd formulas of matmuls.sparseSoftmax / sampledMM / sparse_attention can
be checked against torch autograd in float64.  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm import *  # noqa: F401,F403
from fake_custom_mm import _np, _write, calls  # noqa: F401


def _rows_of(offs, batch, rows):
    """(start, end) of every row, in order, of offsets [batch, rows + 1] with the items' bases."""
    o = _np(offs).reshape(batch, rows + 1).astype(np.int64)
    return o[:, :-1].reshape(-1), o[:, 1:].reshape(-1)


def csr_softmax(values, offsets, nnz, batch, rows, scale, out):
    calls.append(("csr_softmax", (batch, rows)))
    assert offsets.dtype == torch.int32 and offsets.numel() == batch * (rows + 1) and values.dtype == out.dtype
    x = _np(values).astype(np.float64) * float(scale)
    y = np.zeros_like(x)
    for s, e in zip(*_rows_of(offsets, batch, rows)):
        if e > s:
            ex = np.exp(x[s:e] - x[s:e].max())
            y[s:e] = ex / ex.sum()
    out.copy_(torch.from_numpy(y).to(out.dtype))
    return out


def csr_softmax_backward(y, dy, offsets, nnz, batch, rows, scale, out):
    calls.append(("csr_softmax_backward", (batch, rows)))
    assert offsets.dtype == torch.int32 and offsets.numel() == batch * (rows + 1) and y.dtype == dy.dtype == out.dtype
    yv, gv = _np(y).astype(np.float64), _np(dy).astype(np.float64)
    dx = np.zeros_like(yv)
    for s, e in zip(*_rows_of(offsets, batch, rows)):
        dx[s:e] = float(scale) * yv[s:e] * (gv[s:e] - np.dot(gv[s:e], yv[s:e]))
    out.copy_(torch.from_numpy(dx).to(out.dtype))
    return out


def _entry_rows(offs, rows):
    o = _np(offs).astype(np.int64)
    return np.repeat(np.arange(rows), np.diff(o)), int(o[0]), int(o[-1])


def _spmm64(vals, cols, offs, rows, kcols, B):
    r, s0, s1 = _entry_rows(offs, rows)
    out = np.zeros((rows, B.shape[1]), np.float64)
    np.add.at(out, r, _np(vals).astype(np.float64)[s0:s1, None] * B[_np(cols).astype(np.int64)[s0:s1]])
    return out


def naive_spmm(vals, cols, offs, nnz, rows, kcols, B, C):
    calls.append(("naive_spmm", (rows, kcols)))
    return _write(C, _spmm64(vals, cols, offs, rows, kcols, _np(B).astype(np.float64)))


def naive_spmm_ex(vals, cols, offs, nnz, rows, kcols, B, C, long_rows):
    calls.append(("naive_spmm_ex", (rows, kcols)))
    return _write(C, _spmm64(vals, cols, offs, rows, kcols, _np(B).astype(np.float64)))


def naive_spmm_batched(vals, cols, offs, nnz, batch, rows, kcols, B, C):
    calls.append(("naive_spmm_batched", (batch, rows, kcols)))
    o, Bn = offs.reshape(batch, rows + 1), _np(B).astype(np.float64)
    res = np.stack([_spmm64(vals, cols, o[i], rows, kcols, Bn if Bn.ndim == 2 else Bn[i]) for i in range(batch)])
    return _write(C, res)


def _sddmm64(cols, offs, rows, dC, B):
    r, s0, s1 = _entry_rows(offs, rows)
    return s0, s1, np.einsum("ij,ij->i", dC[r], B[_np(cols).astype(np.int64)[s0:s1]])


def sddmm(cols, offs, nnz, rows, kcols, dC, B):
    calls.append(("sddmm", (rows, kcols)))
    return torch.from_numpy(_sddmm64(cols, offs, rows, _np(dC).astype(np.float64), _np(B).astype(np.float64))[2]).to(dC.dtype)


def sddmm_batched(cols, offs, nnz, batch, rows, kcols, dC, B, out):
    import fake_custom_mm
    calls.append(("sddmm_batched", (batch, rows, kcols)))
    if not fake_custom_mm.batched_sddmm:
        return False
    o, g, b = offs.reshape(batch, rows + 1), _np(dC).astype(np.float64), _np(B).astype(np.float64)
    for i in range(batch):
        s0, s1, v = _sddmm64(cols, o[i], rows, g[i], b if b.ndim == 2 else b[i])
        out[s0:s1] = torch.from_numpy(v).to(out.dtype)
    return True
