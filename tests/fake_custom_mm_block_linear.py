"""fake_custom_mm_block_mm plus the block-sparse linear entries — TEST ONLY.

Re-exports tests/fake_custom_mm_block_mm.py and adds float64 numpy forms of custom_mm.bsr_linear / bsr_wgrad /
bsr_wgrad_split_count with the real entries' argument lists, so that the wiring of matmuls.blockSparseLinearFn (the
sorted lists and their entry ids, the transposed lists, the entry rows, the bias, what is saved and what is computed)
can be checked on CPU tensors against torch autograd of x @ W_dense.T + bias.  bsr_linear uses the lists it is handed and
nothing else, as the kernels do: with trans_w the TRANSPOSED lists, every block transposed.  column_sums takes the
low-precision dtypes here.  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_mm import *  # noqa: F401,F403
from fake_custom_mm_block_mm import _ids, _np, calls  # noqa: F401

TILE = 64


def bsr_linear(offsets, columns, entry_ids, nnz, values, X, bias, Y, trans_w):
    calls.append(("bsr_linear", (tuple(X.shape), tuple(Y.shape), nnz, bias is not None, bool(trans_w))))
    assert offsets.dtype == torch.int32 and columns.dtype == torch.int32 and columns.numel() == nnz
    assert entry_ids is None or (entry_ids.dtype == torch.int32 and entry_ids.numel() == nnz)
    assert values.dim() == 3 and values.shape[1:] == (TILE, TILE) and values.is_contiguous()
    assert X.dim() == 2 and Y.dim() == 2 and X.shape[0] == Y.shape[0] and X.dtype == Y.dtype == values.dtype
    own, inner = Y.shape[1] // TILE, X.shape[1] // TILE
    assert Y.shape[1] % TILE == 0 and X.shape[1] % TILE == 0 and offsets.numel() == own + 1 and int(offsets[-1]) == nnz
    assert bias is None or (bias.dtype == Y.dtype and tuple(bias.shape) == (Y.shape[1],))
    off, col, ids = _np(offsets).astype(np.int64), _np(columns).astype(np.int64), _ids(entry_ids, nnz)
    v, x = _np(values.double()), _np(X.double())
    out = np.zeros(tuple(Y.shape))
    for r in range(own):
        lst = col[off[r]:off[r + 1]]
        assert (np.diff(lst) > 0).all(), "every list is handed over in ascending order, no block twice"
        for p in range(off[r], off[r + 1]):
            assert 0 <= col[p] < inner and 0 <= ids[p] < values.shape[0]
            blk = v[ids[p]].T if trans_w else v[ids[p]]  # Wblk(c, k)
            out[:, r * TILE:(r + 1) * TILE] += x[:, col[p] * TILE:(col[p] + 1) * TILE] @ blk.T
    if bias is not None:
        out += _np(bias.double())
    Y.copy_(torch.from_numpy(out).to(Y.dtype))
    return Y


def bsr_wgrad_split_count(nnz, tokens):
    if nnz <= 0 or tokens < 2048:
        return 1
    cap = min(1024 // nnz, tokens // 512, 32)
    s = 1
    while 2 * s <= cap:
        s *= 2
    while s > 1 and tokens % (32 * s):
        s //= 2
    return s


def bsr_wgrad(entry_row, columns, entry_ids, nnz, dY, X, dvalues, splits=0):
    calls.append(("bsr_wgrad", (tuple(dY.shape), tuple(X.shape), nnz, splits)))
    assert entry_row.dtype == torch.int32 and columns.dtype == torch.int32
    assert entry_row.numel() == nnz and columns.numel() == nnz
    assert dY.dim() == 2 and X.dim() == 2 and dY.shape[0] == X.shape[0]
    assert dvalues.dim() == 3 and dvalues.shape[1:] == (TILE, TILE) and dvalues.is_contiguous()
    row, col, ids = _np(entry_row).astype(np.int64), _np(columns).astype(np.int64), _ids(entry_ids, nnz)
    assert sorted(ids.tolist()) == list(range(dvalues.shape[0])), "every block of the gradient is written once"
    g, x = _np(dY.double()), _np(X.double())
    out = np.zeros(tuple(dvalues.shape))
    for p in range(nnz):
        out[ids[p]] = g[:, row[p] * TILE:(row[p] + 1) * TILE].T @ x[:, col[p] * TILE:(col[p] + 1) * TILE]
    dvalues.copy_(torch.from_numpy(out).to(dvalues.dtype))
    return dvalues


def column_sums(src):
    calls.append(("column_sums", tuple(src.shape)))
    return src.double().sum(dim=0).to(src.dtype)
