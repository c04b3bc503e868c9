"""fake_custom_mm_block_attention plus the two block product entries — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention.py and adds float64 numpy forms of custom_mm.bsr_mm / bsr_sddmm with the
real entries' argument lists, so that the wiring of matmuls.blockSparseMM (the sorted lists and their entry ids, the
transposed lists, the entry rows, what is saved) can be checked on CPU tensors against torch autograd of A_dense @ b.
bsr_mm uses the lists it is handed and nothing else, as the kernels do: with trans_a the TRANSPOSED lists, every block
transposed.  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_attention import *  # noqa: F401,F403
from fake_custom_mm_block_attention import _np, calls  # noqa: F401

TILE = 64


def _ids(entry_ids, nnz):
    return np.arange(nnz) if entry_ids is None else _np(entry_ids).astype(np.int64)[:nnz]


def bsr_mm(offsets, columns, entry_ids, nnz, values, B, C, trans_a):
    calls.append(("bsr_mm", (tuple(B.shape), tuple(C.shape), nnz, bool(trans_a))))
    assert offsets.dtype == torch.int32 and columns.dtype == torch.int32 and columns.numel() == nnz
    assert entry_ids is None or (entry_ids.dtype == torch.int32 and entry_ids.numel() == nnz)
    assert values.dim() == 3 and values.shape[1:] == (TILE, TILE) and values.is_contiguous()
    assert B.dim() == 3 and C.dim() == 3 and B.shape[0] == C.shape[0] and B.shape[2] == C.shape[2]
    rows, inner = C.shape[1] // TILE, B.shape[1] // TILE
    assert C.shape[1] % TILE == 0 and B.shape[1] % TILE == 0 and offsets.numel() == rows + 1 and int(offsets[-1]) == nnz
    off, col, ids = _np(offsets).astype(np.int64), _np(columns).astype(np.int64), _ids(entry_ids, nnz)
    v = _np(values.double())
    b = _np(B.double())
    out = np.zeros(tuple(C.shape))
    for r in range(rows):
        lst = col[off[r]:off[r + 1]]
        assert (np.diff(lst) > 0).all(), "every list is handed over in ascending order, no block twice"
        for p in range(off[r], off[r + 1]):
            assert 0 <= col[p] < inner and 0 <= ids[p] < values.shape[0]
            blk = v[ids[p]].T if trans_a else v[ids[p]]
            out[:, r * TILE:(r + 1) * TILE] += blk @ b[:, col[p] * TILE:(col[p] + 1) * TILE]
    C.copy_(torch.from_numpy(out).to(C.dtype))
    return C


def bsr_sddmm(entry_row, columns, entry_ids, nnz, dC, B, dvalues):
    calls.append(("bsr_sddmm", (tuple(dC.shape), tuple(B.shape), nnz)))
    assert entry_row.dtype == torch.int32 and columns.dtype == torch.int32
    assert entry_row.numel() == nnz and columns.numel() == nnz
    assert dvalues.dim() == 3 and dvalues.shape[1:] == (TILE, TILE) and dvalues.is_contiguous()
    row, col, ids = _np(entry_row).astype(np.int64), _np(columns).astype(np.int64), _ids(entry_ids, nnz)
    assert sorted(ids.tolist()) == list(range(dvalues.shape[0])), "every block of the gradient is written once"
    g, b = _np(dC.double()), _np(B.double())
    out = np.zeros(tuple(dvalues.shape))
    for p in range(nnz):
        gi, bj = g[:, row[p] * TILE:(row[p] + 1) * TILE], b[:, col[p] * TILE:(col[p] + 1) * TILE]
        out[ids[p]] = np.einsum("bin,bjn->ij", gi, bj)
    dvalues.copy_(torch.from_numpy(out).to(dvalues.dtype))
    return dvalues
