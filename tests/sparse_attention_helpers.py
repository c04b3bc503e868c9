"""Shared by tests/test_gpu_csr_softmax.py, tests/test_gpu_sparse_attention.py, tests/test_gpu_fused_attention.py and
tests/test_gpu_block_attention.py: input builders, the float64 / float32 torch-CPU references (dense_step: dense masked
attention, optionally narrowed once per stage) and the e_dev ≤ 8 · e_ref rule, for a whole tensor and per class of rows.
The measured pairs are printed and appended to the file MI_SOFTMAX_LOG names, when it names one."""
import os

import numpy as np
import torch

FACTOR = 8.0  # e_dev ≤ FACTOR · e_ref: torch-CPU's float32 figure is two half-ulps; a 1-ulp expf, a reciprocal-multiply and a
#               tree sum of depth ≤ 15 fit under 16 half-ulps; the fast exponential at a spread of 40 does not


def record(what, e_ref, e_dev):
    line = f"{what}: e_ref {e_ref:.3e}  e_dev {e_dev:.3e}  ratio {e_dev / e_ref if e_ref > 0 else float('nan'):.2f}"
    print(line)
    path = os.environ.get("MI_SOFTMAX_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def assert_under_rule(what, e_ref, e_dev):
    record(what, e_ref, e_dev)
    assert e_dev <= FACTOR * e_ref, f"{what}: e_dev {e_dev:.3e} > {FACTOR:g} · e_ref {e_ref:.3e}"


def _f64(x):
    return np.asarray(torch.as_tensor(x).detach().cpu().double().numpy(), np.float64)


def assert_tensor_under_rule(what, got, yard, ref):
    """The rule on one whole tensor: `got` the device result, `yard` the yardstick's, `ref` the float64 one."""
    got, yard, ref = _f64(got), _f64(yard), _f64(ref)
    assert got.shape == yard.shape == ref.shape, (what, got.shape, yard.shape, ref.shape)
    assert_under_rule(what, scaled_err(yard, ref), scaled_err(got, ref))


def assert_under_rule_by_rows(what, got, yard, ref, classes):
    """The rule on the whole row-indexed tensor [rows, D] (out, dq), then on each class of rows alone: `classes` maps a
    name to row indices, scaled_err is taken over those rows only — a long row's small outputs are measured against their
    own maximum, not against the short rows' — and the bound is FACTOR · max(e_ref of the class, e_ref of the whole
    tensor): the floor keeps a class of few elements from failing on a lucky yardstick.  `yard` is the yardstick's result,
    `ref` the float64 one."""
    got, yard, ref = _f64(got), _f64(yard), _f64(ref)
    assert got.ndim == 2, (what, got.shape)
    assert_tensor_under_rule(f"{what}, all rows", got, yard, ref)
    e_all = scaled_err(yard, ref)
    for name, rows in classes.items():
        rows = np.asarray(rows, np.int64)
        e_class = scaled_err(yard[rows], ref[rows])
        assert_under_rule(f"{what}, rows {name} ({len(rows)} rows, their own e_ref {e_class:.3e})", max(e_class, e_all),
                          scaled_err(got[rows], ref[rows]))


def dense_step(q, k, v, w, mask, scale, wide, narrow=None):
    """Dense masked attention on the CPU in `wide`, with autograd: (out, dq, dk, dv) for the incoming gradient w; rows of
    the mask that see nothing give zero rows.  `narrow` (T) rounds the scores, the probabilities and the product to T and
    widens them again — with wide = float32 the yardstick of a bfloat16 / float16 device result; for a float32 device
    result the yardstick is the plain expression in float32 (narrow=None), the reference the one in float64."""
    rnd = (lambda t: t) if narrow is None else (lambda t: t.to(narrow).to(wide))
    rq, rk, rv = (t.detach().cpu().to(wide).requires_grad_(True) for t in (q, k, v))
    s = rnd(scale * (rq @ rk.transpose(-1, -2)))
    empty = ~mask.any(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(~mask & ~empty, -float("inf")), -1)
    p = rnd(torch.where(empty, torch.zeros_like(p), p))
    out = rnd(p @ rv)
    grads = torch.autograd.grad(out, (rq, rk, rv), grad_outputs=w.detach().cpu().to(wide))
    return (out.detach(),) + tuple(g.detach() for g in grads)


def rel_err(y, y64):
    """max over entries of |y − y64| / y64 (entries of the float64 reference that are 0 or non-finite are left out)."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    ok = np.isfinite(y64) & (y64 != 0)
    return float(np.max(np.abs(y[ok] - y64[ok]) / np.abs(y64[ok]))) if ok.any() else 0.0


def scaled_err(g, g64):
    """max |g − g64| / max |g64|."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return float(np.max(np.abs(g - g64)) / np.max(np.abs(g64)))


def rows_pattern(lens, K, seed):
    """(rowptr int32, columns int32) with sorted distinct columns per row."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cols = np.empty(int(rowptr[-1]), np.int32)
    for r in np.nonzero(lens)[0]:
        n = int(lens[r])
        cols[rowptr[r]:rowptr[r + 1]] = np.arange(K, dtype=np.int32) if n == K else np.sort(g.choice(K, n, replace=False))
    return rowptr, cols


def accuracy_matrix(seed=1, M=4000, K=20000):
    """The matrix of the accuracy check: row lengths uniform 1 … 200 with 10 % empty, the first six rows forced to 0, 1, 64,
    65, 5000 and 20000 entries."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens = g.integers(1, 201, size=M)
    lens[g.random(M) < 0.1] = 0
    lens[:6] = (0, 1, 64, 65, 5000, 20000)
    rowptr, cols = rows_pattern(lens, K, seed + 100)
    nnz = int(rowptr[-1])
    return rowptr, cols, (4.0 * g.standard_normal(nnz)).astype(np.float32), (g.random(nnz) - 0.5).astype(np.float32), \
        g.standard_normal(nnz).astype(np.float32)


def coo_of(rowptr, cols, vals, M, K, dtype):
    rows = np.repeat(np.arange(M), np.diff(rowptr.astype(np.int64)))
    idx = torch.from_numpy(np.stack([rows, cols.astype(np.int64)]))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(vals)).to(dtype), (M, K)).coalesce()


def cpu_sparse_softmax(rowptr, cols, vals, M, K, dy, dtype):
    """torch.sparse.softmax on the CPU, on the COO form (sorted distinct columns: the coalesced order is the CSR order);
    returns (y, dx) as numpy arrays in CSR order, dx for the incoming gradient dy through torch autograd."""
    x = coo_of(rowptr, cols, vals, M, K, dtype).requires_grad_(True)
    y = torch.sparse.softmax(x, 1)
    w = coo_of(rowptr, cols, dy, M, K, dtype)
    (gx,) = torch.autograd.grad(y, x, grad_outputs=w)
    return y.detach().coalesce().values().numpy(), gx.coalesce().values().numpy()


def row_sums64(rowptr, y):
    y = np.asarray(y, np.float64)
    out = np.zeros(len(rowptr) - 1)
    lens = np.diff(rowptr.astype(np.int64))
    nz = lens > 0
    out[nz] = np.add.reduceat(y, rowptr[:-1][nz].astype(np.int64)) if len(y) else 0
    return out, lens


def dev_softmax(cmm, dev, vals, rowptr, M, scale=1.0, batch=1, dtype=torch.float32, in_place=False):
    x = torch.as_tensor(vals).to(device=dev, dtype=dtype).contiguous()
    off = torch.as_tensor(np.asarray(rowptr, np.int32)).to(dev)
    out = x if in_place else torch.full_like(x, float("nan"))
    got = cmm.csr_softmax(x, off, x.numel(), batch, M, scale, out)
    assert got.data_ptr() == out.data_ptr()
    return out


def dev_softmax_backward(cmm, dev, y, dy, rowptr, M, scale=1.0, batch=1, in_place=False):
    y = torch.as_tensor(y).to(dev).contiguous()
    dy = torch.as_tensor(dy).to(device=dev, dtype=y.dtype).contiguous()
    off = torch.as_tensor(np.asarray(rowptr, np.int32)).to(dev)
    out = dy if in_place else torch.full_like(y, float("nan"))
    got = cmm.csr_softmax_backward(y, dy, off, y.numel(), batch, M, scale, out)
    assert got.data_ptr() == out.data_ptr()
    return out


def device_pattern(dev, batch_shape, S, keep, seed, index_dtype=torch.int64):
    """A batched (or, batch_shape = (), 2-d) CSR pattern [*batch_shape, S, S] built on the device: every row keeps
    exactly max(1, round(keep · S)) sorted distinct columns.  Values 1."""
    g = torch.Generator(device=dev).manual_seed(seed)
    k = max(1, int(round(keep * S)))
    nb = int(np.prod(batch_shape)) if batch_shape else 1
    cols = torch.rand((nb, S, S), device=dev, generator=g).topk(k, dim=-1).indices.sort(dim=-1).values
    crow = (torch.arange(S + 1, device=dev) * k).expand(nb, S + 1)
    shape = tuple(batch_shape) + (S, S)
    crow = crow.reshape(tuple(batch_shape) + (S + 1,)).to(index_dtype).contiguous()
    col = cols.reshape(tuple(batch_shape) + (S * k,)).to(index_dtype).contiguous()
    vals = torch.ones(tuple(batch_shape) + (S * k,), device=dev)
    return torch.sparse_csr_tensor(crow, col, vals, size=shape)


def with_values(a, values):
    v = torch.Tensor.values(a)
    return torch.sparse_csr_tensor(torch.Tensor.crow_indices(a), torch.Tensor.col_indices(a), values.reshape(v.shape),
                                   size=a.shape)


def dense_mask(a):
    """Boolean CPU mask of a CSR tensor's stored positions."""
    return with_values(a, torch.ones_like(torch.Tensor.values(a))).cpu().to_dense() != 0
