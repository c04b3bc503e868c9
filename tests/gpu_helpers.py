"""Shared helpers of the GPU parity modules (tests/test_gpu_*.py): input builders, reference expressions, C-ABI shims.
Fixtures (dev, cmm, mm, capi) live in conftest.py."""
import ctypes
import sys

import numpy as np
import pytest
import torch

RTOL, ATOL = 1e-5, 1e-8

__all__ = ['RTOL', 'ATOL', 't', 'torch_cpu_csr_matmul', 'assert_matches_reference_expression', 'run_spmm', '_random_rows_csr', '_transpose_through_the_c_abi', 'gemm_ref', '_dense_of', 'fwd_bwd_device', '_panel_sorted', '_sub_csr', '_moderately_dense_with_hub_rows',
           'assert_same_bits', 'gamma', 'assert_within_gamma_bound',
           'sum_grads_f64', 'select_grads_f64', 'Padded', 'padded', 'SENTINEL', 'assert_outside_untouched', '_sparse_attention_through_the_c_abi',
           '_sparse_attention_backward_through_the_c_abi', '_block_attention_fwd_through_the_c_abi',
           '_block_attention_bwd_through_the_c_abi']


def t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def torch_cpu_csr_matmul(rowptr, col, val, M, K, B):
    """The reference's own CPU expression `a @ b` (reference matmuls.py:41,71,210,234,279,302) with A as a torch
    CSR tensor, evaluated by torch-CPU: the expectation of the reference's tests (tests/naive_kernel_test.py:30)."""
    a_csr = torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                    torch.from_numpy(val), (M, K))
    return (a_csr @ torch.from_numpy(B)).numpy()


def assert_matches_reference_expression(got, ref):
    """tests/naive_kernel_test.py:36-37: shape equality + torch.allclose at its defaults, on the FULL output."""
    assert got.shape == ref.shape
    assert torch.allclose(torch.from_numpy(got), torch.from_numpy(ref), rtol=RTOL, atol=ATOL), \
        f"max rel err vs torch-CPU A_csr @ B: {np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30))}"


def run_spmm(cmm, dev, rowptr, col, val, M, K, B, op="naive_spmm"):
    C = torch.full((M, B.shape[1]), float("nan"), device=dev)
    out = getattr(cmm, op)(t(val, dev), t(col, dev), t(rowptr, dev), len(val), M, K, t(B, dev), C)
    assert out is C or out.data_ptr() == C.data_ptr()  # same tensor returned (reference custom_mm.cpp:178,216)
    return C.cpu().numpy()


def _random_rows_csr(M, K, lens, seed, shuffle=0.0, duplicates=False):
    g = np.random.Generator(np.random.PCG64(seed))
    cols = []
    lens = np.asarray(lens)
    for r in np.nonzero(lens)[0]:
        n = int(lens[r])
        c = g.integers(0, K, size=n) if (duplicates or n > K) else g.choice(K, size=n, replace=False)
        c = np.sort(c)
        if shuffle and g.random() < shuffle:
            c = g.permutation(c)
        cols.append(c.astype(np.int32))
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate(cols) if cols else np.zeros(0, np.int32)
    return rowptr, col, (g.random(len(col), dtype=np.float32) - 0.5)


def _transpose_through_the_c_abi(capi, dev, rowptr, col, val, M, K, plan):
    """mi_csr_transpose_f32 with the plan pinned (1 tables, 2 one-sweep); returns (t_rowptr, t_col, t_val) on the host and
    checks the one-sweep plan's give-up flag."""
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_size_t
    capi.mi_csr_transpose_workspace_bytes.restype = sz
    capi.mi_csr_transpose_workspace_bytes.argtypes = [i32, i32, i64]
    capi.mi_csr_transpose_f32.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, sz, vp]
    capi.mi_csr_transpose_check.argtypes = [vp, sz, i32, i32, i32, i64, vp]
    nnz = len(val)
    d_rp, d_col, d_val = t(rowptr, dev), t(col, dev), t(val, dev)
    ws_bytes = capi.mi_csr_transpose_workspace_bytes(M, K, nnz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    t_rp = torch.full((K + 1,), -1, dtype=torch.int32, device=dev)
    t_col = torch.full((nnz,), -1, dtype=torch.int32, device=dev)
    t_val = torch.full((nnz,), -1.0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    assert capi.mi_csr_transpose_set_plan(plan) == 0
    try:
        st = capi.mi_csr_transpose_f32(d_rp.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), nnz, M, K, t_rp.data_ptr(),
                                       t_col.data_ptr(), t_val.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    finally:
        capi.mi_csr_transpose_set_plan(0)
    assert st == 0, st
    assert capi.mi_csr_transpose_check(ws.data_ptr(), ws_bytes, 1, M, K, nnz, stream) == 0, "a look-back poll gave up"
    return t_rp.cpu().numpy(), t_col.cpu().numpy(), t_val.cpu().numpy()


class Padded:
    """A dense operand [batch, rows, D] of the attention entries inside a larger buffer of its own: `buf` (1-d), the logical
    view `x` on it, the leading dimension `ld` and the item stride `stride` in elements."""

    def __init__(self, buf, x, ld, stride):
        self.buf, self.x, self.ld, self.stride = buf, x, ld, stride

    def args(self, stride=None):
        return [self.buf.data_ptr(), self.ld, self.stride if stride is None else stride]

    def outside(self):
        """The buffer's elements outside the logical [batch][rows][:D]."""
        inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        inside.as_strided(self.x.shape, self.x.stride()).fill_(True)
        return self.buf[~inside]


def padded(x, number, fill, step=8):
    """Operand number `number` of a call as a Padded: leading dimension D + step·(number + 1), item stride rows·ld +
    step·(number + 1) — different from every other operand's and from the packed ones; with step = 8 rows are 16-byte
    aligned for every dtype, with step = 4 a 2-byte dtype's rows of the even-numbered operands sit on 8-byte boundaries
    only (what the fused bfloat16 / float16 entries ask for) —, everything outside the logical region set to `fill` (NaN
    for an input: it stays out of the results only if nothing outside is read; SENTINEL for an output, checked afterwards
    with assert_outside_untouched)."""
    batch, rows, D = x.shape
    ld = D + step * (number + 1)
    stride = rows * ld + step * (number + 1)
    buf = torch.full((batch * stride + 8,), fill, dtype=x.dtype, device=x.device)
    view = buf.as_strided((batch, rows, D), (stride, ld, 1))
    view.copy_(x)
    return Padded(buf, view, ld, stride)


SENTINEL = -7.5  # around the outputs of a padded call: finite, exact in float32, bfloat16 and float16


def assert_outside_untouched(p, what):
    """The call left every element of the Padded output `p` outside its logical region at SENTINEL."""
    rest = p.outside()
    assert_same_bits(rest, torch.full_like(rest, SENTINEL), f"{what}: outside the logical region")


def _attention_entry(capi, name):
    """A fused / block attention entry of the C ABI with its argument types (include/mi_spmm.h)."""
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    dense = [vp, i64, i64]
    fn = getattr(capi, name)
    if name.startswith("mi_sparse_attention_backward_"):
        fn.argtypes = [vp, vp, i64, i32, i32, i32, i32] + 4 * dense + [vp, f32] + dense + [vp, vp, vp, sz, vp]
    elif name.startswith("mi_sparse_attention_"):
        fn.argtypes = [vp, vp, i64, i32, i32, i32, i32] + 3 * dense + [f32] + dense + [vp, vp, sz, vp]
    elif name.startswith("mi_block_attention_fwd_"):
        fn.argtypes = [vp, vp, i64] + 6 * [i32] + 3 * dense + [f32] + dense + [vp, vp]
    else:
        fn.argtypes = [vp, vp, vp, vp, i64] + 6 * [i32] + 5 * dense + [vp, f32] + 3 * dense + [vp, sz, vp]
    fn.restype = ctypes.c_int
    return fn


_SUFFIX = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def _sparse_attention_through_the_c_abi(capi, dtype, offsets, columns, batch, M, K, D, q, k, v, scale, out, stats,
                                        kv_stride=None):
    """mi_sparse_attention_T on Padded operands (kv_stride: the item stride passed for k and v instead of their own);
    returns the status."""
    fn = _attention_entry(capi, f"mi_sparse_attention_{_SUFFIX[dtype]}")
    stream = torch.cuda.current_stream().cuda_stream
    return fn(offsets.data_ptr(), columns.data_ptr(), columns.numel(), batch, M, K, D, *q.args(), *k.args(kv_stride),
              *v.args(kv_stride), scale, *out.args(), stats.data_ptr(), None, 0, stream)


def _sparse_attention_backward_through_the_c_abi(capi, dtype, offsets, columns, batch, M, K, D, q, k, v, dout, stats, scale,
                                                 dq, y, ds, kv_stride=None):
    """mi_sparse_attention_backward_T on Padded operands (y, ds: plain [nnz] tensors); returns the status."""
    fn = _attention_entry(capi, f"mi_sparse_attention_backward_{_SUFFIX[dtype]}")
    stream = torch.cuda.current_stream().cuda_stream
    return fn(offsets.data_ptr(), columns.data_ptr(), columns.numel(), batch, M, K, D, *q.args(), *k.args(kv_stride),
              *v.args(kv_stride), *dout.args(), stats.data_ptr(), scale, *dq.args(), y.data_ptr(), ds.data_ptr(), None, 0, stream)


def _block_attention_fwd_through_the_c_abi(capi, dtype, offsets, columns, nnz, layouts, batch, Sq, Sk, D, causal, q, k, v,
                                           scale, out, lse, kv_stride=None):
    """mi_block_attention_fwd_T on Padded operands; returns the status."""
    fn = _attention_entry(capi, f"mi_block_attention_fwd_{_SUFFIX[dtype]}")
    stream = torch.cuda.current_stream().cuda_stream
    return fn(offsets.data_ptr(), columns.data_ptr(), nnz, layouts, batch, Sq, Sk, D, causal, *q.args(), *k.args(kv_stride),
              *v.args(kv_stride), scale, *out.args(), lse.data_ptr(), stream)


def _block_attention_bwd_through_the_c_abi(capi, dtype, offsets, columns, t_offsets, t_columns, nnz, layouts, batch, Sq, Sk, D,
                                           causal, q, k, v, out, dout, lse, scale, dq, dk, dv, kv_stride=None):
    """mi_block_attention_bwd_T on Padded operands, with a workspace of mi_block_attention_workspace_bytes; returns the
    status."""
    fn = _attention_entry(capi, f"mi_block_attention_bwd_{_SUFFIX[dtype]}")
    capi.mi_block_attention_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
    capi.mi_block_attention_workspace_bytes.restype = ctypes.c_size_t
    ws_bytes = capi.mi_block_attention_workspace_bytes(batch, Sq)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=lse.device)
    stream = torch.cuda.current_stream().cuda_stream
    return fn(offsets.data_ptr(), columns.data_ptr(), t_offsets.data_ptr(), t_columns.data_ptr(), nnz, layouts, batch, Sq, Sk, D,
              causal, *q.args(), *k.args(kv_stride), *v.args(kv_stride), *out.args(), *dout.args(), lse.data_ptr(), scale,
              *dq.args(), *dk.args(), *dv.args(), ws.data_ptr(), ws_bytes, stream)


def gemm_ref(oracle_mod, a, b, ta, tb):
    return oracle_mod.gemm(a, b, ta, tb)


def _dense_of(rowptr, col, val, M, K):
    A = np.zeros((M, K), np.float64)
    rows = np.repeat(np.arange(M), np.diff(rowptr))
    np.add.at(A, (rows, col), val)
    return A


def fwd_bwd_device(fn, ref_fn, a, b, dev):
    a1, b1 = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    a2, b2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out, exp = fn(a1, b1), ref_fn(a2, b2)
    assert out.is_cuda and out.shape == exp.shape
    assert torch.allclose(exp, out.cpu(), rtol=RTOL, atol=ATOL)
    dc = torch.rand(exp.shape, generator=torch.Generator().manual_seed(3))
    out.backward(dc.to(dev))
    exp.backward(dc)
    assert torch.allclose(a2.grad, a1.grad.cpu(), rtol=RTOL, atol=ATOL)
    assert torch.allclose(b2.grad, b1.grad.cpu(), rtol=RTOL, atol=ATOL)


def _panel_sorted(rowptr, col, val, split):
    """Entries of each row reordered the way two unchecked panel passes would consume them."""
    c2, v2 = col.copy(), val.copy()
    for r in range(len(rowptr) - 1):
        s0, e0 = rowptr[r], rowptr[r + 1]
        order = np.argsort(col[s0:e0] >= split, kind="stable")
        c2[s0:e0], v2[s0:e0] = col[s0:e0][order], val[s0:e0][order]
    return c2, v2


def _sub_csr(rowptr, col, val, rows):
    """CSR of the selected rows (rows of a product are independent: the oracle on this equals the
    oracle on the whole matrix restricted to these rows)."""
    lens = [int(rowptr[r + 1] - rowptr[r]) for r in rows]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows]) if rows else np.zeros(0, np.int64)
    return rp, col[idx], val[idx]


def _moderately_dense_with_hub_rows(M, K, density, hubs, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    mask = g.random((M, K), dtype=np.float32) < density
    mask[hubs] = True
    rows, col = np.nonzero(mask)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M))]).astype(np.int32)
    return rowptr, col.astype(np.int32), g.random(len(col), dtype=np.float32) - 0.5


def assert_same_bits(got, want, what=""):
    """Bit-for-bit equality of two float tensors / arrays (float32, bfloat16 or float16): NaN by position, every other value
    by its bits (−0 and ±inf included)."""
    got = torch.as_tensor(got).detach().cpu()
    want = torch.as_tensor(want).detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn), f"{what}: NaN positions differ ({torch.nonzero(gn != wn)[:5].tolist()})"
    ib = torch.int32 if got.element_size() == 4 else torch.int16
    gb, wb = got.view(ib)[~gn], want.view(ib)[~wn]
    bad = torch.nonzero(gb != wb).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {gb.numel()} values differ, first at {bad[:5].tolist()}: got "
                              f"{got[~gn][bad[:5]].tolist()} want {want[~wn][bad[:5]].tolist()}")


def gamma(n, u=2.0 ** -24):
    """γ_n = n·u / (1 − n·u): the rounding-error factor of any summation of n (fused) products in precision u."""
    return n * u / (1 - n * u)


def assert_within_gamma_bound(got, ref64, abs64, n, what="", store_u=0.0, store_abs=0.0):
    """|got − ref| ≤ γ_n·Σ|terms| (+ the store rounding store_u·|ref| + store_abs of a narrowing to 16 bits), elementwise,
    against a float64 reference `ref64` whose terms' absolute values sum to `abs64`; non-finite references are skipped
    (specials are checked bit for bit elsewhere).  Catches a wrong formula that a kernel and an order-restating oracle
    could share (a transposed gradient, a wrong divisor)."""
    got = np.asarray(torch.as_tensor(got).detach().cpu().double().numpy(), np.float64)
    ref64, abs64 = np.asarray(ref64, np.float64), np.asarray(abs64, np.float64)
    assert got.shape == ref64.shape == abs64.shape, (what, got.shape, ref64.shape, abs64.shape)
    fin = np.isfinite(ref64) & np.isfinite(abs64)
    tol = gamma(n) * abs64 * (1 + store_u) + store_u * np.abs(ref64) + store_abs
    err = np.abs(got - ref64)
    bad = fin & ~(err <= tol)
    assert not bad.any(), (f"{what}: {int(bad.sum())} values outside γ_{n}·Σ|terms| of the float64 reference; first "
                           f"{np.argwhere(bad)[:3].tolist()} got {got[bad][:3].tolist()} ref {ref64[bad][:3].tolist()} "
                           f"tol {tol[bad][:3].tolist()}")


def _rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(np.asarray(rowptr, np.int64)))


def sum_grads_f64(rowptr, col, val, M, K, B, G):
    """Float64 gradients of C = A·B (A CSR, duplicates and unsorted columns allowed), each with the sum of its terms'
    absolute values: (grad_val, Σ|terms| of grad_val, grad_B, Σ|terms| of grad_B).  grad_val[e] = Σ_j G[row(e), j]·B[col[e], j]
    (numpy, float64, in chunks); grad_B = Aᵀ·G through a torch-CPU float64 sparse product."""
    B64, G64 = np.asarray(B, np.float64), np.asarray(G, np.float64)
    rows, col = _rows_of(rowptr), np.asarray(col, np.int64)
    gv, gva = np.zeros(len(col)), np.zeros(len(col))
    step = max(1, (1 << 21) // max(B64.shape[1], 1))
    for s0 in range(0, len(col), step):
        r, c = rows[s0:s0 + step], col[s0:s0 + step]
        gv[s0:s0 + len(r)] = np.einsum("ij,ij->i", G64[r], B64[c])
        gva[s0:s0 + len(r)] = np.einsum("ij,ij->i", np.abs(G64[r]), np.abs(B64[c]))

    def at_g(v, g):
        idx = torch.from_numpy(np.stack([col, rows])) if len(col) else torch.zeros((2, 0), dtype=torch.int64)
        at = torch.sparse_coo_tensor(idx, torch.from_numpy(np.asarray(v, np.float64)), (K, M))
        return torch.sparse.mm(at, torch.from_numpy(g)).numpy()

    v64 = np.asarray(val, np.float64)
    return gv, gva, at_g(v64, G64), at_g(np.abs(v64), np.abs(G64))


def select_grads_f64(rowptr, col, val, M, K, B, G, arg):
    """Float64 gradients of amax / amin from the forward's selected entry per output element (`arg`, nnz where none):
    grad_val[e] = Σ_{j: arg[i,j] = e} G[i,j]·B[col[e],j], grad_B[col[e], j] = Σ_{i: arg[i,j] = e} val[e]·G[i,j]; with the
    sums of the terms' absolute values, as sum_grads_f64.  (Row blocks at a time: the 10⁶-row cases stay small.)"""
    nnz, N = len(col), np.shape(arg)[1]
    col = np.asarray(col, np.int64)
    gv, gva, gb, gba = np.zeros(nnz), np.zeros(nnz), np.zeros(K * N), np.zeros(K * N)
    step = max(1, (1 << 21) // max(N, 1))
    for r0 in range(0, M, step):
        a = np.asarray(arg[r0:r0 + step], np.int64)
        i, j = np.nonzero((a >= 0) & (a < nnz))
        e = a[i, j]
        i = i + r0
        g = np.asarray(G[i, j], np.float64)
        b = np.asarray(B[col[e], j], np.float64)
        v = np.asarray(val, np.float64)[e]
        gv += np.bincount(e, weights=g * b, minlength=nnz)
        gva += np.bincount(e, weights=np.abs(g * b), minlength=nnz)
        gb += np.bincount(col[e] * N + j, weights=v * g, minlength=K * N)
        gba += np.bincount(col[e] * N + j, weights=np.abs(v * g), minlength=K * N)
    return gv, gva, gb.reshape(K, N), gba.reshape(K, N)
