"""CSR × dense with reduce = mean / amax / amin (torch.sparse.mm's `reduce`) and its autograd, on the MI355X.

The expectation is torch-CPU's own kernel, aten::_sparse_mm_reduce_impl, on the same CSR arrays (torch implements
`reduce` for CSR on the CPU only).  amax / amin round nothing beyond one fp32 multiply, so output and arg are compared
bit for bit: NaN by position, every other value by its bits (the sign of zero included).  mean is bit-exact against
naive_spmm's bits divided by the row counts in numpy float32, and close to torch.  Gradients are close to torch-CPU
autograd and bit-identical from run to run (no float atomics).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 64, 100, 128, 130, 256, 320, 512, 602, 1024]


def csr_rows(M, K, lens, seed, sort=False, replace=False):
    g = np.random.Generator(np.random.PCG64(seed))
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cols = [g.integers(0, K, int(n)) if replace else g.choice(K, int(n), replace=False) for n in lens]
    col = np.concatenate([np.sort(c) if sort else c for c in cols]).astype(np.int32) if len(cols) else np.zeros(0, np.int32)
    val = (g.random(len(col), dtype=np.float32) - 0.5).astype(np.float32)
    return rowptr, col, val


def torch_reduce(rowptr, col, val, M, K, B, reduce):
    a = torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                torch.from_numpy(val), (M, K)).requires_grad_()
    out, arg = torch.ops.aten._sparse_mm_reduce_impl(a, torch.from_numpy(B), reduce)
    return out.detach().numpy(), arg.numpy()


def gpu_reduce(cmm, dev, rowptr, col, val, M, K, B, reduce, with_arg=True):
    C = torch.empty((M, B.shape[1]), device=dev)
    arg = torch.empty((M, B.shape[1]), device=dev, dtype=torch.int32) if with_arg else None
    cmm.naive_spmm_reduce(torch.from_numpy(val).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(rowptr).to(dev),
                          len(val), M, K, torch.from_numpy(np.ascontiguousarray(B)).to(dev), C, reduce, arg)
    return C.cpu().numpy(), None if arg is None else arg.cpu().numpy()


def assert_same_bits(got, want, what=""):
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ ({np.argwhere(gn != wn)[:5].tolist()})"
    gb, wb = got.view(np.int32)[~gn], want.view(np.int32)[~wn]
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, f"{what}: {bad.size} values differ, first got {got[~gn][bad[:5]]} want {want[~wn][bad[:5]]}"


def check_select(cmm, dev, rowptr, col, val, M, K, B, what=""):
    for r in ("amax", "amin"):
        want, want_arg = torch_reduce(rowptr, col, val, M, K, B, r)
        got, got_arg = gpu_reduce(cmm, dev, rowptr, col, val, M, K, B, r)
        assert_same_bits(got, want, f"{what} {r}")
        assert np.array_equal(got_arg, want_arg), f"{what} {r}: arg differs at {np.argwhere(got_arg != want_arg)[:5].tolist()}"
        got_noarg, _ = gpu_reduce(cmm, dev, rowptr, col, val, M, K, B, r, with_arg=False)
        assert_same_bits(got_noarg, want, f"{what} {r} without arg")


def mixed_lengths(M, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    lens = g.integers(1, 201, M)
    lens[g.random(M) < 0.1] = 0  # empty rows
    lens[:3] = (0, 1, 200)
    return lens


@pytest.mark.parametrize("N", WIDTHS)
def test_amax_amin_bit_exact_vs_torch_at_every_width(cmm, dev, N):
    M, K = 160, 700
    rowptr, col, val = csr_rows(M, K, mixed_lengths(M, N), seed=N)  # unsorted columns
    B = np.random.Generator(np.random.PCG64(100 + N)).standard_normal((K, N), dtype=np.float32)
    check_select(cmm, dev, rowptr, col, val, M, K, B, f"N={N}")


@pytest.mark.parametrize("N", [3, 33, 64, 130, 256])
def test_unaligned_leading_dimension_of_B(cmm, dev, N):
    M, K = 120, 400
    rowptr, col, val = csr_rows(M, K, mixed_lengths(M, 7 + N), seed=7 + N)
    Bw = np.random.Generator(np.random.PCG64(N)).standard_normal((K, N + 3), dtype=np.float32)
    Bt = torch.from_numpy(Bw).to(dev)[:, 1:N + 1]  # a view: ldb = N + 3, first column 4 bytes in
    for r in ("amax", "amin"):
        want, want_arg = torch_reduce(rowptr, col, val, M, K, np.ascontiguousarray(Bw[:, 1:N + 1]), r)
        C = torch.empty((M, N), device=dev)
        arg = torch.empty((M, N), device=dev, dtype=torch.int32)
        cmm.naive_spmm_reduce(torch.from_numpy(val).to(dev), torch.from_numpy(col).to(dev),
                              torch.from_numpy(rowptr).to(dev), len(val), M, K, Bt, C, r, arg)
        assert_same_bits(C.cpu().numpy(), want, f"N={N} {r}")
        assert np.array_equal(arg.cpu().numpy(), want_arg)


def test_ties_everywhere(cmm, dev):
    M, K = 200, 300
    g = np.random.Generator(np.random.PCG64(5))
    rowptr, col, _ = csr_rows(M, K, mixed_lengths(M, 5), seed=5)
    val = g.choice(np.array([1.0, -1.0, 2.0, 0.5], np.float32), len(col))
    for N in (1, 4, 37, 256):
        B = g.integers(-2, 3, (K, N)).astype(np.float32)  # products from a handful of values: ties in every row
        check_select(cmm, dev, rowptr, col, val, M, K, B, f"ties N={N}")


def test_signed_zeros_infinities_and_nan(cmm, dev):
    M, K = 200, 300
    g = np.random.Generator(np.random.PCG64(9))
    rowptr, col, _ = csr_rows(M, K, mixed_lengths(M, 9), seed=9)
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, np.inf, -np.inf, np.nan], np.float32)
    val = g.choice(np.array([0.0, -0.0, 1.0, -1.0, 2.0, np.inf], np.float32), len(col))  # 0 × inf = NaN
    for N in (1, 5, 64, 130):
        B = g.choice(special, (K, N), p=[.15, .15, .15, .15, .1, .1, .08, .08, .04]).astype(np.float32)
        check_select(cmm, dev, rowptr, col, val, M, K, B, f"specials N={N}")
    # every product of a column is -inf (amax: out -inf, arg nnz) or +inf (amin)
    val = g.random(len(col), dtype=np.float32) + 0.5
    B = np.random.Generator(np.random.PCG64(1)).standard_normal((K, 8), dtype=np.float32)
    B[:, 2] = -np.inf
    B[:, 5] = np.inf
    check_select(cmm, dev, rowptr, col, val, M, K, B, "all-inf columns")


@pytest.mark.parametrize("N", [64, 256])
def test_hub_rows_bit_exact_vs_torch(cmm, dev, N):
    M, K = 1200, 200_000
    lens = np.full(M, 100, np.int64)
    lens[[3, 700]] = (100_000, 1_000_000)
    lens[900] = 20_000  # split into one chunk
    rowptr, col, val = csr_rows(M, K, lens, seed=N, replace=True)
    g = np.random.Generator(np.random.PCG64(N + 1))
    B = g.standard_normal((K, N), dtype=np.float32)
    check_select(cmm, dev, rowptr, col, val, M, K, B, f"hub rows N={N}")
    B = g.integers(-2, 3, (K, N)).astype(np.float32)  # ties across the chunks of a hub row
    B[g.random((K, N)) < 2e-6] = np.nan
    check_select(cmm, dev, rowptr, col, val, M, K, B, f"hub rows with ties N={N}")


@pytest.mark.parametrize("N", [3, 6, 258])
def test_hub_rows_at_partial_widths_bit_exact_vs_torch(cmm, dev, N):
    """The hub kernels at the widths the test above does not reach: N = 3 is their one-column-per-lane form, N = 6 ends in
    a quad shifted back over its neighbour, N = 258 has a second column block whose only quad is shifted back, in the hub
    and in the combine kernel.  One row in one chunk, a short row, a row through the two-chunk combine, an empty row."""
    M, K = 4, 4096
    rowptr, col, val = csr_rows(M, K, (9000, 5, 40000, 0), seed=N, replace=True)
    B = np.random.Generator(np.random.PCG64(N + 1)).standard_normal((K, N), dtype=np.float32)
    check_select(cmm, dev, rowptr, col, val, M, K, B, f"hub rows N={N}")


def test_c3_amax_with_arg_sampled_rows_vs_torch(cmm, dev):
    M = K = 1_000_000
    N, per_row = 256, 100  # 0.01 %
    gen = torch.Generator(device=dev).manual_seed(3)
    rowptr_d = torch.arange(0, (M + 1) * per_row, per_row, device=dev, dtype=torch.int32)
    col_d = torch.randint(0, K, (M * per_row,), device=dev, dtype=torch.int32, generator=gen)
    val_d = torch.rand(M * per_row, device=dev, generator=gen) - 0.5
    B_d = torch.randn(K, N, device=dev, generator=gen)
    C = torch.empty(M, N, device=dev)
    arg = torch.empty(M, N, device=dev, dtype=torch.int32)
    cmm.naive_spmm_reduce(val_d, col_d, rowptr_d, M * per_row, M, K, B_d, C, "amax", arg)
    rows = np.sort(np.random.Generator(np.random.PCG64(11)).choice(M, 4096, replace=False))
    rows_d = torch.from_numpy(rows).to(dev)
    idx = (rows_d[:, None].long() * per_row + torch.arange(per_row, device=dev)).reshape(-1)
    sub_col = col_d[idx]
    uniq, inv = torch.unique(sub_col, return_inverse=True)
    rp_sub = np.arange(0, (len(rows) + 1) * per_row, per_row, dtype=np.int32)
    want, want_arg = torch_reduce(rp_sub, inv.int().cpu().numpy(), val_d[idx].cpu().numpy(), len(rows), len(uniq),
                                  B_d[uniq.long()].cpu().numpy(), "amax")
    # the sub-CSR renumbers entries: entry rp_sub[k] + t of sub-row k is rowptr[r] + t of the matrix; nnz_sub → nnz
    rowptr = rowptr_d.cpu().numpy()
    mapped = np.where(want_arg == len(idx), M * per_row,
                      rowptr[rows][:, None].astype(np.int64) + (want_arg - rp_sub[:-1][:, None]))
    assert_same_bits(C[rows_d.long()].cpu().numpy(), want, "C3 amax")
    assert np.array_equal(arg[rows_d.long()].cpu().numpy(), mapped)


def test_mean_and_sum(cmm, dev):
    for N, seed in ((1, 1), (33, 2), (256, 3), (602, 4)):
        M, K = 300, 900
        lens = mixed_lengths(M, seed)
        if N == 256:
            lens[10] = 20_000  # a long row: the sum path's split order, kept by mean
        rowptr, col, val = csr_rows(M, K, lens, seed=seed, replace=N == 256)
        K = max(K, int(col.max()) + 1)
        B = np.random.Generator(np.random.PCG64(seed)).standard_normal((K, N), dtype=np.float32)
        plain = torch.empty((M, N), device=dev)
        cmm.naive_spmm(torch.from_numpy(val).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(rowptr).to(dev),
                       len(val), M, K, torch.from_numpy(B).to(dev), plain)
        plain = plain.cpu().numpy()
        got_sum, _ = gpu_reduce(cmm, dev, rowptr, col, val, M, K, B, "sum", with_arg=False)
        assert_same_bits(got_sum, plain, f"sum N={N}")
        got_mean, _ = gpu_reduce(cmm, dev, rowptr, col, val, M, K, B, "mean", with_arg=False)
        cnt = np.diff(rowptr).astype(np.float32)[:, None]
        expect = np.where(cnt > 0, plain / np.maximum(cnt, np.float32(1)), np.float32(0)).astype(np.float32)
        assert_same_bits(got_mean, expect, f"mean N={N}")
        want, _ = torch_reduce(rowptr, col, val, M, K, B, "mean")
        assert np.allclose(got_mean, want, rtol=1e-5, atol=1e-6), f"mean N={N} vs torch"
        assert np.all(got_mean[lens == 0].view(np.int32) == 0), "empty rows give +0"


ATOL_GRAD = 1e-5  # gradients are sums of O(10) products of values of size O(1) in a different order than torch's


@pytest.mark.parametrize("reduce", ["sum", "mean", "amax", "amin"])
@pytest.mark.parametrize("N", [5, 64, 130])
def test_autograd_vs_torch_cpu_and_deterministic(dev, reduce, N):
    import matmuls
    M, K = 180, 260
    rowptr, col, val = csr_rows(M, K, mixed_lengths(M, N), seed=N, sort=True)
    g = np.random.Generator(np.random.PCG64(N + 50))
    B = g.standard_normal((K, N), dtype=np.float32)
    if reduce in ("amax", "amin"):
        B = g.integers(-3, 4, (K, N)).astype(np.float32)  # ties: the gradient goes to the selected entry only
    G = g.standard_normal((M, N), dtype=np.float32)

    def csr(device):
        return torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                       torch.from_numpy(val), (M, K), device=device).requires_grad_()

    a_cpu, b_cpu = csr("cpu"), torch.from_numpy(B).requires_grad_()
    torch.sparse.mm(a_cpu, b_cpu, reduce=reduce).backward(torch.from_numpy(G))
    runs = []
    for _ in range(2):
        a, b = csr(dev), torch.from_numpy(B).to(dev).requires_grad_()
        out = matmuls.sparse_mm_reduce(a, b, reduce)
        out.backward(torch.from_numpy(G).to(dev))
        assert a.grad.layout == torch.sparse_csr
        assert torch.equal(a.grad.crow_indices().cpu(), a_cpu.crow_indices())
        runs.append((out.detach().cpu().numpy(), a.grad.values().cpu().numpy(), b.grad.cpu().numpy()))
    want_out = torch.sparse.mm(a_cpu.detach(), b_cpu.detach(), reduce=reduce).numpy()
    assert np.allclose(runs[0][0], want_out, rtol=1e-5, atol=1e-6), reduce
    assert np.allclose(runs[0][1], a_cpu.grad.values().numpy(), rtol=1e-5, atol=ATOL_GRAD), f"{reduce}: grad of A's values"
    assert np.allclose(runs[0][2], b_cpu.grad.numpy(), rtol=1e-5, atol=ATOL_GRAD), f"{reduce}: grad of B"
    for x, y in zip(runs[0], runs[1]):
        assert_same_bits(x, y, f"{reduce}: second run")


def test_amax_backward_gathers_no_values(mm, cmm, dev, monkeypatch):
    """grad B of amax reads A's values through the kept permutation inside its kernel: the backward takes Aᵀ's pattern
    alone and gathers no copy of Aᵀ's values (the sum backward, which multiplies by them, does)."""
    M, K, N = 180, 260, 64
    rowptr, col, val = csr_rows(M, K, mixed_lengths(M, N), seed=9, sort=True)
    a = torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                torch.from_numpy(val), (M, K), device=dev).requires_grad_()
    b = torch.randn(K, N, device=dev, requires_grad=True)
    gathers = []
    real = cmm.gather_perm
    monkeypatch.setattr(cmm, "gather_perm", lambda *args: (gathers.append(1), real(*args))[1])
    mm.sparse_mm_reduce(a, b, "amax").sum().backward()
    assert a.grad is not None and b.grad is not None and not gathers
    mm.sparse_mm_reduce(a, b, "sum").sum().backward()
    assert len(gathers) == 1


def test_int32_indices_and_grad_of_one_operand(dev):
    import matmuls
    M, K, N = 50, 80, 16
    rowptr, col, val = csr_rows(M, K, mixed_lengths(M, 1) % 60, seed=1, sort=True)
    a = torch.sparse_csr_tensor(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), (M, K), device=dev)
    B = torch.randn(K, N, device=dev)
    want, _ = torch_reduce(rowptr, col, val, M, K, B.cpu().numpy(), "amin")
    assert_same_bits(matmuls.sparse_mm_reduce(a, B, "amin").cpu().numpy(), want, "int32 indices")
    b = B.clone().requires_grad_()
    matmuls.sparse_mm_reduce(a, b, "amax").sum().backward()
    assert b.grad is not None and b.grad.shape == (K, N)


def test_amax_with_arg_graph_capture_replays_the_eager_result(cmm, dev):
    M, K, N = 3000, 20_000, 64
    lens = np.full(M, 30, np.int64)
    lens[5] = 40_000  # a hub row: the follow-up launches are captured too
    rowptr, col, val = csr_rows(M, K, lens, seed=4, replace=True)
    B = torch.randn(K, N, device=dev)
    args = [torch.from_numpy(x).to(dev) for x in (val, col, rowptr)]
    C_eager, arg_eager = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev, dtype=torch.int32)
    cmm.naive_spmm_reduce(*args, len(val), M, K, B, C_eager, "amax", arg_eager)
    C, arg = torch.full((M, N), 7.0, device=dev), torch.full((M, N), -7, device=dev, dtype=torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cmm.naive_spmm_reduce(*args, len(val), M, K, B, C, "amax", arg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cmm.naive_spmm_reduce(*args, len(val), M, K, B, C, "amax", arg)
    C.fill_(7.0)
    arg.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(C.cpu().numpy(), C_eager.cpu().numpy(), "graph replay")
    assert torch.equal(arg, arg_eager)
