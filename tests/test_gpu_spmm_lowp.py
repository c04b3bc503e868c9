"""bfloat16 / float16 CSR × dense products and their autograd, on the MI355X.

The contract (include/mi_spmm.h, low-precision section): C = rne_T(C32), where C32 is what the fp32 product writes for
the exactly widened operands with long rows split (naive_spmm_ex(..., 1)).  So the witness of every forward here is the
fp32 GPU path on widened operands, narrowed by torch on the host; outputs are compared NaN by position and every other
value by its 16 bits (−0, ±inf, overflow and T's subnormals included).  The gradient of the values is rne_T of the fp32
SDDMM on widened operands, the gradient of B the low-precision product on Aᵀ.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 16, 31, 32, 33, 64, 100, 128, 130, 256, 257, 320, 512, 602, 768, 1024]


def csr_rows(K, lens, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = g.integers(0, K, int(lens.sum())).astype(np.int32)
    val = ((g.random(len(col), dtype=np.float32) - 0.5) * scale).astype(np.float32)
    return rowptr, col, val


def to_dev(dev, rowptr, col, val, dtype):
    return (torch.from_numpy(val).to(dtype).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(rowptr).to(dev))


def lowp_product(cmm, dev, vals, cols, offs, M, K, B, entry="naive_spmm", mode=None):
    C = torch.empty((M, B.shape[1]), device=dev, dtype=B.dtype)
    f = getattr(cmm, entry)
    if mode is None:
        f(vals, cols, offs, vals.numel(), M, K, B, C)
    else:
        f(vals, cols, offs, vals.numel(), M, K, B, C, mode)
    return C


def witness(cmm, dev, vals, cols, offs, M, K, B):
    '''rne_T of the fp32 product on widened operands (long rows split), the narrowing done by torch on the host.'''
    C32 = torch.empty((M, B.shape[1]), device=dev, dtype=torch.float32)
    cmm.naive_spmm_ex(vals.float(), cols, offs, vals.numel(), M, K, B.float(), C32, 1)
    return C32.cpu().to(B.dtype)


def assert_same_bits(got, want, what=""):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn), f"{what}: NaN positions differ ({torch.nonzero(gn != wn)[:5].tolist()})"
    gb, wb = got.view(torch.int16)[~gn], want.view(torch.int16)[~wn]
    bad = torch.nonzero(gb != wb).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} values differ, first got {got[~gn][bad[:5]].tolist()} "
                              f"want {want[~wn][bad[:5]].tolist()}")


# ---- 1. forward against the fp32 path ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_forward_bit_exact_against_the_fp32_path(cmm, dev, dtype):
    g = np.random.Generator(np.random.PCG64(7))
    M, K = 403, 1500
    lens = g.integers(0, 300, M)
    lens[::7] = 0  # empty rows
    lens[5] = 1
    rowptr, col, val = csr_rows(K, lens, seed=8)
    vals, cols, offs = to_dev(dev, rowptr, col, val, dtype)
    for N in WIDTHS:
        Bbig = (torch.rand((K, N + 3), generator=torch.Generator().manual_seed(N)) - 0.5).to(dtype).to(dev)
        for B, layout in ((Bbig[:, :N].contiguous(), "contiguous"), (Bbig[:, 1:N + 1], "offset view, ldb = N + 3")):
            want = witness(cmm, dev, vals, cols, offs, M, K, B)
            for entry, mode in (("naive_spmm", None), ("cusparse_mmul", None), ("naive_spmm_ex", 0),
                                ("naive_spmm_ex", 1), ("naive_spmm_ex", -1)):
                got = lowp_product(cmm, dev, vals, cols, offs, M, K, B, entry, mode)
                assert_same_bits(got, want, f"{dtype} N={N} {layout} {entry}({mode})")


# ---- 2. long rows -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_long_rows_split_like_the_fp32_path_and_the_oracle(cmm, dev, dtype, oracle_mod):
    K = 200_000
    long_lens = [8192, 8193, 40_000, 100_000, 1_000_000]
    lens = np.full(1200, 100)
    at = [3, 200, 501, 777, 1100]
    for i, n in zip(at, long_lens):
        lens[i] = n
    M = len(lens)
    rowptr, col, val = csr_rows(K, lens, seed=11)
    vals, cols, offs = to_dev(dev, rowptr, col, val, dtype)
    sample = np.array(sorted(set(at) | {0, 1, 2, 600, M - 1}))
    for N in (3, 64, 256):
        B = (torch.rand((K, N), generator=torch.Generator().manual_seed(N)) - 0.5).to(dtype).to(dev)
        want = witness(cmm, dev, vals, cols, offs, M, K, B)
        for entry, mode in (("naive_spmm", None), ("naive_spmm_ex", 1)):
            got = lowp_product(cmm, dev, vals, cols, offs, M, K, B, entry, mode)
            assert_same_bits(got, want, f"{dtype} long rows N={N} {entry}")
        # the sampled rows against the oracle's split rule on widened arrays, narrowed by torch
        sub_lens = lens[sample]
        sub_ptr = np.concatenate([[0], np.cumsum(sub_lens)]).astype(np.int32)
        idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in sample])
        wide_val = vals.float().cpu().numpy()[idx]
        ref = oracle_mod.spmm_csr_long(sub_ptr, col[idx], wide_val, len(sample), K, B.float().cpu().numpy())
        assert_same_bits(got.cpu()[torch.from_numpy(sample)], torch.from_numpy(ref).to(dtype), f"{dtype} N={N} vs oracle")


# ---- 3. special values --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_special_values_overflow_and_subnormals(cmm, dev, dtype):
    g = torch.Generator().manual_seed(5)
    M, K = 256, 300
    lens = np.random.Generator(np.random.PCG64(6)).integers(1, 40, M)
    rowptr, col, val = csr_rows(K, lens, seed=9)
    val = torch.from_numpy(val)
    specials = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])
    v = val.clone()
    v[::11] = specials[torch.randint(0, 5, v[::11].shape, generator=g)]
    for N in (3, 8, 64, 256, 33):
        B = torch.rand((K, N), generator=g) - 0.5
        B.view(-1)[::13] = specials[torch.randint(0, 5, B.view(-1)[::13].shape, generator=g)]
        big = 1e30 if dtype == torch.bfloat16 else 250.0          # products beyond T's range; fp16 sums beyond 65504
        tiny = 1e-20 if dtype == torch.bfloat16 else 2e-3          # products in T's subnormal range
        for scale_v, scale_b, what in ((1.0, 1.0, "specials"), (big, big, "overflow"), (tiny, tiny, "subnormal"),
                                       (-0.0, 1.0, "negative zero")):
            vv, BB = (v * scale_v).to(dtype), (B * scale_b).to(dtype)
            if what == "negative zero":
                vv = torch.full_like(vv, -0.0)
                BB = BB.abs()
            vals, cols, offs = vv.to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(rowptr).to(dev)
            Bd = BB.to(dev)
            want = witness(cmm, dev, vals, cols, offs, M, K, Bd)
            got = lowp_product(cmm, dev, vals, cols, offs, M, K, Bd)
            assert_same_bits(got, want, f"{dtype} N={N} {what}")


@pytest.mark.parametrize("dtype", LOWP)
def test_store_rounding_matches_torch_on_fp32_sums(cmm, dev, dtype):
    '''C = rne_T(a·b + c·d) for two-entry rows chosen so that the fp32 sums cover ties, overflow, NaN and subnormals.'''
    g = torch.Generator().manual_seed(3)
    M, K, N = 4096, 2, 8
    x = torch.empty(M * N).uniform_(-4, 4, generator=g) * torch.pow(2.0, torch.randint(-140 if dtype == torch.bfloat16 else -30,
                                                                                    120 if dtype == torch.bfloat16 else 18,
                                                                                    (M * N,), generator=g).float())
    hi = x.to(dtype).float()
    lo = ((x - hi) * 0.5).to(dtype).float()  # a second term that moves the sum towards the next representable value
    B = torch.stack([hi, lo.mul(2)]).reshape(2, M, N).permute(1, 0, 2)  # [M, 2, N]: each row sees its own two B rows
    # a block-diagonal A: row r holds entries (2r, 1.0) and (2r+1, 0.5) over a B of 2M rows
    rowptr = np.arange(0, 2 * M + 1, 2, dtype=np.int32)
    col = np.arange(2 * M, dtype=np.int32)
    val = torch.tensor([1.0, 0.5]).repeat(M).to(dtype)
    Bt = B.reshape(2 * M, N).to(dtype)
    vals, cols, offs = val.to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(rowptr).to(dev)
    got = lowp_product(cmm, dev, vals, cols, offs, M, 2 * M, Bt.to(dev))
    want = witness(cmm, dev, vals, cols, offs, M, 2 * M, Bt.to(dev))
    assert_same_bits(got, want, f"{dtype} rounding sweep")


# ---- 4. C3 at full size -------------------------------------------------------------------------------------------

def test_c3_bf16_full_size(cmm, dev):
    import synthetic
    M = K = 1 << 20
    N = 256
    rowptr, col, val = synthetic.make_csr(M, K, 1e-4, seed=0)
    B = torch.from_numpy(synthetic.make_dense(K, N, seed=1)).to(torch.bfloat16)
    vals, cols, offs = to_dev(dev, rowptr, col, val, torch.bfloat16)
    Bd = B.to(dev)
    got = lowp_product(cmm, dev, vals, cols, offs, M, K, Bd)
    want = witness(cmm, dev, vals, cols, offs, M, K, Bd)
    assert_same_bits(got, want, "C3 bf16")
    rows = np.sort(np.random.Generator(np.random.PCG64(4)).choice(M, 4096, replace=False))
    idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows])
    sub_ptr = np.concatenate([[0], np.cumsum(np.diff(rowptr)[rows])]).astype(np.int64)
    a = torch.sparse_csr_tensor(torch.from_numpy(sub_ptr), torch.from_numpy(col[idx].astype(np.int64)),
                                vals.cpu()[torch.from_numpy(idx)].float(), (len(rows), K))
    ref = (a @ B.float()).to(torch.bfloat16)
    torch.testing.assert_close(got.cpu()[torch.from_numpy(rows)].float(), ref.float(), rtol=1.6e-2, atol=1e-2)


# ---- 5. autograd --------------------------------------------------------------------------------------------------

def grads(mm, fn, a, b, g):
    a = a.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    out = fn(a, b)
    out.backward(g)
    return out.detach(), a.grad, b.grad


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [3, 64, 130, 256])
def test_autograd_bit_exact_and_close_to_torch(cmm, mm, dev, dtype, N):
    M, K = 700, 900
    lens = np.random.Generator(np.random.PCG64(N)).integers(0, 60, M)
    rowptr, col, val = csr_rows(K, lens, seed=21)
    # torch CSR wants unique, sorted columns per row: dedupe through a dense matrix
    dense = torch.zeros(M, K)
    rows = np.repeat(np.arange(M), lens)
    dense[torch.from_numpy(rows), torch.from_numpy(col.astype(np.int64))] = torch.from_numpy(val)
    a = dense.to(dtype).to_sparse_csr().to(dev)
    b = (torch.rand((K, N), generator=torch.Generator().manual_seed(1)) - 0.5).to(dtype).to(dev)
    g = (torch.rand((M, N), generator=torch.Generator().manual_seed(2)) - 0.5).to(dtype).to(dev)
    crow, ccol = a.crow_indices().int(), a.col_indices().int()
    nnz = a.values().numel()
    for fn in (mm.naiveSpMM.apply, mm.cusparseMM.apply):
        out, ga, gb = grads(mm, fn, a, b, g)
        assert out.dtype == dtype and ga.dtype == dtype and gb.dtype == dtype and ga.is_sparse_csr
        assert_same_bits(out, witness(cmm, dev, a.values(), ccol, crow, M, K, b), f"{dtype} N={N} forward")
        # values: rne_T of the fp32 SDDMM on widened operands
        want_gv = cmm.sddmm(ccol, crow, nnz, M, K, g.float(), b.float()).cpu().to(dtype)
        assert_same_bits(ga.values(), want_gv, f"{dtype} N={N} grad values")
        assert torch.equal(ga.crow_indices().cpu(), a.crow_indices().cpu())
        # B: the fp32 Aᵀ·g product (long rows split) on widened operands, narrowed
        at = a.float().cpu().t().to_sparse_csr()
        want_gb = witness(cmm, dev, at.values().to(dev).to(dtype), at.col_indices().int().to(dev),
                          at.crow_indices().int().to(dev), K, M, g)
        assert_same_bits(gb, want_gb, f"{dtype} N={N} grad B")
        # close to torch autograd of the dense fp32 product on widened operands
        ad = a.to_dense().float().requires_grad_(True)
        bd = b.float().requires_grad_(True)
        (ad @ bd).backward(g.float())
        tol = dict(rtol=2e-2, atol=2e-2) if dtype == torch.bfloat16 else dict(rtol=2e-3, atol=2e-3)
        mask = a.to_dense().float() != 0
        torch.testing.assert_close(ga.to_dense().float()[mask], ad.grad[mask], **tol)
        torch.testing.assert_close(gb.float(), bd.grad, **tol)
        # two runs, the same bits
        out2, ga2, gb2 = grads(mm, fn, a, b, g)
        assert_same_bits(out2, out, "rerun forward")
        assert_same_bits(ga2.values(), ga.values(), "rerun grad values")
        assert_same_bits(gb2, gb, "rerun grad B")


# ---- 6. torch.matmul shapes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_batched_b_and_vector_forward_and_backward(cmm, mm, dev, dtype):
    M, K, N = 300, 200, 40
    dense = (torch.rand(M, K, generator=torch.Generator().manual_seed(3)) < 0.05) * (torch.rand(M, K) - 0.5)
    a = dense.to(dtype).to_sparse_csr().to(dev)
    for b in ((torch.rand(3, K, N) - 0.5).to(dtype).to(dev), (torch.rand(K) - 0.5).to(dtype).to(dev)):
        g = (torch.rand(*((3, M, N) if b.dim() == 3 else (M,))) - 0.5).to(dtype).to(dev)
        out, ga, gb = grads(mm, mm.naiveSpMM.apply, a, b, g)
        ref = torch.matmul(a.to_dense().float(), b.float())
        assert out.shape == ref.shape and out.dtype == dtype
        tol = dict(rtol=2e-2, atol=2e-2) if dtype == torch.bfloat16 else dict(rtol=2e-3, atol=2e-3)
        torch.testing.assert_close(out.float(), ref, **tol)
        # forward bits: the 2-d product on the flattened operand
        flat = b.reshape(-1, K, N).permute(1, 0, 2).reshape(K, -1) if b.dim() == 3 else b.unsqueeze(-1)
        want = witness(cmm, dev, a.values(), a.col_indices().int(), a.crow_indices().int(), M, K, flat)
        want = want.view(M, -1, N).permute(1, 0, 2).reshape(out.shape) if b.dim() == 3 else want.squeeze(-1)
        assert_same_bits(out, want, f"{dtype} {b.dim()}-d B forward")
        assert gb.shape == b.shape and gb.dtype == dtype and ga.dtype == dtype
        bd = b.float().requires_grad_(True)
        ad = a.to_dense().float().requires_grad_(True)
        torch.matmul(ad, bd).backward(g.float())
        torch.testing.assert_close(gb.float(), bd.grad, **tol)
        mask = a.to_dense().float() != 0
        torch.testing.assert_close(ga.to_dense().float()[mask], ad.grad[mask], **tol)


# ---- 7. graph capture ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_graph_captured_forward_replays_to_the_eager_bits(cmm, dev, dtype):
    lens = np.full(500, 30)
    lens[7] = 20_000  # a long row: the split rule and its workspace under capture
    K, N = 30_000, 256
    rowptr, col, val = csr_rows(K, lens, seed=31)
    vals, cols, offs = to_dev(dev, rowptr, col, val, dtype)
    M = len(lens)
    B = (torch.rand((K, N)) - 0.5).to(dtype).to(dev)
    eager = lowp_product(cmm, dev, vals, cols, offs, M, K, B)
    C = torch.empty_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cmm.naive_spmm(vals, cols, offs, vals.numel(), M, K, B, C)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    C.zero_()
    with torch.cuda.graph(graph):
        cmm.naive_spmm(vals, cols, offs, vals.numel(), M, K, B, C)
    C.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(C, eager, f"{dtype} graph replay")
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(C, eager, f"{dtype} second replay")


# ---- 8. refusals on the device ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_refusals_on_the_device(cmm, mm, dev, dtype):
    name = str(dtype).replace("torch.", "")
    a = (torch.rand(6, 5) < 0.5).float().to(dtype).to_sparse_csr().to(dev)
    b = torch.rand(5, 3).to(dtype).to(dev)
    for f in (mm.naiveSpMM.apply, mm.cusparseMM.apply, mm.naive_matmul, mm.sparse_matmul):
        with pytest.raises(RuntimeError, match=name):
            f(a, b.float())
        with pytest.raises(RuntimeError, match=rf"batched.*{name}"):
            f(torch.rand(2, 6, 5).to(dtype).to_sparse_csr().to(dev), b)
        with pytest.raises(RuntimeError, match=rf"dense.*{name}"):
            f(torch.rand(6, 5).to(dtype).to(dev), b)
    vals, cols, offs = a.values(), a.col_indices().int(), a.crow_indices().int()
    C = torch.empty(6, 3, device=dev, dtype=dtype)
    with pytest.raises(RuntimeError, match="(?s)(?=.*Float)(?=.*" + ("BFloat16" if dtype == torch.bfloat16 else "Half") + ")"):
        cmm.naive_spmm(vals.float(), cols, offs, vals.numel(), 6, 5, b, C)
    with pytest.raises(RuntimeError, match="float32"):  # double stays refused the fp32 way
        cmm.naive_spmm(vals.double(), cols, offs, vals.numel(), 6, 5, b.double(), C.double())
