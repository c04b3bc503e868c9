"""Pins the CPU oracle (oracle/spmm_oracle.c) — runs without a GPU.

The reference's own tests hold no stored vectors; their expectation is
torch.matmul(a, b) under torch.allclose defaults (rtol 1e-5, atol 1e-8;
reference tests/naive_kernel_test.py:30,36-37, tests/cusparse_kernel_test.py:53,58).
These tests check the oracle against that expectation: on the committed fixtures
(tests/golden/golden_v1.npz, generated from torch-CPU by make_golden.py) and on
the reference tests' shape list evaluated live with torch-CPU.
"""
import numpy as np
import pytest
import torch

RTOL, ATOL = 1e-5, 1e-8  # torch.allclose defaults, the reference tests' criterion


def close(a, b):
    return np.allclose(a, b, rtol=RTOL, atol=ATOL)


def test_spmm_matches_golden(oracle_mod, golden):
    for name in golden.cases("spmm"):
        c = golden.case(name)
        M, K = c["a"].shape
        got = oracle_mod.spmm_csr(c["rowptr"], c["col"], c["val"], M, K, c["b"])
        assert got.shape == c["c"].shape, name
        assert close(got, c["c"]), name
        assert np.array_equal(oracle_mod.spmm_csr_omp(c["rowptr"], c["col"], c["val"], M, K, c["b"]), got), name


def test_spmm_gradients_match_golden(oracle_mod, golden):
    """grad_b = Aᵀ·dC through the oracle's CSR transpose + SpMM; grad_a = dC·Bᵀ (dense)."""
    for name in golden.cases("spmm"):
        c = golden.case(name)
        if "dc" not in c:
            continue
        M, K = c["a"].shape
        t_rp, t_col, t_val = oracle_mod.csr_transpose(c["rowptr"], c["col"], c["val"], M, K)
        gb = oracle_mod.spmm_csr(t_rp, t_col, t_val, K, M, c["dc"])
        assert close(gb, c["grad_b"]), name
        ga = oracle_mod.gemm(c["dc"], c["b"], False, True)
        assert close(ga, c["grad_a"]), name
        # SDDMM = grad_a sampled on A's pattern
        rows = np.repeat(np.arange(M), np.diff(c["rowptr"]))
        assert close(oracle_mod.sddmm(c["rowptr"], c["col"], M, c["dc"], c["b"]), c["grad_a"][rows, c["col"]]), name


def test_gemm_matches_golden(oracle_mod, golden):
    for name in golden.cases("gemm"):
        c = golden.case(name)
        ta, tb = (bool(x) for x in c["flags"])
        a, b = c["a"], c["b"]
        if a.ndim != b.ndim:  # fc_3d_x_wt: broadcast the 2-d weight like torch.matmul
            b = np.broadcast_to(b, a.shape[:-2] + b.shape).copy()
        got = oracle_mod.gemm(a, b, ta, tb)
        assert got.shape == c["c"].shape, name
        assert close(got, c["c"]), name


def test_colmajor_matches_golden(oracle_mod, golden):
    c = golden.case("colmajor/fc")
    M, K = c["a"].shape
    N = c["x"].shape[0]
    y = oracle_mod.spmm_csr_colmajor(c["rowptr"], c["col"], c["val"], M, K, N, c["x"]).reshape(N, M)
    assert close(y, c["y"])
    # and it is the same arithmetic as the row-major form on transposed operands
    ref = oracle_mod.spmm_csr(c["rowptr"], c["col"], c["val"], M, K, np.ascontiguousarray(c["x"].T))
    assert np.array_equal(y, ref.T)


def test_coo_to_csr_matches_golden(oracle_mod, golden):
    c = golden.case("coo")
    rp, col, val = oracle_mod.coo_to_csr(c["a"].shape[0], c["row"], c["col"], c["val"])
    assert np.array_equal(rp, c["rowptr"]) and np.array_equal(col, c["csr_col"]) and np.array_equal(val, c["csr_val"])
    with pytest.raises(ValueError):
        oracle_mod.coo_to_csr(c["a"].shape[0], c["row"][::-1].copy(), c["col"], c["val"])


def test_dense_to_csr_is_torch_to_sparse_csr(oracle_mod, golden):
    """Integer artefacts bit-exact: same arrays as get_sparse_tensor_properties extracts."""
    for name in golden.cases("spmm"):
        c = golden.case(name)
        rp, col, val = oracle_mod.dense_to_csr(c["a"])
        assert np.array_equal(rp.reshape(-1), c["rowptr"]), name
        assert np.array_equal(col, c["col"]) and np.array_equal(val, c["val"]), name
    c = golden.case("batched/bert")
    rp, col, val = oracle_mod.dense_to_csr(c["a"])
    a = c["a"].reshape(-1, *c["a"].shape[-2:])
    base = 0
    for i in range(a.shape[0]):
        s = torch.from_numpy(a[i]).to_sparse_csr()
        assert np.array_equal(rp[i] - base, s.crow_indices().numpy())
        n = s.values().numel()
        assert np.array_equal(col[base:base + n], s.col_indices().numpy())
        base += n
    assert base == len(val)


def test_batched_matches_golden(oracle_mod, golden):
    c = golden.case("batched/bert")
    a = c["a"]
    batch = int(np.prod(a.shape[:-2]))
    rp, col, val = oracle_mod.dense_to_csr(a)
    got = oracle_mod.spmm_csr_batched(rp, col, val, batch, a.shape[-2], a.shape[-1],
                                      c["b"].reshape(batch, *c["b"].shape[-2:]))
    assert close(got.reshape(c["c"].shape), c["c"])


def test_csr_transpose_against_scipy(oracle_mod):
    import scipy.sparse as sp
    rp, col, val = oracle_mod.make_csr(300, 170, 0.05, 7)
    t_rp, t_col, t_val = oracle_mod.csr_transpose(rp, col, val, 300, 170)
    ref = sp.csr_matrix((val, col, rp), shape=(300, 170)).T.tocsr()
    ref.sort_indices()
    assert np.array_equal(t_rp, ref.indptr) and np.array_equal(t_col, ref.indices) and np.array_equal(t_val, ref.data)


@pytest.mark.parametrize("a_shape,b_shape,density", [
    # reference tests/cusparse_kernel_test.py:32-38 (≈10 % dense A), full sizes
    ((10, 10), (10, 10), 0.1), ((10, 20), (20, 10), 0.1), ((10, 10), (10, 5), 0.1), ((20, 10), (10, 5), 0.1),
    ((512, 1024), (1024, 256), 0.1),
    # reference tests/naive_kernel_test.py:62 (torch.rand: 100 % dense "sparse" A)
    ((4, 2), (2, 3), 1.0),
    # reference tests/tiledsppm_kernel_test.py:34-39 at n = 128 instead of 1024
    ((128, 128), (128, 128), 0.02), ((128, 256), (256, 128), 0.02), ((256, 128), (128, 64), 0.02),
])
def test_spmm_equals_torch_matmul_on_reference_shapes(oracle_mod, a_shape, b_shape, density):
    g = torch.Generator().manual_seed(hash((a_shape, b_shape)) % (2 ** 31))
    a = torch.rand(a_shape, generator=g) * (torch.rand(a_shape, generator=g) < density)
    b = torch.rand(b_shape, generator=g)
    expected = torch.matmul(a, b).numpy()
    rp, col, val = oracle_mod.dense_to_csr(a.numpy())
    got = oracle_mod.spmm_csr(rp.reshape(-1), col, val, a_shape[0], a_shape[1], b.numpy())
    assert got.shape == expected.shape and close(got, expected)


@pytest.mark.parametrize("a_shape,b_shape,tb", [
    # reference tests/naive_kernel_test.py:63-64 and the BERT shapes of :67-68 /
    # tests/cublas_kernel_test.py:68-69 with the batch cut from 256·16 / 16·16 to 2·2
    ((2, 4, 2), (2, 2, 3), False), ((2, 4, 2), (2, 4, 2), True),
    ((2, 2, 512, 512), (2, 2, 512, 64), False), ((2, 2, 512, 64), (2, 2, 512, 64), True),
])
def test_gemm_equals_torch_matmul_on_reference_shapes(oracle_mod, a_shape, b_shape, tb):
    g = torch.Generator().manual_seed(5)
    a, b = torch.rand(a_shape, generator=g), torch.rand(b_shape, generator=g)
    expected = torch.matmul(a, b.transpose(-1, -2) if tb else b).numpy()
    got = oracle_mod.gemm(a.numpy(), b.numpy(), False, tb)
    assert got.shape == expected.shape and close(got, expected)


def test_pinned_generator_is_stable(oracle_mod):
    """SURVEY.md §8(d) generator: fixed seed → fixed arrays (recorded digest)."""
    import hashlib
    rp, col, val = oracle_mod.make_csr(1024, 1024, 1e-2, 0)
    assert rp[-1] == len(col) == len(val)
    assert rp.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
    assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(0, 1024, 37))  # sorted, unique
    digest = hashlib.sha256(rp.tobytes() + col.tobytes() + val.tobytes()).hexdigest()
    assert digest == PINNED_DIGEST, digest
    # bench.py's generator (product side, no oracle import) is the same function
    import synthetic
    rp2, col2, val2 = synthetic.make_csr(1024, 1024, 1e-2, 0)
    assert np.array_equal(rp, rp2) and np.array_equal(col, col2) and np.array_equal(val, val2)
    assert np.array_equal(synthetic.make_dense(7, 5, 1), np.random.Generator(np.random.PCG64(1)).random((7, 5), dtype=np.float32))


PINNED_DIGEST = "79ff35ca20d2cd54c4a2c59f975a106bd2463ffeb37eb5cbc058671113352e84"


def test_long_row_rule_is_a_reassociation_only(oracle_mod):
    """Rows of more than 8192 non-zeros (mi_spmm_csr_ws_f32's 16-chain order): same product within
    the reference tolerance, identical bits for every shorter row."""
    M, K, N = 6, 20000, 24
    g = np.random.Generator(np.random.PCG64(3))
    lens = [20000, 8193, 8192, 0, 17, 12000]
    cols = [np.sort(g.choice(K, size=n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate(cols)
    val = g.random(len(col), dtype=np.float32)
    B = g.random((K, N), dtype=np.float32)
    plain = oracle_mod.spmm_csr(rowptr, col, val, M, K, B)
    long_ = oracle_mod.spmm_csr_long(rowptr, col, val, M, K, B)
    assert np.array_equal(plain[[2, 3, 4]], long_[[2, 3, 4]])
    assert not np.array_equal(plain[0], long_[0])  # really a different order …
    assert np.allclose(plain, long_, rtol=1e-5, atol=1e-8)  # … of the same sum
    A = torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                torch.from_numpy(val), (M, K))
    assert np.allclose((A @ torch.from_numpy(B)).numpy(), long_, rtol=1e-5, atol=1e-8)


def test_long_row_rule_split_rows(oracle_mod):
    """Rows of ≥ 65536 non-zeros use S = len/32768 groups of 16 chains (mi_spmm_csr_ws_f32): still
    only a reassociation, and restated here chunk by chunk in numpy for one column."""
    M, K, N = 3, 140000, 5  # N >= 4: below that the narrow-N rule applies instead
    g = np.random.Generator(np.random.PCG64(5))
    lens = [131072, 65535, 70000]
    cols = [np.sort(g.choice(K, size=n, replace=False)).astype(np.int32) for n in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate(cols)
    val = g.random(len(col), dtype=np.float32) - 0.5
    B = g.random((K, N), dtype=np.float32)
    long_ = oracle_mod.spmm_csr_long(rowptr, col, val, M, K, B)
    exact = np.stack([val[rowptr[r]:rowptr[r + 1]].astype(np.float64) @ B[col[rowptr[r]:rowptr[r + 1]]].astype(np.float64)
                      for r in range(M)])
    assert np.allclose(long_, exact, rtol=1e-4, atol=1e-3)
    # independent restatement of the rule for row 0 (S = 4), column 1
    s, e = int(rowptr[0]), int(rowptr[1])
    S = min(128, max(1, (e - s) >> 15))
    assert S == 4
    prods_v, prods_b = val[s:e], B[col[s:e], 1]
    chains = []
    for q in range(16 * S):
        acc = np.float32(0)
        for cb in range(q * 1024, e - s, 16 * S * 1024):
            for p in range(cb, min(cb + 1024, e - s)):
                acc = np.float32(np.float64(prods_v[p]) * np.float64(prods_b[p]) + np.float64(acc))  # fma: one rounding
        chains.append(acc)
    tot = None
    for gi in range(S):
        grp = chains[16 * gi]
        for w in range(1, 16):
            grp = np.float32(grp + chains[16 * gi + w])
        tot = grp if tot is None else np.float32(tot + grp)
    assert tot == long_[0, 1]


def test_gemm_split_k_order_matches_the_v2_golden(oracle_mod):
    """Round 6: the dense product's split-k order (few output tiles, k >= 4096: S equal k-ranges added in index order — what
    custom_mm.cublas_mmul computes) against fixtures generated from torch-CPU by tests/golden/make_golden_v2.py: within the
    reference tests' criterion (torch.allclose defaults, tests/cublas_kernel_test.py:27-28) of torch's fp32 product, and of the
    fp64 product; the plain chain too; and the rule really splits these shapes."""
    from pathlib import Path
    data = np.load(Path(__file__).resolve().parent / "golden" / "golden_v2.npz")
    names = [str(n) for n in data["__names__"]]
    assert len(names) == 4
    for name in names:
        a, b = data[name + "/a_u8"].astype(np.float32) / 256.0, data[name + "/b_u8"].astype(np.float32) / 256.0
        ta, tb = bool(data[name + "/transa"]), bool(data[name + "/transb"])
        m, k = (a.shape[1], a.shape[0]) if ta else a.shape
        n = b.shape[0] if tb else b.shape[1]
        S = oracle_mod.gemm_split_count(m, n, k)
        assert S > 1 and k % (32 * S) == 0, (name, S)
        split = oracle_mod.gemm(a, b, ta, tb)
        chain = oracle_mod.gemm(a, b, ta, tb, split=False)
        assert not np.array_equal(split, chain)
        for got in (split, chain):
            assert np.allclose(got, data[name + "/c"], rtol=1e-5, atol=1e-8), name
            assert np.allclose(got, data[name + "/c_fp64"], rtol=1e-5, atol=1e-8), name


# ---- the gradient restatements of amax / amin (oracle.reduce_grad_val / reduce_grad_b) -------------------------------

def _reduce_case(M, K, N, seed, integer=False):
    """A CSR with empty rows, empty columns, rows of 1 … 150 entries and a few duplicate / unsorted columns; B, G."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens = g.integers(0, 150, M)
    lens[::5] = 0
    lens[1] = 1
    used = np.arange(K)[g.random(K) < 0.8]  # the other columns stay empty: their rows of grad B must be +0
    col = np.concatenate([g.choice(used, int(n)) for n in lens]).astype(np.int32)  # with replacement: duplicates
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    if integer:  # nonzero small integers: every product and every partial sum is exact in fp32
        pick = lambda *s: (g.integers(1, 4, s) * g.choice([-1, 1], s)).astype(np.float32)  # noqa: E731
        val, B, G = pick(len(col)), pick(K, N), pick(M, N)
    else:
        val = g.standard_normal(len(col), dtype=np.float32)
        B, G = g.standard_normal((K, N), dtype=np.float32), g.standard_normal((M, N), dtype=np.float32)
    return rowptr, col, val, B, G


def _torch_csr(rowptr, col, val, M, K):
    return torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                   torch.from_numpy(val), (M, K))


@pytest.mark.parametrize("reduce", ["amax", "amin"])
@pytest.mark.parametrize("N", [1, 3, 5, 64, 65, 130, 1100])
def test_reduce_grad_restatements_within_float64_bound(oracle_mod, reduce, N):
    from gpu_helpers import assert_within_gamma_bound, select_grads_f64
    M, K = 120, 90
    rowptr, col, val, B, G = _reduce_case(M, K, N, seed=N)
    _, arg = torch.ops.aten._sparse_mm_reduce_impl(_torch_csr(rowptr, col, val, M, K).requires_grad_(),
                                                  torch.from_numpy(B), reduce)
    arg = arg.numpy()
    gv = oracle_mod.reduce_grad_val(rowptr, col, M, B, G, arg)
    gb = oracle_mod.reduce_grad_b(rowptr, col, val, M, K, G, arg)
    ref_v, abs_v, ref_b, abs_b = select_grads_f64(rowptr, col, val, M, K, B, G, arg)
    assert_within_gamma_bound(gv, ref_v, abs_v, N, f"{reduce} N={N} grad_val")
    assert_within_gamma_bound(gb, ref_b, abs_b, int(np.bincount(col, minlength=K).max()), f"{reduce} N={N} grad_B")
    empty = np.bincount(col, minlength=K) == 0
    assert empty.any() and np.all(gb[empty].view(np.int32) == 0), "empty columns of A give +0 rows of grad B"


@pytest.mark.parametrize("reduce", ["sum", "amax", "amin"])
@pytest.mark.parametrize("N", [1, 3, 64, 65, 130, 1100])
def test_gradient_restatements_equal_torch_autograd_on_exact_integers(oracle_mod, reduce, N):
    """On nonzero small-integer operands every sum is exact, whatever its order: the restatements (amax / amin) and the
    sum's composition (SDDMM; the product on the stable transpose) must give torch-CPU autograd's bits exactly."""
    from gpu_helpers import assert_same_bits
    M, K = 120, 90
    rowptr, col, val, B, G = _reduce_case(M, K, N, seed=100 + N, integer=True)
    a = _torch_csr(rowptr, col, val, M, K).requires_grad_()
    b = torch.from_numpy(B).requires_grad_()
    torch.sparse.mm(a, b, reduce=reduce).backward(torch.from_numpy(G))
    if reduce == "sum":
        gv = oracle_mod.sddmm(rowptr, col, M, G, B)
        t_rp, t_col, t_val = oracle_mod.csr_transpose(rowptr, col, val, M, K)
        gb = oracle_mod.spmm_csr_long(t_rp, t_col, t_val, K, M, G)
    else:
        _, arg = torch.ops.aten._sparse_mm_reduce_impl(_torch_csr(rowptr, col, val, M, K).requires_grad_(),
                                                  torch.from_numpy(B), reduce)
        gv = oracle_mod.reduce_grad_val(rowptr, col, M, B, G, arg.numpy())
        gb = oracle_mod.reduce_grad_b(rowptr, col, val, M, K, G, arg.numpy())
    assert_same_bits(gv, a.grad.values().detach(), f"{reduce} N={N} grad_val")
    assert_same_bits(gb, b.grad, f"{reduce} N={N} grad_B")
