"""Gradients of the CSR × dense products, bit for bit, on the MI355X.

Every case runs forward + backward through matmuls' autograd (naiveSpMM, cusparseMM, sparse_mm_reduce) and compares both
gradients with the CPU oracle's bits: NaN by position, every other value by its bits (−0 included).  The expectations:

  path                      grad of A's values                          grad of B
  fp32 sum                  oracle.sddmm(rowptr, col, M, g, B)          the oracle's product on oracle.csr_transpose(A)
  (naiveSpMM, cusparseMM,                                               with g: spmm_csr_long where the plan splits long
  sparse_mm_reduce 'sum')                                               rows (custom_mm.spmm_plan(nnz, K, M, g, gb)[3]),
                                                                        else spmm_csr
  bf16 / fp16 sum           rne_T of the fp32 row on exactly widened    rne_T of spmm_csr_long (N ≥ 4) or spmm_csr
                            operands (narrowed by torch on the host)    (N < 4) on widened Aᵀ values and g
  mean (fp32)               as fp32 sum with g′ = float32(g / count)    same
                            per row (rows without entries: g as is)
  amax / amin               oracle.reduce_grad_val on torch-CPU's arg   oracle.reduce_grad_b on torch-CPU's arg
                            (64 lane chains over j = 64t + l, then the  (one fmaf chain per (k, j) in Aᵀ order)
                            xor tree 32 … 1)

test_fp32_sum_gradients, test_lowp_sum_gradients, test_mean_gradients and test_amax_amin_gradients hold one row each, at
the widths below and on three row structures (rows of 0 … 200 entries; hub rows of 8193 and 40 000; hub columns of
8192, 8193, 40 000 and 10⁵ entries, i.e. long rows of Aᵀ), all with empty columns.  Besides the bits, every finite result
must lie within γ_n·Σ|terms| of a float64 reference (tests/gpu_helpers.assert_within_gamma_bound; + the store rounding in
bf16 / fp16), which catches a wrong formula the oracle composition and a kernel could share.  Further tests: a 10⁶-entry
column under amax, exact-integer hub cases of all four reductions against float64 torch-CPU autograd, operand layouts and
index dtypes, vector / batched mat2, three passes on one tensor (the Aᵀ schedule and the transposed-pattern cache), ±0 /
±inf / NaN, unsorted and duplicate columns, nnz = 0, and fp32 and low-precision products interleaved on one stream's
shared long-row workspace.
"""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits, assert_within_gamma_bound, select_grads_f64, sum_grads_f64

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 33, 64, 65, 128, 130, 256, 257, 512, 602, 1024, 1100]
LOWP = (torch.bfloat16, torch.float16)
STORE_U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
STORE_ABS = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}  # half of fp16's smallest subnormal


class Pattern:
    """A CSR pattern with fp32 values (host arrays) and its row and column counts."""

    def __init__(self, name, M, K, rows_cols, seed):
        g = np.random.Generator(np.random.PCG64(seed))
        lens = np.array([len(c) for c in rows_cols], np.int64)
        self.name, self.M, self.K = name, M, K
        self.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.col = (np.concatenate(rows_cols) if lens.sum() else np.zeros(0)).astype(np.int32)
        self.val = (g.random(len(self.col), dtype=np.float32) - 0.5).astype(np.float32)
        self.counts = np.bincount(self.col, minlength=K)
        self.row_counts = np.diff(self.rowptr)
        self.nnz = len(self.col)

    def with_values(self, val):
        p = object.__new__(Pattern)
        p.__dict__.update(self.__dict__)
        p.val = np.ascontiguousarray(val, np.float32)
        return p

    def csr(self, dev, dtype=torch.float32, index=torch.int64, grad=True):
        a = torch.sparse_csr_tensor(torch.from_numpy(self.rowptr).to(index), torch.from_numpy(self.col).to(index),
                                    torch.from_numpy(self.val).to(dtype), (self.M, self.K), device=dev)
        return a.requires_grad_() if grad else a

    def widened(self, dtype):
        return self if dtype == torch.float32 else self.with_values(torch.from_numpy(self.val).to(dtype).float().numpy())


def _sorted_rows(g, lens, choose_from):
    return [np.sort(g.choice(choose_from, int(n), replace=False)) for n in lens]


@functools.lru_cache(maxsize=None)
def pattern(name):
    g = np.random.Generator(np.random.PCG64(sum(map(ord, name))))
    if name == "rows":  # rows of 0, 1, 63, 64, 65 and 200 entries between short random ones; every 10th column empty
        M, K = 700, 2500
        lens = g.integers(0, 40, M)
        lens[::3] = np.resize([0, 1, 63, 64, 65, 200], len(lens[::3]))
        return Pattern(name, M, K, _sorted_rows(g, lens, np.arange(K)[np.arange(K) % 10 != 3]), 1)
    if name == "hub_rows":  # rows of 8193 and 40 000 entries (split in the forward; long SDDMM rows in the backward)
        M, K = 400, 48_000
        lens = g.integers(0, 30, M)
        lens[3], lens[9] = 8193, 40_000
        return Pattern(name, M, K, _sorted_rows(g, lens, np.arange(K - 1000)), 2)
    if name == "hub_cols":  # columns of 8192, 8193, 40 000 and 10⁵ entries: long rows of Aᵀ; columns ≥ 1400 empty
        M, K = 100_500, 1500
        hubs = {5: 8192, 6: 8193, 7: 40_000, 8: 100_000}
        rows = [[] for _ in range(M)]
        for c, n in hubs.items():
            for r in g.choice(M, n, replace=False):
                rows[r].append(c)
        for r in range(2000):
            rows[r].extend(g.choice(np.arange(10, 1400), int(g.integers(0, 20)), replace=False).tolist())
        return Pattern(name, M, K, [np.sort(np.array(r, np.int64)) for r in rows], 3)
    raise KeyError(name)


def operands(P, N, seed, dtype=torch.float32):
    """B [K, N] and G [M, N] in dtype (torch, host) and their exactly widened fp32 numpy forms."""
    g = torch.Generator().manual_seed(seed)
    B = (torch.rand((P.K, N), generator=g) * 2 - 1).to(dtype)
    G = (torch.rand((P.M, N), generator=g) * 2 - 1).to(dtype)
    return B, G, B.float().numpy(), G.float().numpy()


def grad_b_splits(cmm, dev, P, N):
    """Whether the fp32 plan of the grad-B product (Aᵀ [K, M] · g [M, N]) splits long rows."""
    g = torch.empty((P.M, N), device=dev)
    gb = torch.empty((P.K, N), device=dev)
    return bool(cmm.spmm_plan(P.nnz, P.K, P.M, g, gb)[3])


def sum_expect(oracle_mod, P, B, G, split):
    """(grad_val, grad_B) of the sum product in fp32 from the oracle: the SDDMM and the product on the stable transpose."""
    gv = oracle_mod.sddmm(P.rowptr, P.col, P.M, G, B)
    t_rp, t_col, t_val = oracle_mod.csr_transpose(P.rowptr, P.col, P.val, P.M, P.K)
    gb = (oracle_mod.spmm_csr_long if split else oracle_mod.spmm_csr)(t_rp, t_col, t_val, P.K, P.M, G)
    return gv, gb


def check_bound_sum(P, B, G, gv, gb, what, dtype=torch.float32, extra_terms=0):
    ref_v, abs_v, ref_b, abs_b = sum_grads_f64(P.rowptr, P.col, P.val, P.M, P.K, B, G)
    u, ab = STORE_U.get(dtype, 0.0), STORE_ABS.get(dtype, 0.0)
    assert_within_gamma_bound(gv, ref_v, abs_v, B.shape[1] + extra_terms, what + " grad_val (float64 bound)", u, ab)
    assert_within_gamma_bound(gb, ref_b, abs_b, int(P.counts.max(initial=0)) + extra_terms, what + " grad_B (float64 bound)",
                              u, ab)


def run_autograd(mm, dev, P, B, G, fn, dtype=torch.float32, index=torch.int64):
    a = P.csr(dev, dtype, index)
    b = B.to(dev).requires_grad_()
    out = fn(mm, a, b)
    out.backward(G.to(dev))
    assert a.grad.layout == torch.sparse_csr and tuple(a.grad.shape) == (P.M, P.K)
    assert torch.equal(a.grad.crow_indices().cpu().long(), torch.from_numpy(P.rowptr).long())
    assert a.grad.values().dtype == dtype and b.grad.dtype == dtype
    return a.grad.values().detach().cpu(), b.grad.detach().cpu()


ENTRIES = {
    "naiveSpMM": lambda mm, a, b: mm.naiveSpMM.apply(a, b),
    "cusparseMM": lambda mm, a, b: mm.cusparseMM.apply(a, b),
    "sparse_mm_reduce": lambda mm, a, b: mm.sparse_mm_reduce(a, b, "sum"),
}
CASES = [("rows", N) for N in WIDTHS] + [("hub_rows", N) for N in (3, 64, 130)] + [("hub_cols", N) for N in (2, 64, 257)]


# ---- 1. fp32 sum ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,N", CASES)
def test_fp32_sum_gradients(cmm, mm, dev, oracle_mod, name, N):
    P = pattern(name)
    B, G, Bn, Gn = operands(P, N, seed=N)
    want_v, want_b = sum_expect(oracle_mod, P, Bn, Gn, grad_b_splits(cmm, dev, P, N))
    entry = list(ENTRIES)[N % 3]
    gv, gb = run_autograd(mm, dev, P, B, G, ENTRIES[entry])
    assert_same_bits(gv, torch.from_numpy(want_v), f"{name} N={N} {entry} grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b), f"{name} N={N} {entry} grad_B")
    empty = P.counts == 0
    assert empty.any() and torch.all(gb[torch.from_numpy(empty)].view(torch.int32) == 0), "empty columns: +0 rows"
    check_bound_sum(P, Bn, Gn, gv.numpy(), gb.numpy(), f"{name} N={N}")


# ---- 2. bf16 / fp16 sum ----------------------------------------------------------------------------------------------

LOWP_CASES = CASES[:] + [("hub_cols", 3)]


@pytest.mark.parametrize("dtype", LOWP, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name,N", LOWP_CASES)
def test_lowp_sum_gradients(cmm, mm, dev, oracle_mod, dtype, name, N):
    P = pattern(name)
    B, G, Bn, Gn = operands(P, N, seed=N + 7, dtype=dtype)
    Pw = P.widened(dtype)
    want_v, want_b = sum_expect(oracle_mod, Pw, Bn, Gn, split=True)  # (N < 4: both oracle forms keep the narrow order)
    gv, gb = run_autograd(mm, dev, P, B, G, ENTRIES["naiveSpMM"], dtype)
    assert_same_bits(gv, torch.from_numpy(want_v).to(dtype), f"{dtype} {name} N={N} grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b).to(dtype), f"{dtype} {name} N={N} grad_B")
    check_bound_sum(Pw, Bn, Gn, gv.float().numpy(), gb.float().numpy(), f"{dtype} {name} N={N}", dtype)


# ---- 3. mean ---------------------------------------------------------------------------------------------------------

def mean_g(P, Gn):
    cnt = P.row_counts.astype(np.float32)[:, None]
    return np.where(cnt > 0, Gn / np.maximum(cnt, np.float32(1)), Gn).astype(np.float32)


@pytest.mark.parametrize("name,N", CASES)
def test_mean_gradients(cmm, mm, dev, oracle_mod, name, N):
    P = pattern(name)
    B, G, Bn, Gn = operands(P, N, seed=N + 11)
    Gm = mean_g(P, Gn)
    want_v, want_b = sum_expect(oracle_mod, P, Bn, Gm, grad_b_splits(cmm, dev, P, N))
    gv, gb = run_autograd(mm, dev, P, B, G, lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, "mean"))
    assert_same_bits(gv, torch.from_numpy(want_v), f"mean {name} N={N} grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b), f"mean {name} N={N} grad_B")
    cnt = P.row_counts.astype(np.float64)[:, None]
    check_bound_sum(P, Bn, np.where(cnt > 0, Gn / np.maximum(cnt, 1), Gn), gv.numpy(), gb.numpy(), f"mean {name} N={N}",
                    extra_terms=1)


# ---- 4. amax / amin --------------------------------------------------------------------------------------------------

def torch_arg(P, Bn, reduce):
    a = P.csr("cpu")
    _, arg = torch.ops.aten._sparse_mm_reduce_impl(a, torch.from_numpy(Bn), reduce)
    return arg.numpy()


def select_expect(oracle_mod, P, Bn, Gn, arg):
    return oracle_mod.reduce_grad_val(P.rowptr, P.col, P.M, Bn, Gn, arg), \
        oracle_mod.reduce_grad_b(P.rowptr, P.col, P.val, P.M, P.K, Gn, arg)


def check_bound_select(P, Bn, Gn, arg, gv, gb, what):
    ref_v, abs_v, ref_b, abs_b = select_grads_f64(P.rowptr, P.col, P.val, P.M, P.K, Bn, Gn, arg)
    assert_within_gamma_bound(gv, ref_v, abs_v, Bn.shape[1], what + " grad_val (float64 bound)")
    assert_within_gamma_bound(gb, ref_b, abs_b, int(P.counts.max(initial=0)), what + " grad_B (float64 bound)")


@pytest.mark.parametrize("reduce", ["amax", "amin"])
@pytest.mark.parametrize("name,N", CASES)
def test_amax_amin_gradients(mm, dev, oracle_mod, reduce, name, N):
    P = pattern(name)
    B, G, Bn, Gn = operands(P, N, seed=N + 13)
    arg = torch_arg(P, Bn, reduce)
    want_v, want_b = select_expect(oracle_mod, P, Bn, Gn, arg)
    gv, gb = run_autograd(mm, dev, P, B, G, lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, reduce))
    assert_same_bits(gv, torch.from_numpy(want_v), f"{reduce} {name} N={N} grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b), f"{reduce} {name} N={N} grad_B")
    check_bound_select(P, Bn, Gn, arg, gv.numpy(), gb.numpy(), f"{reduce} {name} N={N}")


def test_amax_column_of_a_million_entries(mm, dev, oracle_mod):
    """The hub-matrix backward's 10⁶-entry row of Aᵀ, left to one wave: its result, bit for bit."""
    g = np.random.Generator(np.random.PCG64(5))
    M, K, N = 1_000_000, 64, 64
    second = g.integers(1, K, M)
    rows = [np.array([0, second[r]]) if r % 3 == 0 else np.array([0]) for r in range(M)]
    P = Pattern("million", M, K, rows, 6)
    B, G, Bn, Gn = operands(P, N, seed=17)
    arg = torch_arg(P, Bn, "amax")
    want_v, want_b = select_expect(oracle_mod, P, Bn, Gn, arg)
    gv, gb = run_autograd(mm, dev, P, B, G, lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, "amax"))
    assert_same_bits(gv, torch.from_numpy(want_v), "amax 10⁶ column grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b), "amax 10⁶ column grad_B")
    check_bound_select(P, Bn, Gn, arg, gv.numpy(), gb.numpy(), "amax 10⁶ column")


# ---- 5. exact arithmetic on hubs: any order gives float64 torch-CPU autograd's value ------------------------------------

@functools.lru_cache(maxsize=None)
def exact_hub_pattern():
    g = np.random.Generator(np.random.PCG64(21))
    M, K = 41_000, 9000
    rows = [[] for _ in range(M)]
    rows[0] = list(range(100, 100 + 8193))  # a hub row
    for c, n in ((1, 40_000), (2, 8193)):  # hub columns
        for r in g.choice(np.arange(1, M), n, replace=False):
            rows[r].append(c)
    for r in range(1, 3000):
        rows[r].extend(g.choice(np.arange(10, 8000), int(g.integers(0, 12)), replace=False).tolist())
    P = Pattern("exact_hubs", M, K, [np.sort(np.array(r, np.int64)) for r in rows], 22)
    return P.with_values((g.integers(1, 3, P.nnz) * g.choice([-1, 1], P.nnz)).astype(np.float32))


@pytest.mark.parametrize("N", [3, 64])
@pytest.mark.parametrize("reduce", ["sum", "mean", "amax", "amin"])
def test_exact_integer_hubs_equal_float64_autograd(mm, dev, reduce, N):
    """Nonzero small integers, |partial sums| < 2²⁴: every sum is exact in fp32 whatever its order (for mean, each row of g
    is a multiple of the row's count, so g / count is exact too).  The mean's float64 reference is the sum's autograd on
    g / count: torch-CPU's own mean backward scales by a rounded reciprocal (1e-16 off where the exact value is 0)."""
    P = exact_hub_pattern()
    g = np.random.Generator(np.random.PCG64(N))
    Bn = (g.integers(1, 4, (P.K, N)) * g.choice([-1, 1], (P.K, N))).astype(np.float32)
    Gn = (g.integers(1, 4, (P.M, N)) * g.choice([-1, 1], (P.M, N))).astype(np.float32)
    if reduce == "mean":
        Gn = (Gn * np.maximum(P.row_counts, 1)[:, None]).astype(np.float32)
    a64 = torch.sparse_csr_tensor(torch.from_numpy(P.rowptr).long(), torch.from_numpy(P.col).long(),
                                  torch.from_numpy(P.val).double(), (P.M, P.K)).requires_grad_()
    b64 = torch.from_numpy(Bn).double().requires_grad_()
    G64 = torch.from_numpy(Gn).double()
    if reduce == "mean":
        G64 = G64 / torch.from_numpy(np.maximum(P.row_counts, 1)).double()[:, None]  # exact: integer quotients
    torch.sparse.mm(a64, b64, reduce="sum" if reduce == "mean" else reduce).backward(G64)
    gv, gb = run_autograd(mm, dev, P, torch.from_numpy(Bn), torch.from_numpy(Gn),
                          lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, reduce))
    assert_same_bits(gv, a64.grad.values().float(), f"{reduce} N={N} grad_val")
    assert_same_bits(gb, b64.grad.float(), f"{reduce} N={N} grad_B")


# ---- 6. layouts --------------------------------------------------------------------------------------------------------

def _mat2(B, layout, dev):
    """(leaf, mat2 view, how to read mat2's gradient from the leaf's)."""
    K, N = B.shape
    if layout == "contiguous":
        leaf = B.to(dev).requires_grad_()
        return leaf, leaf, lambda gr: gr
    if layout == "transposed":
        leaf = B.t().contiguous().to(dev).requires_grad_()
        return leaf, leaf.t(), lambda gr: gr.t()
    big = torch.zeros((K, N + 2), dtype=B.dtype)
    big[:, 1:N + 1] = B
    leaf = big.to(dev).requires_grad_()  # a column slice one element in: ldb = N + 2 = 67, odd
    assert leaf[:, 1:N + 1].stride(0) % 2 == 1
    return leaf, leaf[:, 1:N + 1], lambda gr: gr[:, 1:N + 1]


@pytest.mark.parametrize("index", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("glayout", ["contiguous", "expanded", "transposed"])
@pytest.mark.parametrize("blayout", ["contiguous", "transposed", "slice"])
@pytest.mark.parametrize("path", ["fp32", "bf16", "amax"])
def test_layouts(cmm, mm, dev, oracle_mod, path, blayout, glayout, index):
    P = pattern("hub_rows")
    N = 65
    dtype = torch.bfloat16 if path == "bf16" else torch.float32
    B, G, Bn, Gn = operands(P, N, seed=3, dtype=dtype)
    if glayout == "expanded":
        G = torch.ones((P.M, N), dtype=dtype)
        Gn = G.float().numpy()
    leaf, b, grad_of = _mat2(B, blayout, dev)
    a = P.csr(dev, dtype, index)
    out = mm.sparse_mm_reduce(a, b, "amax") if path == "amax" else mm.naiveSpMM.apply(a, b)
    if glayout == "expanded":
        out.sum().backward()
    elif glayout == "transposed":
        out.backward(G.t().contiguous().to(dev).t())
    else:
        out.backward(G.to(dev))
    gv, gb = a.grad.values().detach().cpu(), grad_of(leaf.grad).detach().cpu()
    what = f"{path} mat2 {blayout} grad_output {glayout} {index}"
    if path == "amax":
        arg = torch_arg(P, Bn, "amax")
        want_v, want_b = select_expect(oracle_mod, P, Bn, Gn, arg)
    else:
        Pw = P.widened(dtype)
        want_v, want_b = sum_expect(oracle_mod, Pw, Bn, Gn, True if dtype != torch.float32 else grad_b_splits(cmm, dev, P, N))
    assert_same_bits(gv, torch.from_numpy(want_v).to(dtype), what + " grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b).to(dtype), what + " grad_B")
    if path == "amax":
        check_bound_select(P, Bn, Gn, arg, gv.numpy(), gb.numpy(), what)
    else:
        check_bound_sum(P.widened(dtype), Bn, Gn, gv.float().numpy(), gb.float().numpy(), what, dtype)
    if blayout == "slice":
        rest = torch.cat([leaf.grad[:, :1], leaf.grad[:, N + 1:]], 1).cpu()
        assert torch.all(rest == 0), "columns outside the slice get no gradient"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", ["vector", "batched"])
def test_vector_and_batched_mat2(cmm, mm, dev, oracle_mod, dtype, shape):
    """A 1-d mat2 and a [2, 3, K, N] mat2, checked on the flattened form _sparse_backward uses (B → [K, items·N] item-major)."""
    P = pattern("hub_cols")
    N = 1 if shape == "vector" else 5
    items = 1 if shape == "vector" else 6
    g = torch.Generator().manual_seed(29)
    Bf = (torch.rand((P.K, items * N), generator=g) * 2 - 1).to(dtype)
    Gf = (torch.rand((P.M, items * N), generator=g) * 2 - 1).to(dtype)
    if shape == "vector":
        B, G = Bf[:, 0].contiguous(), Gf[:, 0].contiguous()
    else:
        B = Bf.view(P.K, items, N).permute(1, 0, 2).reshape(2, 3, P.K, N).contiguous()
        G = Gf.view(P.M, items, N).permute(1, 0, 2).reshape(2, 3, P.M, N).contiguous()
    Pw = P.widened(dtype)
    split = True if dtype != torch.float32 else grad_b_splits(cmm, dev, P, items * N)
    want_v, want_b = sum_expect(oracle_mod, Pw, Bf.float().numpy(), Gf.float().numpy(), split)
    gv, gb = run_autograd(mm, dev, P, B, G, ENTRIES["naiveSpMM"], dtype)
    flat_gb = gb.reshape(P.K) if shape == "vector" else gb.reshape(items, P.K, N).permute(1, 0, 2).reshape(P.K, items * N)
    assert_same_bits(gv, torch.from_numpy(want_v).to(dtype), f"{shape} {dtype} grad_val")
    assert_same_bits(flat_gb, torch.from_numpy(want_b).to(dtype).reshape(flat_gb.shape), f"{shape} {dtype} grad_B")
    check_bound_sum(Pw, Bf.float().numpy(), Gf.float().numpy(), gv.float().numpy(),
                    flat_gb.float().numpy().reshape(P.K, items * N), f"{shape} {dtype}", dtype)


# ---- 7. repeats: plain, then the Aᵀ schedule is built, then it is used ---------------------------------------------------

@pytest.mark.parametrize("name", ["hub_cols", "hub_rows"])
def test_three_passes_on_one_tensor_share_its_csr_state(cmm, mm, dev, oracle_mod, monkeypatch, name):
    """Pass 1 runs plain and marks the pattern; pass 2 builds the Aᵀ row schedule; pass 3 finds it kept on the tensor.  On
    hub_cols (Aᵀ rows of up to 10⁵ entries) the schedule is active, so grad B of passes 2 and 3 comes from
    naive_spmm_scheduled; on hub_rows (Aᵀ rows of a few entries) the inspector finds no skew and the plain product runs.
    Every pass also reuses the transposed pattern kept on the tensor, and gives the oracle's bits."""
    P = pattern(name)
    N = 64
    scheduled_grad_b = []
    real = cmm.naive_spmm_scheduled

    def counting(sched, *args, **kw):
        if args[4] == P.K and args[5] == P.M:  # (A_values, A_columns, A_offsets, nnz, rows, cols, …): a product on Aᵀ
            scheduled_grad_b.append(sched)
        return real(sched, *args, **kw)

    monkeypatch.setattr(cmm, "naive_spmm_scheduled", counting)
    a = P.csr(dev)
    cache = None
    for rep in range(3):
        B, G, Bn, Gn = operands(P, N, seed=40 + rep)
        want_v, want_b = sum_expect(oracle_mod, P, Bn, Gn, grad_b_splits(cmm, dev, P, N))
        a.grad = None
        b = B.to(dev).requires_grad_()
        mm.naiveSpMM.apply(a, b).backward(G.to(dev))
        assert_same_bits(a.grad.values(), torch.from_numpy(want_v), f"{name} pass {rep} grad_val")
        assert_same_bits(b.grad, torch.from_numpy(want_b), f"{name} pass {rep} grad_B")
        check_bound_sum(P, Bn, Gn, a.grad.values().cpu().numpy(), b.grad.cpu().numpy(), f"{name} pass {rep}")
        state = getattr(a, "_mi_state", None)
        assert state is not None and state.transposed is not None, "the transposed pattern is kept on the tensor"
        _, t_col, _ = state.transposed
        assert cache is None or t_col is cache, "later passes reuse the kept transposed pattern"
        cache = t_col
        book = state.sched_t
        assert N in book
        if rep == 0:
            assert book[N] == "seen" and not scheduled_grad_b, "the first backward runs plain"
            continue
        ent = book[N]
        assert ent != "seen", "the second backward builds the Aᵀ schedule"
        if name == "hub_cols":
            assert ent.info()["active"], "hub columns: the Aᵀ schedule is active"
            assert len(scheduled_grad_b) == rep and scheduled_grad_b[-1] is ent, f"pass {rep}: grad B ran on the schedule"
        else:
            assert not scheduled_grad_b, "no skew in Aᵀ: the plain product"


# ---- 8. specials ------------------------------------------------------------------------------------------------------

def _with_specials(x, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    x = x.copy()
    flat = x.reshape(-1)
    idx = g.choice(flat.size, min(flat.size, 60), replace=False)
    flat[idx] = np.resize(np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32), len(idx))
    return x


@pytest.mark.parametrize("path", ["fp32", "bf16", "amax", "amin"])
@pytest.mark.parametrize("name,N", [("rows", 3), ("rows", 64), ("hub_cols", 65)])
def test_specials(cmm, mm, dev, oracle_mod, path, name, N):
    P = pattern(name)
    dtype = torch.bfloat16 if path == "bf16" else torch.float32
    _, _, Bn, Gn = operands(P, N, seed=N + 3, dtype=dtype)
    Bn, Gn = _with_specials(Bn, 1), _with_specials(Gn, 2)
    B, G = torch.from_numpy(Bn).to(dtype), torch.from_numpy(Gn).to(dtype)
    if path in ("amax", "amin"):
        arg = torch_arg(P, Bn, path)
        want_v, want_b = select_expect(oracle_mod, P, Bn, Gn, arg)
        gv, gb = run_autograd(mm, dev, P, B, G, lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, path))
    else:
        split = True if dtype != torch.float32 else grad_b_splits(cmm, dev, P, N)
        want_v, want_b = sum_expect(oracle_mod, P.widened(dtype), Bn, Gn, split)
        gv, gb = run_autograd(mm, dev, P, B, G, ENTRIES["naiveSpMM"], dtype)
    assert_same_bits(gv, torch.from_numpy(want_v).to(dtype), f"{path} {name} N={N} specials grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b).to(dtype), f"{path} {name} N={N} specials grad_B")
    with np.errstate(invalid="ignore", over="ignore"):  # inf·0 and inf − inf make the reference NaN there: skipped
        if path in ("amax", "amin"):
            check_bound_select(P, Bn, Gn, arg, gv.numpy(), gb.numpy(), f"{path} {name} N={N} specials")
        else:
            check_bound_sum(P.widened(dtype), Bn, Gn, gv.float().numpy(), gb.float().numpy(),
                            f"{path} {name} N={N} specials", dtype)


# ---- 9. unsorted and duplicate columns -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shuffled_pattern():
    g = np.random.Generator(np.random.PCG64(31))
    M, K = 900, 700
    lens = g.integers(0, 90, M)
    lens[4] = 9000  # a row beyond the long-row threshold, with repeats
    rows = [g.integers(0, K - 50, int(n)) for n in lens]  # drawn with replacement: duplicates; unsorted
    rows[7] = np.full(30, 5)  # one column thirty times
    return Pattern("shuffled", M, K, rows, 32)


@pytest.mark.parametrize("N", [2, 64, 130])
@pytest.mark.parametrize("path", ["fp32", "bf16", "fp16", "mean"])
def test_unsorted_duplicate_columns_sum_paths(cmm, mm, dev, oracle_mod, path, N):
    P = shuffled_pattern()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(path, torch.float32)
    B, G, Bn, Gn = operands(P, N, seed=N + 19, dtype=dtype)
    Pw = P.widened(dtype)
    split = True if dtype != torch.float32 else grad_b_splits(cmm, dev, P, N)
    want_v, want_b = sum_expect(oracle_mod, Pw, Bn, mean_g(P, Gn) if path == "mean" else Gn, split)
    fn = (lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, "mean")) if path == "mean" else ENTRIES["naiveSpMM"]
    gv, gb = run_autograd(mm, dev, P, B, G, fn, dtype)
    assert_same_bits(gv, torch.from_numpy(want_v).to(dtype), f"{path} N={N} unsorted grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b).to(dtype), f"{path} N={N} unsorted grad_B")
    if path == "mean":
        cnt = P.row_counts.astype(np.float64)[:, None]
        check_bound_sum(P, Bn, np.where(cnt > 0, Gn / np.maximum(cnt, 1), Gn), gv.numpy(), gb.numpy(),
                        f"mean N={N} unsorted", extra_terms=1)
    else:
        check_bound_sum(Pw, Bn, Gn, gv.float().numpy(), gb.float().numpy(), f"{path} N={N} unsorted", dtype)


@pytest.mark.parametrize("N", [2, 5, 64, 300, 1100])
@pytest.mark.parametrize("reduce", ["amax", "amin"])
def test_unsorted_duplicate_columns_reduce_grad_entries(cmm, dev, oracle_mod, reduce, N):
    """custom_mm.spmm_reduce_grad_val / _grad_b on unsorted, repeated columns, with torch-CPU's arg and the oracle's Aᵀ."""
    P = shuffled_pattern()
    _, _, Bn, Gn = operands(P, N, seed=N + 23)
    arg = torch_arg(P, Bn, reduce)
    want_v, want_b = select_expect(oracle_mod, P, Bn, Gn, arg)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t_rp, t_row, _ = oracle_mod.csr_transpose(P.rowptr, P.col, P.val, P.M, P.K)
    perm = np.argsort(P.col, kind="stable").astype(np.int32)  # the stable transpose's entry order
    assert np.array_equal(np.repeat(np.arange(P.M), P.row_counts)[perm], t_row)
    arg_d = d(arg.astype(np.int32))
    gv = cmm.spmm_reduce_grad_val(d(P.col), d(P.rowptr), P.nnz, P.M, P.K, d(Bn), d(Gn), arg_d)
    gb = cmm.spmm_reduce_grad_b(d(t_rp), d(t_row), d(perm), d(P.val), P.nnz, P.M, P.K, d(Gn), arg_d)
    assert_same_bits(gv, torch.from_numpy(want_v), f"{reduce} N={N} unsorted grad_val")
    assert_same_bits(gb, torch.from_numpy(want_b), f"{reduce} N={N} unsorted grad_B")
    check_bound_select(P, Bn, Gn, arg, gv.cpu().numpy(), gb.cpu().numpy(), f"{reduce} N={N} unsorted")


# ---- 10. nnz = 0 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [3, 64])
@pytest.mark.parametrize("path", ["fp32", "bf16", "mean", "amax"])
def test_no_entries(mm, dev, path, N):
    P = Pattern("empty", 50, 40, [np.zeros(0, np.int64)] * 50, 0)
    dtype = torch.bfloat16 if path == "bf16" else torch.float32
    B, G, _, _ = operands(P, N, seed=1, dtype=dtype)
    fn = {"fp32": ENTRIES["naiveSpMM"], "bf16": ENTRIES["naiveSpMM"],
          "mean": lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, "mean"),
          "amax": lambda mm_, a, b: mm_.sparse_mm_reduce(a, b, "amax")}[path]
    gv, gb = run_autograd(mm, dev, P, B, G, fn, dtype)
    assert gv.numel() == 0
    assert_same_bits(gb, torch.zeros((P.K, N), dtype=dtype), f"{path} N={N}: grad B of an empty matrix is +0")


# ---- 11. the per-stream long-row workspace, shared by fp32 and low-precision products --------------------------------------

def test_workspace_interleaving_on_one_stream(cmm, mm, dev, oracle_mod, capi):
    """One stream, one per-stream long-row workspace shared by the fp32 and the low-precision products: each product's
    follow-up launch must leave its 16-byte header zero for the next one, and a workspace that has to grow (step 3) is
    re-allocated with a zero header.  The steps run on a high-priority stream, on which no other test runs a product, so
    the workspace sizes below are this test's own."""
    import ctypes
    hub_rows, hub_cols = pattern("hub_rows"), pattern("hub_cols")
    capi.mi_spmm_csr_workspace_bytes.restype = ctypes.c_size_t
    capi.mi_spmm_csr_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32]
    N3 = 2048
    need = [capi.mi_spmm_csr_workspace_bytes(P.nnz, n) for P, n in
            ((hub_rows, 64), (hub_cols, 64), (hub_rows, N3), (hub_cols, 64), (hub_rows, 64))]
    cap, grows = 0, []
    for b in need:  # the growth rule of the per-stream workspace (custom_mm_reference.inc, zeroed_stream_workspace)
        grows.append(b > cap)
        cap = b + b // 2 + 4096 if b > cap else cap
    assert grows == [True, False, True, False, False], (need, grows)  # step 3 re-allocates; steps 2, 4, 5 reuse

    alive = []  # every operand stays allocated: no later product meets an earlier one's addresses (no automatic schedule)

    def fp32_forward(N, seed, must_split):
        a = hub_rows.csr(dev, grad=False)  # a fresh tensor: no row schedule, the plain entry with the zero-kept workspace
        B, _, Bn, _ = operands(hub_rows, N, seed)
        B = B.to(dev)
        C = torch.empty((hub_rows.M, N), device=dev)
        split = bool(cmm.spmm_plan(hub_rows.nnz, hub_rows.M, hub_rows.K, B, C)[3])
        assert split or not must_split, "the hub-row product splits its long rows (the workspace header in use)"
        want = (oracle_mod.spmm_csr_long if split else oracle_mod.spmm_csr)(hub_rows.rowptr, hub_rows.col, hub_rows.val,
                                                                             hub_rows.M, hub_rows.K, Bn)
        got = mm.naiveSpMM.apply(a, B)
        alive.extend([a, B, C, got])
        return got, want

    def lowp_fwd_bwd(dtype, N, seed):
        B, G, Bn, Gn = operands(hub_cols, N, seed, dtype)
        Pw = hub_cols.widened(dtype)
        want_out = torch.from_numpy(oracle_mod.spmm_csr_long(Pw.rowptr, Pw.col, Pw.val, Pw.M, Pw.K, Bn)).to(dtype)
        want_v, want_b = sum_expect(oracle_mod, Pw, Bn, Gn, True)
        a = hub_cols.csr(dev, dtype)
        b = B.to(dev).requires_grad_()
        out = mm.naiveSpMM.apply(a, b)
        out.backward(G.to(dev))
        alive.extend([a, b, out])
        assert_same_bits(out, want_out, f"{dtype} forward")
        assert_same_bits(a.grad.values(), torch.from_numpy(want_v).to(dtype), f"{dtype} grad_val")
        assert_same_bits(b.grad, torch.from_numpy(want_b).to(dtype), f"{dtype} grad_B (hub columns: long Aᵀ rows)")
        check_bound_sum(Pw, Bn, Gn, a.grad.values().float().cpu().numpy(), b.grad.float().cpu().numpy(), f"{dtype}", dtype)

    stream = torch.cuda.Stream(device=dev, priority=-1)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got, want = fp32_forward(64, 1, True)        # 1. fp32 forward with a hub row: the workspace is allocated
        assert_same_bits(got, torch.from_numpy(want), "1. fp32 hub-row forward")
        lowp_fwd_bwd(torch.bfloat16, 64, 2)          # 2. bf16 forward + backward, hub columns: the same workspace
        got, want = fp32_forward(N3, 3, False)       # 3. fp32 at N = 2048: needs more than steps 1-2 left, re-allocated
        assert_same_bits(got, torch.from_numpy(want), f"3. fp32 forward at N = {N3}")
        lowp_fwd_bwd(torch.float16, 64, 4)           # 4. fp16 forward + backward on the grown workspace
        got, want = fp32_forward(64, 1, True)        # 5. fp32 AUTO_ZEROED forward again
        assert_same_bits(got, torch.from_numpy(want), "5. fp32 hub-row forward after the low-precision products")
    stream.synchronize()
