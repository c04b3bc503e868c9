"""bfloat16 / float16 sparse_mm_reduce (sum / mean / amax / amin) and its autograd on the MI355X — DESIGN.md §3.11.

Contract: the fp32 result of the exactly widened operands, narrowed once.  Witnesses: torch-CPU's own kernel
(aten::_sparse_mm_reduce_impl) on the widened operands for amax / amin values and arg, the float32 device path on the widened
operands, the CPU oracle for the sums and the gradients.  NaN is compared by position, everything else by bits.

Shape → kernel (contiguous B: the 8-byte form where N % 4 == 0, else the 2-byte element form; an offset view B[:, 1:N+1] with
ldb = N + 3 is always the element form):

  amax / amin  N = 1, 3, 4 → 1 lane per row;  8 → 2;  16 → 4;  32 → 8;  37, 64 → 16;  100, 128 → 32;
               256, 512, 602, 1024 → one wave per row (wave-uniform col / val; 602 and 1024 in passes);
               a row beyond 8192 entries → hub kernel (S = 1); beyond 2·16384 → hub kernel with S = 2 + hub combine
  mean         N = 1, 3 → narrow;  256, 512, 1024 → wave-row;  4 … 128 → lane groups of 1 … 32;  602 → the 64-lane group;
               the hub rows → the long-row follow-up with the division at its final store
`test_every_kernel_form_is_reached` restates the launchers' rule and asserts that the shapes below reach every form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
WIDTHS = [1, 3, 4, 8, 16, 32, 37, 64, 100, 128, 256, 512, 602, 1024]
VIEW_WIDTHS = [1, 4, 8, 16, 32, 37, 64, 128, 256]  # B[:, 1:N+1] of a [K, N+3] tensor
HUB_WIDTHS = [3, 37, 64, 256]                      # (37 from an offset view too)
SELECT = ("amax", "amin")


# ---- helpers ------------------------------------------------------------------------------------------------------

def rne(x, dtype):
    """numpy float32 → torch tensor of `dtype` (torch's round-to-nearest-even narrowing)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype)


def up(t):
    """torch tensor of T → numpy float32 (exact)."""
    return t.detach().float().cpu().numpy()


def csr_rows(K, lens, seed, dtype, scale=1.0):
    """Unsorted columns with duplicates; values already representable in `dtype` (as float32)."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = g.integers(0, K, int(lens.sum())).astype(np.int32)
    val = up(rne((g.random(len(col), dtype=np.float32) - 0.5) * scale, dtype))
    return rowptr, col, val


def mixed_lengths(M, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    lens = g.integers(1, 201, M)
    lens[g.random(M) < 0.1] = 0  # empty rows
    lens[g.random(M) < 0.1] = 1  # one-entry rows
    lens[:3] = (0, 1, 200)
    return lens


def dense(g, shape, dtype):
    return up(rne(g.standard_normal(shape, dtype=np.float32), dtype))


def assert_same_bits(got, want, what=""):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn), f"{what}: NaN positions differ ({torch.nonzero(gn != wn)[:5].tolist()})"
    gb, wb = got.view(torch.int16)[~gn], want.view(torch.int16)[~wn]
    bad = torch.nonzero(gb != wb).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} values differ, first got {got[~gn][bad[:5]].tolist()} "
                              f"want {want[~wn][bad[:5]].tolist()}")


def torch_cpu_reduce(rowptr, col, val, M, K, B, reduce):
    """torch-CPU's kernel on float32 arrays: (out float32 numpy, arg int32 numpy)."""
    a = torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                torch.from_numpy(val), (M, K)).requires_grad_()
    out, arg = torch.ops.aten._sparse_mm_reduce_impl(a, torch.from_numpy(np.ascontiguousarray(B)), reduce)
    return out.detach().numpy(), arg.numpy().astype(np.int32)


def dev_csr(dev, rowptr, col, val, dtype):
    return torch.from_numpy(val).to(dtype).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(rowptr).to(dev)


def gpu_reduce(cmm, dev, csr, M, K, Bd, reduce, with_arg=False):
    vals, cols, offs = csr
    C = torch.full((M, Bd.shape[1]), 7.0, device=dev, dtype=Bd.dtype)
    arg = torch.full((M, Bd.shape[1]), -7, device=dev, dtype=torch.int32) if with_arg else None
    cmm.naive_spmm_reduce(vals, cols, offs, vals.numel(), M, K, Bd, C, reduce, arg)
    return C, arg


def check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, what, Bd=None):
    """amax / amin in T against torch-CPU on the widened operands (values narrowed, arg equal) and against the float32
    device path on the widened operands; with and without arg.  `val`, `B`: float32 arrays holding T values."""
    csr = dev_csr(dev, rowptr, col, val, dtype)
    Bd = torch.from_numpy(B).to(dtype).to(dev) if Bd is None else Bd
    csr32 = (csr[0].float(), csr[1], csr[2])
    for r in SELECT:
        want, want_arg = torch_cpu_reduce(rowptr, col, val, M, K, B, r)
        got, got_arg = gpu_reduce(cmm, dev, csr, M, K, Bd, r, with_arg=True)
        assert got.dtype == dtype
        assert_same_bits(got, rne(want, dtype), f"{what} {r} vs torch-CPU")
        bad = np.argwhere(got_arg.cpu().numpy() != want_arg)
        assert bad.size == 0, f"{what} {r}: arg differs from torch-CPU at {bad[:5].tolist()}"
        got32, arg32 = gpu_reduce(cmm, dev, csr32, M, K, Bd.float().contiguous(), r, with_arg=True)
        assert_same_bits(got, got32.cpu().to(dtype), f"{what} {r} vs the float32 path")
        assert torch.equal(got_arg, arg32), f"{what} {r}: arg differs from the float32 path"
        got_noarg, _ = gpu_reduce(cmm, dev, csr, M, K, Bd, r)
        assert_same_bits(got_noarg, got, f"{what} {r} without arg")


def mean_witnesses(cmm, dev, oracle_mod, rowptr, col, val, M, K, B, dtype):
    """(fp32 device product with long rows split, divided in float32 on the device; the oracle's split sum divided in numpy
    float32), both narrowed once, and the fp32 sum itself."""
    csr = dev_csr(dev, rowptr, col, val, torch.float32)
    C32 = torch.empty((M, B.shape[1]), device=dev)
    cmm.naive_spmm_ex(*csr, len(val), M, K, torch.from_numpy(B).to(dev), C32, 1)
    first = cmm.spmm_rows_divide(csr[2], M, C32, torch.empty_like(C32)).cpu().to(dtype)
    total = oracle_mod.spmm_csr_long(rowptr, col, val, M, K, B)
    cnt = np.diff(rowptr).astype(np.float32)[:, None]
    second = np.where(cnt > 0, total / np.maximum(cnt, np.float32(1)), total).astype(np.float32)
    return first, rne(second, dtype), total, cnt


def check_mean(cmm, dev, oracle_mod, rowptr, col, val, M, K, B, dtype, what, Bd=None):
    csr = dev_csr(dev, rowptr, col, val, dtype)
    Bd = torch.from_numpy(B).to(dtype).to(dev) if Bd is None else Bd
    got, _ = gpu_reduce(cmm, dev, csr, M, K, Bd, "mean")
    first, second, total, cnt = mean_witnesses(cmm, dev, oracle_mod, rowptr, col, val, M, K, B, dtype)
    assert_same_bits(got, first, f"{what} mean vs the float32 path divided")
    assert_same_bits(got, second, f"{what} mean vs the oracle divided")
    empty = torch.from_numpy(np.diff(rowptr) == 0)
    assert torch.all(got.cpu()[empty].view(torch.int16) == 0), f"{what}: empty rows give +0"
    plain = torch.empty_like(got)
    cmm.naive_spmm(*csr, len(val), M, K, Bd, plain)
    got_sum, _ = gpu_reduce(cmm, dev, csr, M, K, Bd, "sum")
    assert_same_bits(got_sum, plain, f"{what} sum vs naive_spmm")
    return got, total, cnt


# ---- 1 / 2. every width, both layouts ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", WIDTHS)
def test_amax_amin_values_and_arg_at_every_width(cmm, dev, dtype, N):
    M, K = 160, 700
    rowptr, col, val = csr_rows(K, mixed_lengths(M, N), seed=N, dtype=dtype)
    B = dense(np.random.Generator(np.random.PCG64(100 + N)), (K, N), dtype)
    check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} N={N}")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", VIEW_WIDTHS)
def test_column_offset_view_of_B(cmm, dev, oracle_mod, dtype, N):
    M, K = 120, 400
    rowptr, col, val = csr_rows(K, mixed_lengths(M, 7 + N), seed=7 + N, dtype=dtype)
    Bw = dense(np.random.Generator(np.random.PCG64(N)), (K, N + 3), dtype)
    Bd = torch.from_numpy(Bw).to(dtype).to(dev)[:, 1:N + 1]  # ldb = N + 3, first column 2 bytes in
    assert not Bd.is_contiguous()
    B = np.ascontiguousarray(Bw[:, 1:N + 1])
    check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} view N={N}", Bd=Bd)
    check_mean(cmm, dev, oracle_mod, rowptr, col, val, M, K, B, dtype, f"{dtype} view N={N}", Bd=Bd)


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", WIDTHS)
def test_mean_is_one_rounding_of_the_fp32_sum_divided(cmm, dev, oracle_mod, dtype, N):
    M, K = 160, 700
    rowptr, col, val = csr_rows(K, mixed_lengths(M, N), seed=N, dtype=dtype)
    B = dense(np.random.Generator(np.random.PCG64(100 + N)), (K, N), dtype)
    got, total, cnt = check_mean(cmm, dev, oracle_mod, rowptr, col, val, M, K, B, dtype, f"{dtype} N={N}")
    if N == 128:
        # narrowing the sum first and dividing after is a second rounding: other bits on this case (checked on the CPU)
        twice = np.where(cnt > 0, up(rne(total, dtype)) / np.maximum(cnt, np.float32(1)), total).astype(np.float32)
        differs = (rne(twice, dtype).view(torch.int16) != got.cpu().view(torch.int16)).sum().item()
        assert differs > 0, "the case no longer tells one rounding from two"


# ---- hub rows --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", HUB_WIDTHS)
def test_hub_rows(cmm, dev, oracle_mod, dtype, N):
    M, K = 300, 50_000
    lens = np.full(M, 50, np.int64)
    lens[3], lens[200], lens[7] = 9_000, 20_000, 40_000  # S = 1, S = 1, S = 2 (beyond 2 · 16384)
    lens[11] = 0
    rowptr, col, val = csr_rows(K, lens, seed=N, dtype=dtype)
    g = np.random.Generator(np.random.PCG64(N + 1))
    B = dense(g, (K, N), dtype)
    check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} hub rows N={N}")
    check_mean(cmm, dev, oracle_mod, rowptr, col, val, M, K, B, dtype, f"{dtype} hub rows N={N}")
    Bt = g.integers(-2, 3, (K, N)).astype(np.float32)  # ties across the chunks of a hub row
    Bt[g.random((K, N)) < 2e-5] = np.nan
    check_select(cmm, dev, rowptr, col, val, M, K, Bt, dtype, f"{dtype} hub rows with ties N={N}")
    if N == 37:
        Bw = dense(g, (K, N + 3), dtype)
        Bd = torch.from_numpy(Bw).to(dtype).to(dev)[:, 1:N + 1]
        Bv = np.ascontiguousarray(Bw[:, 1:N + 1])
        check_select(cmm, dev, rowptr, col, val, M, K, Bv, dtype, f"{dtype} hub rows, view", Bd=Bd)
        check_mean(cmm, dev, oracle_mod, rowptr, col, val, M, K, Bv, dtype, f"{dtype} hub rows, view", Bd=Bd)


# ---- 3. ties and specials -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_small_integer_ties_select_the_smallest_entry(cmm, dev, dtype):
    M, K = 200, 300
    g = np.random.Generator(np.random.PCG64(5))
    rowptr, col, _ = csr_rows(K, mixed_lengths(M, 5), seed=5, dtype=dtype)
    val = g.choice(np.array([1.0, -1.0, 2.0, 0.5], np.float32), len(col))
    for N in (1, 4, 37, 256):
        B = g.integers(-2, 3, (K, N)).astype(np.float32)
        check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} ties N={N}")
        want, want_arg = torch_cpu_reduce(rowptr, col, val, M, K, B, "amax")
        prod = val[:, None] * B[col]  # exact
        for i in range(0, M, 17):
            lo, hi = rowptr[i], rowptr[i + 1]
            if hi > lo:
                assert np.array_equal(want_arg[i], lo + np.argmax(prod[lo:hi], axis=0)), "the smallest e attaining the maximum"


@pytest.mark.parametrize("dtype", LOWP)
def test_products_that_tie_only_after_narrowing_take_arg_from_fp32(cmm, dev, dtype):
    M, K, N = 64, 50, 16
    eps = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    g = np.random.Generator(np.random.PCG64(21))
    lens = g.integers(2, 30, M)
    rowptr, col, _ = csr_rows(K, lens, seed=21, dtype=dtype)
    steps = np.array([1.0, 1.0 + eps, 1.0 + 2 * eps, 1.0 + 3 * eps], np.float32)  # all exact in T
    val = g.choice(steps, len(col))
    B = g.choice(steps, (K, N))
    assert np.array_equal(up(rne(val, dtype)), val) and np.array_equal(up(rne(B, dtype)), B)
    check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} ties after narrowing")
    # the case does what its name says: choosing among the NARROWED products would pick another entry somewhere
    _, want_arg = torch_cpu_reduce(rowptr, col, val, M, K, B, "amax")
    prod = val[:, None] * B[col]  # one fp32 multiply, exact here
    narrowed = up(rne(prod, dtype))
    assert np.any(narrowed != prod)
    other = np.stack([rowptr[i] + np.argmax(narrowed[rowptr[i]:rowptr[i + 1]], axis=0) for i in range(M)])
    assert np.any(other != want_arg), "no product ties only after narrowing"


@pytest.mark.parametrize("dtype", LOWP)
def test_signed_zeros_infinities_nan_subnormals_and_overflow(cmm, dev, dtype):
    M, K = 200, 300
    g = np.random.Generator(np.random.PCG64(9))
    rowptr, col, _ = csr_rows(K, mixed_lengths(M, 9), seed=9, dtype=dtype)
    tiny = 2.0 ** -130 if dtype == torch.bfloat16 else 2.0 ** -20  # subnormal in T
    assert up(rne(np.array([tiny]), dtype))[0] == np.float32(tiny)
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, np.inf, -np.inf, np.nan, tiny, -tiny, 3 * tiny], np.float32)
    val = g.choice(np.array([0.0, -0.0, 1.0, -1.0, 2.0, np.inf, np.nan, 0.5], np.float32), len(col),
                   p=[.15, .15, .2, .15, .15, .05, .02, .13])  # 0 × inf = NaN; NaN in val
    for N in (1, 5, 64, 256):
        B = g.choice(special, (K, N), p=[.12, .12, .12, .12, .08, .08, .06, .06, .03, .08, .08, .05]).astype(np.float32)
        check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} specials N={N}")
    # every product of a column is -inf (amax: out -inf, arg nnz) or +inf (amin)
    val = up(rne(g.random(len(col), dtype=np.float32) + 0.5, dtype))
    B = dense(np.random.Generator(np.random.PCG64(1)), (K, 8), dtype)
    B[:, 2] = -np.inf
    B[:, 5] = np.inf
    check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} all-inf columns")
    # large products: finite in fp32; in fp16 beyond 65504 they are stored as ±inf while arg stays the fp32 choice
    val = g.choice(np.array([300.0, -300.0, 280.0, 1.0], np.float32), len(col))
    B = g.choice(np.array([300.0, 301.0, 302.0, -301.0, 250.0, 2.0], np.float32), (K, 16))
    assert np.array_equal(up(rne(B, dtype)), B) or dtype == torch.bfloat16
    B, val = up(rne(B, dtype)), up(rne(val, dtype))
    check_select(cmm, dev, rowptr, col, val, M, K, B, dtype, f"{dtype} large products")
    if dtype == torch.float16:
        want, _ = torch_cpu_reduce(rowptr, col, val, M, K, B, "amax")
        assert np.any((want > 65504) & np.isfinite(want)) and torch.isinf(rne(want, dtype)).any()


# ---- 4. gradients -------------------------------------------------------------------------------------------------------

def csr_tensor(rowptr, col, val, M, K, dtype, device):
    return torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                   torch.from_numpy(val).to(dtype), (M, K), device=device).requires_grad_()


def run_backward(mm, dev, rowptr, col, val, M, K, B, G, dtype, reduce):
    a = csr_tensor(rowptr, col, val, M, K, dtype, dev)
    b = torch.from_numpy(B).to(dtype).to(dev).requires_grad_()
    out = mm.sparse_mm_reduce(a, b, reduce)
    assert out.dtype == dtype
    out.backward(torch.from_numpy(G).to(dtype).to(dev))
    assert a.grad.layout == torch.sparse_csr and a.grad.dtype == dtype and b.grad.dtype == dtype
    return out.detach(), a.grad.values().detach(), b.grad.detach()


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("reduce", SELECT)
@pytest.mark.parametrize("N", [3, 37, 64, 256, 1100])
def test_amax_amin_gradients_against_the_oracle(mm, dev, oracle_mod, dtype, reduce, N):
    M, K = 180, 260
    rowptr, col, val = csr_rows(K, mixed_lengths(M, N) % 120, seed=N, dtype=dtype)
    g = np.random.Generator(np.random.PCG64(N + 50))
    B = up(rne(g.integers(-3, 4, (K, N)).astype(np.float32) * 0.75, dtype))  # ties: the gradient goes to the selected entry
    G = dense(g, (M, N), dtype)
    want, want_arg = torch_cpu_reduce(rowptr, col, val, M, K, B, reduce)
    runs = [run_backward(mm, dev, rowptr, col, val, M, K, B, G, dtype, reduce) for _ in range(2)]
    out, gval, gb = runs[0]
    assert_same_bits(out, rne(want, dtype), f"{dtype} {reduce} N={N} forward")
    assert_same_bits(gval, rne(oracle_mod.reduce_grad_val(rowptr, col, M, B, G, want_arg), dtype), f"{dtype} {reduce} N={N} grad val")
    assert_same_bits(gb, rne(oracle_mod.reduce_grad_b(rowptr, col, val, M, K, G, want_arg), dtype), f"{dtype} {reduce} N={N} grad B")
    for x, y in zip(runs[0], runs[1]):
        assert_same_bits(x, y, f"{dtype} {reduce} N={N}: second run")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [3, 37, 64, 256])
def test_mean_and_sum_gradients(cmm, mm, dev, dtype, N):
    M, K = 180, 260
    rowptr, col, val = csr_rows(K, mixed_lengths(M, N) % 120, seed=N, dtype=dtype)
    g = np.random.Generator(np.random.PCG64(N + 60))
    B, G = dense(g, (K, N), dtype), dense(g, (M, N), dtype)
    # sum: naiveSpMM's forward and backward
    a = csr_tensor(rowptr, col, val, M, K, dtype, dev)
    b = torch.from_numpy(B).to(dtype).to(dev).requires_grad_()
    plain = mm.naiveSpMM.apply(a, b)
    plain.backward(torch.from_numpy(G).to(dtype).to(dev))
    runs = [run_backward(mm, dev, rowptr, col, val, M, K, B, G, dtype, "sum") for _ in range(2)]
    for got, want, what in zip(runs[0], (plain.detach(), a.grad.values(), b.grad), ("forward", "grad val", "grad B")):
        assert_same_bits(got, want, f"{dtype} sum N={N} {what}")
    # mean: the T sum backward applied to g' = rne_T(up(g) / count), which is materialised in T
    offs = torch.from_numpy(rowptr).to(dev)
    Gd = torch.from_numpy(G).to(dtype).to(dev)
    g_div = cmm.spmm_rows_divide(offs, M, Gd, torch.empty_like(Gd))
    cnt = np.diff(rowptr).astype(np.float32)[:, None]
    assert_same_bits(g_div, rne(np.where(cnt > 0, G / np.maximum(cnt, np.float32(1)), G), dtype), f"{dtype} g / count N={N}")
    a2 = csr_tensor(rowptr, col, val, M, K, dtype, dev)
    b2 = torch.from_numpy(B).to(dtype).to(dev).requires_grad_()
    mm.naiveSpMM.apply(a2, b2).backward(g_div)
    mruns = [run_backward(mm, dev, rowptr, col, val, M, K, B, G, dtype, "mean") for _ in range(2)]
    assert_same_bits(mruns[0][1], a2.grad.values(), f"{dtype} mean N={N} grad val")
    assert_same_bits(mruns[0][2], b2.grad, f"{dtype} mean N={N} grad B")
    for r in (runs, mruns):
        for x, y in zip(r[0], r[1]):
            assert_same_bits(x, y, f"{dtype} N={N}: second run")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("reduce", ["sum", "mean", "amax", "amin"])
def test_small_integer_operands_equal_float64_autograd(mm, dev, dtype, reduce):
    """Every product, sum and quotient below is exact in T (integers below 2⁸, row counts powers of two), so torch's float64
    autograd on the CPU, narrowed, is the expectation bit for bit."""
    M, K, N = 60, 40, 16
    g = np.random.Generator(np.random.PCG64(33))
    lens = g.choice(np.array([0, 1, 2, 4, 8]), M)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(g.choice(K, int(n), replace=False)) for n in lens]).astype(np.int32)
    val = g.choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), len(col))
    B = g.integers(-2, 3, (K, N)).astype(np.float32)
    G = g.integers(-2, 3, (M, N)).astype(np.float32)
    a64 = csr_tensor(rowptr, col, val, M, K, torch.float64, "cpu")
    b64 = torch.from_numpy(B).double().requires_grad_()
    out64 = torch.sparse.mm(a64, b64, reduce=reduce)
    out64.backward(torch.from_numpy(G).double())
    out, gval, gb = run_backward(mm, dev, rowptr, col, val, M, K, B, G, dtype, reduce)
    assert_same_bits(out, out64.detach().to(dtype), f"{dtype} {reduce} forward")
    assert_same_bits(gval, a64.grad.values().to(dtype), f"{dtype} {reduce} grad val")
    assert_same_bits(gb, b64.grad.to(dtype), f"{dtype} {reduce} grad B")


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("reduce", ["amax", "mean"])
def test_graph_captured_forward_replays_to_the_eager_bits(cmm, dev, dtype, reduce):
    M, K, N = 3000, 20_000, 64
    lens = np.full(M, 30, np.int64)
    lens[5] = 40_000  # a hub row: the follow-up launches are captured too
    rowptr, col, val = csr_rows(K, lens, seed=4, dtype=dtype)
    csr = dev_csr(dev, rowptr, col, val, dtype)
    B = torch.randn(K, N, device=dev).to(dtype)
    with_arg = reduce == "amax"
    C_eager, arg_eager = gpu_reduce(cmm, dev, csr, M, K, B, reduce, with_arg)
    C = torch.full((M, N), 7.0, device=dev, dtype=dtype)
    arg = torch.full((M, N), -7, device=dev, dtype=torch.int32) if with_arg else None
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cmm.naive_spmm_reduce(*csr, len(val), M, K, B, C, reduce, arg)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cmm.naive_spmm_reduce(*csr, len(val), M, K, B, C, reduce, arg)
    for _ in range(2):
        C.fill_(7.0)
        if with_arg:
            arg.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(C, C_eager, f"{dtype} {reduce} graph replay")
        if with_arg:
            assert torch.equal(arg, arg_eager)


# ---- 6. instantiation coverage --------------------------------------------------------------------------------------------

def pow2_ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def select_forms(N, vec, hub):
    """launch_reduce of csr_reduce_device.h with Forms<Lowp<T>> of csr_reduce_lowp.hip (the choice of VEC), restated: lanes per
    row = pow2_ceil(⌈N / 4⌉) up to 64; rows beyond 8192 entries go to the hub kernel, beyond 2 · 16384 also through the combine."""
    forms = {("rows", min(64, pow2_ceil((N + 3) // 4)), vec)}
    if hub:
        forms |= {("hub", vec), ("hub combine",)}
    return forms


def mean_forms(N, vec, hub):
    """spmm_lowp of csr_lowp.hip, restated."""
    if N < 4:
        return {("narrow",)}
    forms = set()
    if vec and N in (256, 512, 1024):
        forms.add(("wave-row", N // 256))
    else:
        nq = (N + 3) // 4
        G = min(64, pow2_ceil(nq))
        forms.add(("group", G, 1 if G < 64 else min(4, pow2_ceil((nq + 63) // 64)), vec))
    if hub:
        forms.add(("long rows", vec))
    return forms


def test_every_kernel_form_is_reached():
    select, mean = set(), set()
    for N in WIDTHS:
        select |= select_forms(N, N % 4 == 0, False)
        mean |= mean_forms(N, N % 4 == 0, False)
    for N in VIEW_WIDTHS:
        select |= select_forms(N, False, False)
        mean |= mean_forms(N, False, False)
    for N in HUB_WIDTHS:
        select |= select_forms(N, N % 4 == 0, True)
        mean |= mean_forms(N, N % 4 == 0, True)
    select |= select_forms(37, False, True)
    mean |= mean_forms(37, False, True)
    want_select = {("rows", G, vec) for G in (1, 2, 4, 8, 16, 32, 64) for vec in (True, False)}
    want_select |= {("hub", True), ("hub", False), ("hub combine",)}
    assert want_select <= select, sorted(want_select - select, key=str)
    want_mean = {("narrow",), ("wave-row", 1), ("wave-row", 2), ("wave-row", 4), ("long rows", True), ("long rows", False)}
    want_mean |= {("group", G, 1, True) for G in (1, 2, 4, 8, 16, 32)}
    want_mean |= {("group", G, 1, False) for G in (1, 2, 4, 8, 16, 32, 64)} | {("group", 64, 4, False)}
    assert want_mean <= mean, sorted(want_mean - mean, key=str)
