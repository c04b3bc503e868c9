"""bfloat16 / float16 dense products and their autograd, on the MI355X.

The contract (include/mi_spmm.h, mi_gemm_bf16 / _f16): fp32 sums, one rounding per element at the store, and one order
for the whole family — the bits of C[i, j] depend on row i of op(A), column j of op(B), k and the dtype only.
  1. exact: integer operands in [−8, 8] keep every fp32 partial sum exact, so the product is (A·B in float64).to(T)
     whatever the order inside the MFMA — bit for bit, in every transpose, batch and broadcast form, and with 65 538 items
     (the second pass of the item loops behind the 65 535-item grid cap, the k = 0 fill included);
  2. invariance: sub-products, batch position, storage transposes, unaligned views and repeated runs give the same bits;
  3. accuracy: |C − E| ≤ u_T·|E| + k·2⁻²³·(|A|·|B|) (+ 2⁻²⁵ for fp16) against the float64 product E;
  4. non-finite values; 5. autograd through the four dense classes; 6. graph capture.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ABS = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
SIZES = [1, 7, 16, 33, 64, 127, 128, 197, 255, 256, 513]


def _triples():
    '''About 40 (m, n, k): every size of SIZES in every position, the other two drawn with a fixed seed.'''
    g = np.random.Generator(np.random.PCG64(7))
    out = []
    for pos in range(3):
        for v in SIZES:
            t = [int(x) for x in g.choice(SIZES, 3)]
            t[pos] = v
            out.append(tuple(t))
    out += [tuple(int(x) for x in g.choice(SIZES, 3)) for _ in range(7)]
    return out


TRIPLES = _triples()


def ints(shape, dev, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(-8, 9, shape, device=dev, generator=g).to(dtype)


def randn(shape, dev, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, device=dev, generator=g).to(dtype)


def nan_c(shape, dev, dtype):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def op(x, t):
    return x.transpose(-1, -2) if t else x


def exact(a, b, ta, tb, dtype):
    '''(op(A)·op(B)) in float64, narrowed to T: exact for integer operands (every partial sum is an integer < 2^24).'''
    return (op(a.double(), ta) @ op(b.double(), tb)).to(dtype)


def product(cmm, a, b, ta, tb, dtype):
    '''cublas_mmul with A / B stored transposed for ta / tb, C pre-filled with NaN (an element never written shows).'''
    m, n = (a.shape[1] if ta else a.shape[0]), (b.shape[0] if tb else b.shape[1])
    C = nan_c((m, n), a.device, dtype)
    cmm.cublas_mmul(a, b, C, ta, tb)
    return C


# ---- 1. exact, bit for bit -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_exact_integer_products_every_transpose(cmm, dev, dtype):
    for i, (m, n, k) in enumerate(TRIPLES):
        for ta in (False, True):
            for tb in (False, True):
                a = ints((k, m) if ta else (m, k), dev, dtype, 100 + i)
                b = ints((n, k) if tb else (k, n), dev, dtype, 200 + i)
                got = product(cmm, a, b, ta, tb, dtype)
                assert_same_bits(got, exact(a, b, ta, tb, dtype), f"{dtype} m{m} n{n} k{k} ta{ta} tb{tb}")


@pytest.mark.parametrize("dtype", LOWP)
def test_exact_long_k(cmm, dev, dtype):
    m, n, k = 1000, 1000, 4099
    for ta, tb in ((False, False), (True, True)):
        a = ints((k, m) if ta else (m, k), dev, dtype, 1)
        b = ints((n, k) if tb else (k, n), dev, dtype, 2)
        assert_same_bits(product(cmm, a, b, ta, tb, dtype), exact(a, b, ta, tb, dtype), f"{dtype} long k ta{ta}")


@pytest.mark.parametrize("dtype", LOWP)
def test_exact_batched_and_broadcast(cmm, dev, dtype):
    for bsz, m, n, k in ((5, 33, 197, 64), (3, 128, 64, 513), (7, 255, 16, 7)):
        a = ints((bsz, m, k), dev, dtype, 3)
        b = ints((bsz, k, n), dev, dtype, 4)
        want = exact(a, b, False, False, dtype)
        C = nan_c((bsz, m, n), dev, dtype)
        cmm.cublas_bmm(a, b, C, 3, False, False)
        assert_same_bits(C, want, f"{dtype} batched {bsz}x{m}x{n}x{k}")
        # broadcast B (item stride 0) and stored-transposed operands
        bb = b[:1].expand(bsz, k, n)
        C = nan_c((bsz, m, n), dev, dtype)
        cmm.cublas_bmm(a.transpose(1, 2).contiguous(), bb, C, 3, True, False)
        assert_same_bits(C, exact(a, bb, False, False, dtype), f"{dtype} broadcast B, A stored transposed")
        # 4-d: [2, bsz] items, A broadcast over the first dim
        a4 = a[None].expand(2, bsz, m, k)
        b4 = ints((2, bsz, n, k), dev, dtype, 5)
        C = nan_c((2, bsz, m, n), dev, dtype)
        cmm.cublas_bmm(a4, b4, C, 4, False, True)
        assert_same_bits(C, exact(a4, b4, False, True, dtype), f"{dtype} 4-d")


@pytest.mark.parametrize("dtype", LOWP)
def test_exact_beyond_65535_items(cmm, dev, dtype):
    '''65 538 items of 8 × 32 · 32 × 8: the grid holds 65 535 of them, the rest come in the second pass of the item loop of
    gemm_lowp_kernel — plain and with A stored transposed — and, with k = 0, of fill_b16_kernel.'''
    bsz, m, n, k = 65538, 8, 8, 32
    a, b = ints((bsz, m, k), dev, dtype, 6), ints((bsz, k, n), dev, dtype, 7)
    want = exact(a, b, False, False, dtype)
    for a_op, ta, what in ((a, False, "plain"), (a.transpose(1, 2).contiguous(), True, "A stored transposed")):
        C = nan_c((bsz, m, n), dev, dtype)
        cmm.cublas_bmm(a_op, b, C, 3, ta, False)
        assert_same_bits(C, want, f"{dtype} {bsz} items, {what}")
    C = nan_c((bsz, m, n), dev, dtype)
    cmm.cublas_bmm(a[:, :, :0], b[:, :0], C, 3, False, False)
    assert_same_bits(C, torch.zeros_like(C), f"{dtype} {bsz} items, k = 0")


def test_exact_rounding_edges(cmm, dev):
    '''bf16 rounds integers above 256 to nearest even; fp16 sums ≥ 65520 become +inf, 65504 … 65519 become 65504.'''
    k = 1024
    for dtype in LOWP:
        a = torch.full((4, k), 8.0, device=dev)
        a[:, -1] = 1.0
        a[2:] *= -1
        b = torch.full((k, 8), 8.0, device=dev)
        extra = torch.tensor([38.0, 47.0, 48.0, 56.0, 1.0, 3.0, 5.0, 7.0], device=dev)  # 65472 + extra
        b[-1] = extra
        a, b = a.to(dtype), b.to(dtype)
        got = product(cmm, a, b, False, False, dtype)
        want = exact(a, b, False, False, dtype)
        assert_same_bits(got, want, f"{dtype} rounding edges")
        if dtype == torch.float16:
            row = got[0].float().cpu()
            assert row[0] == 65504 and row[1] == 65504 and torch.isinf(row[2]) and row[2] > 0
            assert torch.isinf(got[2, 2].float()) and got[2, 2].float() < 0


# ---- 2. invariance -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_bits_depend_on_row_column_and_k_only(cmm, dev, dtype):
    m, n, k = 1031, 777, 1000
    a, b = randn((m, k), dev, dtype, 11), randn((k, n), dev, dtype, 12)
    big = product(cmm, a, b, False, False, dtype)
    # any sub-product of rows / columns (a 64-wide one takes the narrow tile shape; column views are unaligned)
    for r0, r1, c0, c1 in ((100, 357, 33, 290), (0, 1031, 700, 764), (5, 6, 1, 2), (512, 1031, 0, 777)):
        sub = product(cmm, a[r0:r1], b[:, c0:c1], False, False, dtype)
        assert_same_bits(sub, big[r0:r1, c0:c1], f"{dtype} sub-product {r0}:{r1}, {c0}:{c1}")
        sub = product(cmm, a[r0:r1].contiguous(), b[:, c0:c1].contiguous(), False, False, dtype)
        assert_same_bits(sub, big[r0:r1, c0:c1], f"{dtype} contiguous sub-product {r0}:{r1}, {c0}:{c1}")
    # the same matrices as item 0 and as item 37 of a batch
    items_a, items_b = randn((40, 300, k), dev, dtype, 13), randn((40, k, 200), dev, dtype, 14)
    items_a[0], items_a[37] = a[:300], a[:300]
    items_b[0], items_b[37] = b[:, :200], b[:, :200]
    C = nan_c((40, 300, 200), dev, dtype)
    cmm.cublas_bmm(items_a, items_b, C, 3, False, False)
    assert_same_bits(C[0], big[:300, :200], f"{dtype} item 0")
    assert_same_bits(C[37], big[:300, :200], f"{dtype} item 37")
    # a product large enough for the 128 × 128 tiles, and sub-products that take the 128 × 64 ones
    a2, b2 = randn((2048, 256), dev, dtype, 15), randn((256, 4096), dev, dtype, 16)
    big2 = product(cmm, a2, b2, False, False, dtype)
    for r0, r1, c0, c1 in ((0, 1000, 0, 64), (77, 1100, 1000, 1300), (2000, 2048, 4000, 4096)):
        assert_same_bits(product(cmm, a2[r0:r1], b2[:, c0:c1], False, False, dtype), big2[r0:r1, c0:c1],
                         f"{dtype} tile shapes {r0}:{r1}, {c0}:{c1}")
    # stored transposed and plain
    assert_same_bits(product(cmm, a.t().contiguous(), b, True, False, dtype), big, f"{dtype} A stored transposed")
    assert_same_bits(product(cmm, a, b.t().contiguous(), False, True, dtype), big, f"{dtype} B stored transposed")
    assert_same_bits(product(cmm, a.t().contiguous(), b.t().contiguous(), True, True, dtype), big, f"{dtype} both")
    # a 2-byte-offset column view and the contiguous copy
    wide = torch.empty((k, n + 1), device=dev, dtype=dtype)
    wide[:, 1:] = b
    assert_same_bits(product(cmm, a, wide[:, 1:], False, False, dtype), big, f"{dtype} 2-byte offset view")
    # two runs
    assert_same_bits(product(cmm, a, b, False, False, dtype), big, f"{dtype} second run")


# ---- 3. accuracy ---------------------------------------------------------------------------------------------------

def assert_within_bound(got, a, b, ta, tb, dtype, what):
    E = op(a.double(), ta) @ op(b.double(), tb)
    S = op(a.double().abs(), ta) @ op(b.double().abs(), tb)
    k = a.shape[-2] if ta else a.shape[-1]
    tol = U[dtype] * E.abs() + k * 2.0 ** -23 * S + ABS[dtype]
    err = (got.double() - E).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values outside the bound, worst excess {float((err - tol).max())}"


@pytest.mark.parametrize("dtype", LOWP)
def test_accuracy_attention_square_and_fc_shapes(cmm, dev, dtype):
    items, S, D = 24, 512, 64  # BERT-base attention per item (2 × 12 heads here; the benchmark runs 32 × 12)
    q, kk, v = (randn((items, S, D), dev, dtype, s) for s in (21, 22, 23))
    C = nan_c((items, S, S), dev, dtype)
    cmm.cublas_bmm(q, kk, C, 3, False, True)
    assert_within_bound(C, q, kk, False, True, dtype, f"{dtype} q·kᵀ")
    p = torch.softmax(randn((items, S, S), dev, torch.float32, 24), -1).to(dtype)
    C = nan_c((items, S, D), dev, dtype)
    cmm.cublas_bmm(p, v, C, 3, False, False)
    assert_within_bound(C, p, v, False, False, dtype, f"{dtype} probs·V")
    a, b = randn((4096, 4096), dev, dtype, 25), randn((4096, 4096), dev, dtype, 26)
    assert_within_bound(product(cmm, a, b, False, False, dtype), a, b, False, False, dtype, f"{dtype} 4096³")
    x, w = randn((16384, 3072), dev, dtype, 27), randn((768, 3072), dev, dtype, 28)
    assert_within_bound(product(cmm, x, w, False, True, dtype), x, w, False, True, dtype, f"{dtype} FC forward (NT)")
    g = randn((16384, 768), dev, dtype, 29)
    assert_within_bound(product(cmm, x, g, True, False, dtype), x, g, True, False, dtype, f"{dtype} FC weight gradient (TN)")


# ---- 4. non-finite values ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_nan_poisons_its_row_only(cmm, dev, dtype):
    m, n, k = 300, 200, 130
    a, b = randn((m, k), dev, dtype, 31), randn((k, n), dev, dtype, 32)
    clean = product(cmm, a, b, False, False, dtype)
    a[17, 129] = float("nan")
    a[200, 0] = float("nan")
    got = product(cmm, a, b, False, False, dtype)
    assert bool(torch.isnan(got[17].float()).all()) and bool(torch.isnan(got[200].float()).all())
    rest = [i for i in range(m) if i not in (17, 200)]
    assert_same_bits(got[rest], clean[rest], f"{dtype} rows without NaN")


@pytest.mark.parametrize("dtype", LOWP)
def test_infinities_agree_with_torch_by_position_and_sign(cmm, dev, dtype):
    m, n, k = 64, 96, 100
    a, b = randn((m, k), dev, dtype, 33), randn((k, n), dev, dtype, 34)
    a[3, 10] = float("inf")
    a[5, 20] = float("-inf")
    a[7, 30] = float("inf")
    a[7, 31] = float("-inf")      # inf − inf in every column of row 7
    b[10, 4] = 0.0                # 0·inf: NaN at (3, 4)
    b[20, :8] = -1.0
    got = product(cmm, a, b, False, False, dtype).float().cpu()
    want = torch.matmul(a, b).float().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want))
    assert bool(torch.isinf(got[3]).sum() == n - 1) and bool(torch.isnan(got[3, 4]))


# ---- 5. autograd ---------------------------------------------------------------------------------------------------

CLASSES = (("cublasMM", False, False), ("cublasTransaMM", True, False), ("cublasTransbMM", False, True),
           ("cublasTransabMM", True, True))


def _grad_refs(a, b, g, ta, tb):
    '''float64 gradients of C = op(a)·op(b) for dC = g (and of |·| for the bound), as torch autograd computes them.'''
    out = []
    for absval in (False, True):
        f = (lambda x: x.double().abs()) if absval else (lambda x: x.double())
        a64, b64 = f(a).requires_grad_(True), f(b).requires_grad_(True)
        c = torch.matmul(op(a64, ta), op(b64, tb))
        ga, gb = torch.autograd.grad(c, (a64, b64), f(g))
        out.append((ga, gb))
    return out


def _check_grad(got, E, S, k, dtype, what, items=1):
    '''Within the bound of test 3; a broadcast operand's gradient is torch's sum (in T) of `items` such products, each
    rounded once: u_T·Σ|terms| more for those roundings.'''
    assert got.dtype == dtype, what
    tol = U[dtype] * E.abs() + k * 2.0 ** -23 * S + ABS[dtype] + (2 * U[dtype] * S if items > 1 else 0)
    bad = ~((got.double() - E).abs() <= tol)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values outside the bound"


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("name,ta,tb", CLASSES, ids=[c[0] for c in CLASSES])
def test_autograd_in_low_precision(mm, dev, dtype, name, ta, tb):
    cls = getattr(mm, name)
    M, K, N = 96, 80, 112
    for lead_a, lead_b in (((), ()), ((3,), (3,)), ((2, 3), (2, 3)), ((2, 3), ()), ((3,), (1,))):
        a0 = randn(lead_a + ((K, M) if ta else (M, K)), dev, dtype, 41)
        b0 = randn(lead_b + ((N, K) if tb else (K, N)), dev, dtype, 42)
        outs = []
        for _ in range(2):
            a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            c = cls.apply(a, b)
            g = randn(c.shape, dev, dtype, 43)
            c.backward(g)
            outs.append((c.detach(), a.grad, b.grad))
        c, ga, gb = outs[0]
        what = f"{name} {dtype} {lead_a}×{lead_b}"
        assert c.dtype == ga.dtype == gb.dtype == dtype, what
        for x, y in zip(outs[0], outs[1]):
            assert_same_bits(x, y, f"{what}: two runs")
        E = torch.matmul(op(a0.double(), ta), op(b0.double(), tb))
        S = torch.matmul(op(a0.double().abs(), ta), op(b0.double().abs(), tb))
        _check_grad(c, E, S, K, dtype, f"{what} forward")
        (ga64, gb64), (sa64, sb64) = _grad_refs(a0, b0, g, ta, tb)
        # a broadcast operand's gradient is the sum of the items' gradients, each within the bound, rounded once more
        items_a = max(1, c[..., :1, :1].numel() // max(1, a0[..., :1, :1].numel()))
        items_b = max(1, c[..., :1, :1].numel() // max(1, b0[..., :1, :1].numel()))
        _check_grad(ga, ga64, sa64, N * items_a, dtype, f"{what} dA", items_a)
        _check_grad(gb, gb64, sb64, M * items_b, dtype, f"{what} dB", items_b)


def test_fused_pair_stays_float32_only(mm, cmm, dev, monkeypatch):
    calls = []
    real = cmm.cublas_bmm_pair

    def counting(*args):
        calls.append(args[0].dtype)
        return real(*args)

    monkeypatch.setattr(cmm, "cublas_bmm_pair", counting)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        q = randn((2, 3, 128, 64), dev, dtype, 51).requires_grad_(True)
        k = randn((2, 3, 128, 64), dev, dtype, 52).requires_grad_(True)
        s = mm.cublasTransbMM.apply(q, k)
        s.backward(torch.ones_like(s))
        assert q.grad.dtype == k.grad.dtype == dtype
    assert calls == [torch.float32]


# ---- 6. graph capture ----------------------------------------------------------------------------------------------

def test_graph_capture_replays_the_eager_bits(mm, dev):
    q = randn((4, 12, 512, 64), dev, torch.bfloat16, 61)
    k = randn((4, 12, 512, 64), dev, torch.bfloat16, 62)
    eager = mm.cublasTransbMM.apply(q, k)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mm.cublasTransbMM.apply(q, k)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mm.cublasTransbMM.apply(q, k)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(out, eager, "graph replay")
