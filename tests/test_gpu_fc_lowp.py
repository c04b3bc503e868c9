"""bfloat16 / float16 FC layers on the MI355X: the bias epilogue, the deterministic split-k, the column
sums in T, the two modules and their autograd.

Contract (include/mi_spmm.h): every sum fp32, every output element rounded once at the store.
  1. bias epilogue, exact: integer operands and bias keep every fp32 sum an exact integer below 2²⁴;
  2. bias epilogue = the plain accumulator + one fp32 add;          3. split-k exact and rounded once (partials stay fp32);
  4. split-k invariances;      5. column sums = rne_T(float32 column sums of the widened values), bit for bit;
  6. the modules;              7. refusals leave C untouched;       8. graph capture.
Accuracy bound (test_gpu_gemm_lowp.py's, with the extra fp32 roundings counted): |C − E| ≤ u_T·|E| + r·2⁻²³·(|A|·|B| + |bias|)
(+ 2⁻²⁵ for fp16) against the float64 value E of the same T-rounded operands, r = k + 1 for the bias epilogue and k + S for
a split into S ranges.
"""
import sys

import pytest
import torch

from gpu_helpers import assert_same_bits
from test_gpu_gemm_lowp import ABS, LOWP, TRIPLES, U, exact, ints, nan_c, op, randn

pytestmark = pytest.mark.gpu


def int_bias(n, dev, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(-64, 65, (n,), device=dev, generator=g).to(dtype)


def shapes_of(m, n, k, ta, tb):
    return ((k, m) if ta else (m, k)), ((n, k) if tb else (k, n))


def bias_product(cmm, a, b, bias, ta, tb, dtype):
    m, n = (a.shape[1] if ta else a.shape[0]), (b.shape[0] if tb else b.shape[1])
    C = nan_c((m, n), a.device, dtype)
    out = cmm.cublas_mmul_bias(a, b, bias, C, ta, tb)
    assert out.data_ptr() == C.data_ptr()
    return C


def plain_product(cmm, a, b, ta, tb, dtype):
    m, n = (a.shape[1] if ta else a.shape[0]), (b.shape[0] if tb else b.shape[1])
    C = nan_c((m, n), a.device, dtype)
    cmm.cublas_mmul(a, b, C, ta, tb)
    return C


def split_product(cmm, a, b, ta, tb, dtype, bias=None, splits=0):
    m, n = (a.shape[1] if ta else a.shape[0]), (b.shape[0] if tb else b.shape[1])
    C = nan_c((m, n), a.device, dtype)
    cmm.cublas_mmul_splitk(a, b, C, ta, tb, bias, splits)
    return C


def unaligned(x):
    '''The same values behind a 2-byte-offset, odd-leading-dimension view.'''
    wide = torch.empty((x.shape[0], x.shape[1] + 3), device=x.device, dtype=x.dtype)
    wide[:, 1:x.shape[1] + 1] = x
    return wide[:, 1:x.shape[1] + 1]


def unaligned_vec(v):
    wide = torch.empty(v.numel() + 1, device=v.device, dtype=v.dtype)
    wide[1:] = v
    return wide[1:]


def assert_within(got, E, S_abs, rounds, dtype, what):
    tol = U[dtype] * E.abs() + rounds * 2.0 ** -23 * S_abs + ABS[dtype]
    err = (got.double() - E).abs()
    bad = ~(err <= tol)
    print(f"{what}: worst error / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values outside the bound, worst excess {float((err - tol).max())}"


# ---- 1. bias epilogue, exact ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_bias_epilogue_exact_every_transpose(cmm, dev, dtype):
    for i, (m, n, k) in enumerate(TRIPLES):
        for ta in (False, True):
            for tb in (False, True):
                sa, sb = shapes_of(m, n, k, ta, tb)
                a, b, bias = ints(sa, dev, dtype, 300 + i), ints(sb, dev, dtype, 400 + i), int_bias(n, dev, dtype, 500 + i)
                want = (op(a.double(), ta) @ op(b.double(), tb) + bias.double()).to(dtype)
                what = f"{dtype} m{m} n{n} k{k} ta{ta} tb{tb}"
                assert_same_bits(bias_product(cmm, a, b, bias, ta, tb, dtype), want, what)
                if i % 4 == 0:  # the checked form: unaligned operands and an unaligned bias
                    got = bias_product(cmm, unaligned(a), unaligned(b), unaligned_vec(bias), ta, tb, dtype)
                    assert_same_bits(got, want, what + " unaligned")


@pytest.mark.parametrize("dtype", LOWP)
def test_bias_epilogue_exact_vector_form_and_k0(cmm, dev, dtype):
    for m, n, k, ta, tb in ((512, 768, 1024, False, True), (1000, 264, 96, False, False), (2048, 4096, 64, True, False)):
        sa, sb = shapes_of(m, n, k, ta, tb)
        a, b, bias = ints(sa, dev, dtype, 1), ints(sb, dev, dtype, 2), int_bias(n, dev, dtype, 3)
        want = (op(a.double(), ta) @ op(b.double(), tb) + bias.double()).to(dtype)
        assert_same_bits(bias_product(cmm, a, b, bias, ta, tb, dtype), want, f"{dtype} {m}x{n}x{k}")
        assert_same_bits(bias_product(cmm, a, b, unaligned_vec(bias), ta, tb, dtype), want, f"{dtype} {m}x{n}x{k}, bias offset")
    # k == 0: the bias in every row
    bias = int_bias(40, dev, dtype, 4)
    got = bias_product(cmm, torch.empty((7, 0), device=dev, dtype=dtype), torch.empty((0, 40), device=dev, dtype=dtype), bias,
                       False, False, dtype)
    assert_same_bits(got, bias.expand(7, 40).contiguous(), f"{dtype} k = 0")


# ---- 2. bias epilogue = plain accumulator + one add ------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_bias_epilogue_is_the_plain_accumulator_plus_one_add(cmm, dev, dtype):
    for m, n, k, ta, tb in ((1031, 777, 1000, False, False), (4096, 768, 3072, False, True), (300, 200, 130, True, True)):
        sa, sb = shapes_of(m, n, k, ta, tb)
        a, b = randn(sa, dev, dtype, 11), randn(sb, dev, dtype, 12)
        plain = plain_product(cmm, a, b, ta, tb, dtype)
        zero = torch.zeros(n, device=dev, dtype=dtype)
        assert_same_bits(bias_product(cmm, a, b, zero, ta, tb, dtype), plain, f"{dtype} zero bias {m}x{n}x{k}")
        bias = randn((n,), dev, dtype, 13)
        E = op(a.double(), ta) @ op(b.double(), tb) + bias.double()
        S_abs = op(a.double().abs(), ta) @ op(b.double().abs(), tb) + bias.double().abs()
        assert_within(bias_product(cmm, a, b, bias, ta, tb, dtype), E, S_abs, k + 1, dtype, f"{dtype} random bias {m}x{n}x{k}")


# ---- 3. split-k, exact and rounded once ----------------------------------------------------------------------------

SPLIT_SHAPES = ((768, 3072, 16384, 8), (256, 256, 65536, 4), (256, 768, 4096, 8))


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("m,n,k,amp", SPLIT_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in SPLIT_SHAPES])
def test_split_k_exact_and_rounded_once(cmm, dev, dtype, m, n, k, amp):
    assert cmm.gemm_lowp_split_count(m, n, k) > 1
    amp = amp if dtype == torch.float16 else 8     # fp16 at k = 65536: [−4, 4] keeps the sums below 65504

    def draw(shape, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return torch.randint(-amp, amp + 1, shape, device=dev, generator=g).to(dtype)

    bias = int_bias(n, dev, dtype, 23)
    for ta in (False, True):
        for tb in (False, True):
            sa, sb = shapes_of(m, n, k, ta, tb)
            a, b = draw(sa, 21), draw(sb, 22)
            E = op(a.double(), ta) @ op(b.double(), tb)
            assert float(E.abs().max()) < 2.0 ** 24                              # every fp32 partial sum is exact
            if dtype == torch.float16:
                assert not bool(torch.isinf(E.to(dtype)).any())
            elif k >= 16384:
                assert float((E.abs() > 256).double().mean()) > 0.5              # bf16 partials narrowed early would show
            what = f"{dtype} {m}x{n}x{k} ta{ta} tb{tb}"
            assert_same_bits(split_product(cmm, a, b, ta, tb, dtype), E.to(dtype), what)
            assert_same_bits(split_product(cmm, a, b, ta, tb, dtype, bias), (E + bias.double()).to(dtype), what + " + bias")


# ---- 4. split-k invariances ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_split_k_invariances(cmm, dev, dtype):
    m, n, k = 768, 1536, 8192
    S = cmm.gemm_lowp_split_count(m, n, k)
    assert S > 1 and k % (32 * S) == 0
    a, b, bias = randn((k, m), dev, dtype, 31), randn((k, n), dev, dtype, 32), randn((n,), dev, dtype, 33)
    first = split_product(cmm, a, b, True, False, dtype, bias)
    assert_same_bits(split_product(cmm, a, b, True, False, dtype, bias), first, f"{dtype} second run")
    assert_same_bits(split_product(cmm, a, b, True, False, dtype, bias, S), first, f"{dtype} the rule's S given explicitly")
    E = a.double().t() @ b.double() + bias.double()
    S_abs = a.double().abs().t() @ b.double().abs() + bias.double().abs()
    assert_within(first, E, S_abs, k + S, dtype, f"{dtype} split {m}x{n}x{k} S{S}")
    for s in (2, 32):
        got = split_product(cmm, a, b, True, False, dtype, None, s)
        assert_within(got, E - bias.double(), S_abs, k + s, dtype, f"{dtype} S = {s}")
    # an unaligned view gives the bits of its aligned copy (checked loads, scalar combine)
    m2, n2, k2 = 200, 331, 4096
    a2, b2, bias2 = randn((m2, k2), dev, dtype, 34), randn((k2, n2), dev, dtype, 35), randn((n2,), dev, dtype, 36)
    assert cmm.gemm_lowp_split_count(m2, n2, k2) > 1
    want = split_product(cmm, a2, b2, False, False, dtype, bias2)
    assert_same_bits(split_product(cmm, unaligned(a2), unaligned(b2), False, False, dtype, unaligned_vec(bias2)), want,
                     f"{dtype} unaligned views")
    # a shape the rule does not split: the plain entries' bits
    for m3, n3, k3 in ((300, 200, 1000), (4096, 4096, 4096)):
        assert cmm.gemm_lowp_split_count(m3, n3, k3) == 1
        a3, b3, bias3 = randn((m3, k3), dev, dtype, 37), randn((n3, k3), dev, dtype, 38), randn((n3,), dev, dtype, 39)
        assert_same_bits(split_product(cmm, a3, b3, False, True, dtype), plain_product(cmm, a3, b3, False, True, dtype),
                         f"{dtype} S == 1")
        assert_same_bits(split_product(cmm, a3, b3, False, True, dtype, bias3), bias_product(cmm, a3, b3, bias3, False, True, dtype),
                         f"{dtype} S == 1 + bias")


# ---- 5. column sums ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("rows,n", [(1, 1), (5, 7), (1024, 64), (1025, 65), (16384, 3072), (3, 1000), (100000, 24)])
def test_column_sums_round_the_float32_sums_once(cmm, dev, dtype, rows, n):
    x = randn((rows, n), dev, dtype, rows + n)
    got = cmm.column_sums(x)
    assert got.dtype == dtype and got.shape == (n,)
    assert_same_bits(got, cmm.column_sums(x.float()).to(dtype), f"{dtype} {rows}x{n}")
    for off in (1, 4):  # column-offset views: 2-byte and 8-byte offsets
        wide = randn((rows, 2 * n + 5), dev, dtype, rows + n + off)
        view = wide[:, off:off + n]
        assert_same_bits(cmm.column_sums(view), cmm.column_sums(view.float().contiguous()).to(dtype), f"{dtype} view +{off}")
    if rows >= 5 and n >= 7:
        x[3, 2], x[0, 5], x[4, 5], x[1, 6] = float("inf"), float("inf"), float("-inf"), float("nan")
        got = cmm.column_sums(x)
        assert_same_bits(got, cmm.column_sums(x.float()).to(dtype), f"{dtype} {rows}x{n} specials")
        assert bool(torch.isinf(got[2])) and bool(torch.isnan(got[5])) and bool(torch.isnan(got[6]))


# ---- 6. the modules ------------------------------------------------------------------------------------------------

def _layer_refs(x, w, b, dy):
    '''float64 values of y, grad_inp, grad_w, grad_b from the T-rounded tensors, each with Σ|terms| and its k.'''
    x2, g2 = x.double().reshape(-1, x.shape[-1]), dy.double().reshape(-1, dy.shape[-1])
    w64 = w.double()
    y = x2 @ w64.t() + (b.double() if b is not None else 0)
    ya = x2.abs() @ w64.abs().t() + (b.double().abs() if b is not None else 0)
    return {"y": (y.view(dy.shape), ya.view(dy.shape), x.shape[-1]),
            "grad_inp": ((g2 @ w64).view(x.shape), (g2.abs() @ w64.abs()).view(x.shape), w.shape[0]),
            "grad_w": (g2.t() @ x2, g2.abs().t() @ x2.abs(), x2.shape[0]),
            "grad_b": (g2.sum(0), g2.abs().sum(0), x2.shape[0])}


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("lead", [(4, 32), (8, 512)], ids=["128tokens", "4096tokens"])
def test_modules_in_low_precision(mm, cmm, dev, dtype, lead):
    sys.modules.pop("fc_layers", None)
    import fc_layers
    g = torch.Generator().manual_seed(41)
    fin, fout = 768, 256
    tokens = lead[0] * lead[1]
    for bias in (True, False):
        x = torch.relu(torch.rand(*lead, fin, generator=g) - 0.5).to(dev).to(dtype)   # half the activations are exact zeros
        dy = (torch.rand(*lead, fout, generator=g) - 0.5).to(dev).to(dtype)
        results = {}
        for cls in (fc_layers.cublasLinear, fc_layers.cusparseLinear):
            layer = cls(fin, fout, bias=bias).to(dev).to(dtype)
            xi = x.clone().requires_grad_(True)
            y = layer(xi)
            y.backward(dy)
            got = {"y": y.detach(), "grad_inp": xi.grad, "grad_w": layer.weight.grad}
            if bias:
                got["grad_b"] = layer.bias.grad
            results[cls.__name__] = got
            refs = _layer_refs(x, layer.weight.detach(), layer.bias.detach() if bias else None, dy)
            S = cmm.gemm_lowp_split_count(fout, fin, tokens)
            assert (S > 1) == (tokens >= 2048)
            for name, t in got.items():
                E, A, k = refs[name]
                assert t.dtype == dtype and t.shape == E.shape, (cls.__name__, name)
                assert_within(t, E, A, k + (S if name == "grad_w" else 1), dtype, f"{cls.__name__} {dtype} bias={bias} {name}")
        for name, t in results["cublasLinear"].items():
            assert_same_bits(results["cusparseLinear"][name], t, f"cusparseLinear == cublasLinear: {name}")
        # a float32 layer beside it is untouched: the bits of the entry it has always called
        layer32 = fc_layers.cublasLinear(fin, fout, bias=bias).to(dev)
        x32 = x.float()
        want = torch.empty((tokens, fout), device=dev)
        if bias:
            cmm.cublas_mmul_bias(x32.reshape(-1, fin), layer32.weight.detach(), layer32.bias.detach(), want, False, True)
        else:
            cmm.cublas_mmul(x32.reshape(-1, fin), layer32.weight.detach(), want, False, True)
        y32 = layer32(x32)
        assert y32.dtype == torch.float32
        assert_same_bits(y32.detach().reshape(tokens, fout), want, "float32 layer")


def test_layers_refuse_mixed_dtypes_on_the_device(mm, dev):
    sys.modules.pop("fc_layers", None)
    import fc_layers
    for cls in (fc_layers.cublasLinear, fc_layers.cusparseLinear):
        with pytest.raises(RuntimeError, match=r"(?s)(?=.*bfloat16)(?=.*float32)"):
            cls(64, 32).to(dev).to(torch.bfloat16)(torch.rand(4, 64, device=dev))
        with pytest.raises(RuntimeError, match=r"(?s)(?=.*bfloat16)(?=.*float32)"):
            cls(64, 32).to(dev)(torch.rand(4, 64, device=dev).bfloat16())


# ---- 7. refusals on the device -------------------------------------------------------------------------------------

SENTINEL = -7.0


@pytest.mark.parametrize("dtype", LOWP)
def test_refusals_leave_c_untouched(cmm, dev, dtype):
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    a, b, bias = randn((8, 16), dev, dtype, 1), randn((16, 24), dev, dtype, 2), randn((24,), dev, dtype, 3)

    def c_of(dt, *lead):
        return torch.full(lead + (8, 24), SENTINEL, device=dev, dtype=dt)

    cases = [
        (lambda C: cmm.cublas_mmul_bias(a, b, bias.float(), C, False, False), dtype, r"(?s)(?=.*Float\b)(?=.*(BFloat16|Half))"),
        (lambda C: cmm.cublas_mmul_bias(a.float(), b.float(), bias, C, False, False), torch.float32, "bias must be float32"),
        (lambda C: cmm.cublas_mmul_bias(a, b.to(other), bias, C, False, False), dtype, r"(?s)(?=.*BFloat16)(?=.*Half)"),
        (lambda C: cmm.cublas_mmul_bias(a, b, bias.to(other), C, False, False), dtype, r"(?s)(?=.*BFloat16)(?=.*Half)"),
        (lambda C: cmm.cublas_mmul_bias(a.double(), b.double(), bias.double(), C, False, False), torch.float64, "float32"),
        (lambda C: cmm.cublas_mmul_bias(a, b, bias[:-1], C, False, False), dtype, "bias must have"),
        (lambda C: cmm.cublas_mmul_splitk(a.float(), b.float(), C, False, False), torch.float32, "cublas_mmul"),
        (lambda C: cmm.cublas_mmul_splitk(a, b.to(other), C, False, False), dtype, r"(?s)(?=.*BFloat16)(?=.*Half)"),
        (lambda C: cmm.cublas_mmul_splitk(a, b, C, False, False, bias.float()), dtype, r"(?s)(?=.*Float\b)(?=.*(BFloat16|Half))"),
        (lambda C: cmm.cublas_mmul_splitk(a, b, C, False, False, None, 3), dtype, "invalid|argument"),   # 16 % (32·3) != 0
    ]
    for i, (call, c_dtype, pattern) in enumerate(cases):
        C = c_of(c_dtype)
        with pytest.raises((RuntimeError, ValueError), match=pattern):
            call(C)
        torch.cuda.synchronize()
        assert bool((C == SENTINEL).all()), i
    C = c_of(dtype, 2)
    with pytest.raises(RuntimeError, match="2-d"):
        cmm.cublas_mmul_splitk(a[None].expand(2, -1, -1), b[None].expand(2, -1, -1), C, False, False)
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all())
    with pytest.raises(RuntimeError, match="float32"):
        cmm.column_sums(a.double())


# ---- 8. graph capture ----------------------------------------------------------------------------------------------

def test_graph_capture_replays_the_eager_bits(mm, dev):
    sys.modules.pop("fc_layers", None)
    import fc_layers
    dtype = torch.bfloat16
    layer = fc_layers.cublasLinear(768, 256).to(dev).to(dtype)
    x = randn((8, 512, 768), dev, dtype, 61).requires_grad_(True)
    dy = randn((8, 512, 256), dev, dtype, 62)
    params = (x, layer.weight, layer.bias)

    def step():
        y = layer(x)
        return (y,) + torch.autograd.grad(y, params, dy)

    eager = [t.detach().clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.detach().fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for name, got, want in zip(("y", "grad_inp", "grad_w", "grad_b"), outs, eager):
        assert_same_bits(got, want, f"graph replay: {name}")
