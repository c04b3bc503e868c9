"""matmuls.sampled_matmul and matmuls.sparse_attention on the MI355X: the sampled product's values are the SDDMM kernels'
bit for bit, its gradients and the whole attention step are held to the e_dev ≤ 8 · e_ref rule against float64 torch-CPU
autograd of the dense masked expression (e_ref: the same expression in torch-CPU float32), and the bfloat16 / float16 step
is the float32 stages on widened inputs, narrowed once per stage."""
import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits
from sparse_attention_helpers import assert_under_rule, dense_mask, device_pattern, scaled_err, with_values

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)


def csr_from_rows(rows_cols, M, K, dev, index_dtype=torch.int64):
    """A CSR tensor (values 1) from a list of per-row column arrays, kept in the order given (unsorted allowed)."""
    lens = [len(c) for c in rows_cols]
    crow = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=index_dtype)
    col = torch.tensor(np.concatenate(rows_cols) if sum(lens) else np.zeros(0), dtype=index_dtype)
    return torch.sparse_csr_tensor(crow.to(dev), col.to(dev), torch.ones(len(col), device=dev), size=(M, K))


def random_pattern(M, K, lens, seed, dev, shuffle=False):
    g = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for n in lens:
        c = np.sort(g.choice(K, int(n), replace=False))
        rows.append(g.permutation(c) if shuffle else c)
    return csr_from_rows(rows, M, K, dev)


def entry_rows(a):
    crow = a.crow_indices().cpu()
    return torch.repeat_interleave(torch.arange(a.shape[-2]), crow[1:] - crow[:-1])


def cpu_sampled(a, m1, m2t, w, dtype):
    """torch-CPU autograd of the dense masked product (m1 · m2tᵀ) ⊙ mask in `dtype`: (values at the stored positions in
    CSR order, grad m1, grad m2t) for the incoming values-gradient w."""
    r, c = entry_rows(a), a.col_indices().cpu()
    x1, x2 = m1.cpu().to(dtype).requires_grad_(True), m2t.cpu().to(dtype).requires_grad_(True)
    mask = dense_mask(a).to(dtype)
    dense = (x1 @ x2.T) * mask
    wd = torch.zeros_like(mask)
    wd[r, c] = w.cpu().to(dtype)
    g1, g2 = torch.autograd.grad(dense, (x1, x2), grad_outputs=wd)
    return dense.detach()[r, c], g1, g2


@pytest.mark.parametrize("dtype", (torch.float32,) + LOWP)
def test_7_sampled_matmul_values_are_the_sddmm_kernels(mm, cmm, dev, dtype):
    M, K, N = 3000, 2500, 64
    g = np.random.Generator(np.random.PCG64(51))
    a = random_pattern(M, K, g.integers(0, 60, size=M), 52, dev)
    tg = torch.Generator(device=dev).manual_seed(53)
    m1 = torch.randn(M, N, device=dev, generator=tg).to(dtype)
    m2t = torch.randn(K, N, device=dev, generator=tg).to(dtype)
    out = mm.sampled_matmul(a, m1, m2t)
    assert out.layout == torch.sparse_csr and out.dtype == dtype and out.shape == a.shape
    assert out.col_indices().data_ptr() == a.col_indices().data_ptr()
    nnz = a.values().numel()
    direct = cmm.sddmm(a.col_indices().int(), a.crow_indices().int(), nnz, M, K, m1, m2t)
    assert_same_bits(out.values(), direct, f"sampled_matmul vs sddmm, {dtype}")
    if dtype == torch.float32:
        crow, col = a.crow_indices().cpu(), a.col_indices().cpu()
        def ref(dt):
            pat = torch.sparse_csr_tensor(crow, col, torch.zeros(nnz, dtype=dt), size=(M, K))
            return torch.sparse.sampled_addmm(pat, m1.cpu().to(dt), m2t.cpu().to(dt).T.contiguous(), beta=0.0).values()
        v64 = ref(torch.float64)
        assert_under_rule("sampled_matmul forward", scaled_err(ref(torch.float32).numpy(), v64.numpy()),
                          scaled_err(out.values().cpu().numpy(), v64.numpy()))


def test_7_batched_sampled_matmul_values_are_the_sddmm_kernels(mm, cmm, dev):
    a = device_pattern(dev, (2, 3), 128, 0.2, 54)
    tg = torch.Generator(device=dev).manual_seed(55)
    m1, m2t = (torch.randn(2, 3, 128, 32, device=dev, generator=tg) for _ in range(2))
    out = mm.sampled_matmul(a, m1, m2t)
    assert out.values().shape == a.values().shape
    # the block-diagonal form of the batch through the 2-d kernel: what matmuls falls back to, the same bits
    flat_off, diag_col = mm._batched_transposed(a, dev)[:2]
    total = a.values().numel()
    direct = cmm.sddmm(diag_col, flat_off, total, 6 * 128, 6 * 128, m1.reshape(-1, 32), m2t.reshape(-1, 32))
    assert_same_bits(out.values().reshape(-1), direct, "batched sampled_matmul vs sddmm on the block-diagonal matrix")
    per_item = torch.cat([cmm.sddmm(a.col_indices().reshape(6, -1)[i].int(), a.crow_indices().reshape(6, -1)[i].int(),
                                    total // 6, 128, 128, m1.reshape(6, 128, 32)[i], m2t.reshape(6, 128, 32)[i]) for i in range(6)])
    assert_same_bits(out.values().reshape(-1), per_item, "batched sampled_matmul vs per-item sddmm")


@pytest.mark.parametrize("case", ["sorted", "unsorted", "empty rows and columns"])
def test_8_sampled_matmul_gradients(mm, dev, case):
    M, K, N = 1500, 1200, 48
    g = np.random.Generator(np.random.PCG64(61))
    lens = g.integers(1, 50, size=M)
    if case == "empty rows and columns":
        lens[g.random(M) < 0.3] = 0
        rows = [np.sort(g.choice(K // 2, int(n), replace=False)) * 2 for n in lens]  # odd columns stay empty
        a = csr_from_rows(rows, M, K, dev)
    else:
        a = random_pattern(M, K, lens, 62, dev, shuffle=case == "unsorted")
    tg = torch.Generator(device=dev).manual_seed(63)
    m1 = torch.randn(M, N, device=dev, generator=tg, requires_grad=True)
    m2t = torch.randn(K, N, device=dev, generator=tg, requires_grad=True)
    w = torch.randn(a.values().numel(), device=dev, generator=tg)
    runs = []
    for _ in range(2):
        out = mm.sampled_matmul(a, m1, m2t)
        runs.append(torch.autograd.grad(out, (m1, m2t), grad_outputs=with_values(a, w)))
    assert_same_bits(runs[0][0], runs[1][0], "grad m1, run to run")
    assert_same_bits(runs[0][1], runs[1][1], "grad m2t, run to run")
    v64, g1_64, g2_64 = cpu_sampled(a, m1.detach(), m2t.detach(), w, torch.float64)
    v32, g1_32, g2_32 = cpu_sampled(a, m1.detach(), m2t.detach(), w, torch.float32)
    assert_under_rule(f"sampled_matmul values, {case}", scaled_err(v32.numpy(), v64.numpy()),
                      scaled_err(out.values().detach().cpu().numpy(), v64.numpy()))
    assert_under_rule(f"sampled_matmul grad m1, {case}", scaled_err(g1_32.numpy(), g1_64.numpy()),
                      scaled_err(runs[0][0].cpu().numpy(), g1_64.numpy()))
    assert_under_rule(f"sampled_matmul grad m2t, {case}", scaled_err(g2_32.numpy(), g2_64.numpy()),
                      scaled_err(runs[0][1].cpu().numpy(), g2_64.numpy()))
    if case == "empty rows and columns":
        assert (runs[0][0][torch.from_numpy(lens == 0).to(dev)] == 0).all() and (runs[0][1][1::2] == 0).all()


def cpu_dense_attention(q, k, v, mask, scale, w, dtype):
    """torch-CPU autograd of softmax(scale · q·kᵀ with −inf outside the pattern) · v in `dtype`: (out, dq, dk, dv)."""
    xs = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (q, k, v)]
    s = (xs[0] @ xs[1].transpose(-1, -2)) * scale
    s = s.masked_fill(~mask, -float("inf"))
    out = torch.softmax(s, -1) @ xs[2]
    grads = torch.autograd.grad(out, xs, grad_outputs=w.cpu().to(dtype))
    return (out.detach(),) + tuple(grads)


def check_attention(mm, dev, what, a, D, seed):
    shape = tuple(a.shape[:-1]) + (D,)
    tg = torch.Generator(device=dev).manual_seed(seed)
    q, k, v = (torch.randn(shape, device=dev, generator=tg, requires_grad=True) for _ in range(3))
    w = torch.randn(shape, device=dev, generator=tg)
    out = mm.sparse_attention(q, k, v, a)
    assert out.shape == shape and out.dtype == torch.float32
    got = (out.detach(),) + torch.autograd.grad(out, (q, k, v), grad_outputs=w)
    mask = dense_mask(a).bool()
    assert mask.any(-1).all()  # every row keeps an entry: the dense expression has no NaN rows
    scale = 1.0 / D ** 0.5
    ref64 = cpu_dense_attention(q, k, v, mask, scale, w, torch.float64)
    ref32 = cpu_dense_attention(q, k, v, mask, scale, w, torch.float32)
    for name, g, r32, r64 in zip(("out", "grad q", "grad k", "grad v"), got, ref32, ref64):
        assert_under_rule(f"sparse_attention {what}, {name}", scaled_err(r32.numpy(), r64.numpy()),
                          scaled_err(g.cpu().numpy(), r64.numpy()))


def test_9_sparse_attention_on_a_graph_like_pattern(mm, dev):
    S = 20000
    g = np.random.Generator(np.random.PCG64(71))
    lens = np.minimum(1 + (4 * g.pareto(1.5, size=S)).astype(np.int64), 3000)  # Pareto degrees, every node keeps an edge
    check_attention(mm, dev, "graph 20000 nodes", random_pattern(S, S, lens, 72, dev), 64, 73)


def test_9_sparse_attention_batched(mm, dev):
    check_attention(mm, dev, "[2, 4, 512, 512] at 10 %", device_pattern(dev, (2, 4), 512, 0.10, 74), 64, 75)


def test_9_full_pattern_meets_the_dense_attention_criterion(mm, dev):
    """Every entry kept, [2, 2, 128, 64]: against torch's dense attention on the device under the criterion
    benchmarks/bert_attention.py uses (rtol 1e-5, atol 1e-6)."""
    a = device_pattern(dev, (2, 2), 128, 1.0, 76)
    tg = torch.Generator(device=dev).manual_seed(77)
    q, k, v = (torch.randn(2, 2, 128, 64, device=dev, generator=tg, requires_grad=True) for _ in range(3))
    w = torch.randn(2, 2, 128, 64, device=dev, generator=tg)
    out = mm.sparse_attention(q, k, v, a)
    got = (out,) + torch.autograd.grad(out, (q, k, v), grad_outputs=w)
    ref = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v
    want = (ref,) + torch.autograd.grad(ref, (q, k, v), grad_outputs=w)
    for name, x, r in zip(("out", "grad q", "grad k", "grad v"), got, want):
        assert torch.allclose(x, r, rtol=1e-5, atol=1e-6), (name, float((x - r).abs().max()))


@pytest.mark.parametrize("dtype", LOWP)
def test_10_low_precision_attention_is_the_float32_stages_narrowed_once(mm, cmm, dev, dtype):
    S, D = 2000, 64
    g = np.random.Generator(np.random.PCG64(81))
    a = random_pattern(S, S, g.integers(1, 80, size=S), 82, dev)
    tg = torch.Generator(device=dev).manual_seed(83)
    q, k, v = (torch.randn(S, D, device=dev, generator=tg).to(dtype).requires_grad_(True) for _ in range(3))
    w = torch.randn(S, D, device=dev, generator=tg).to(dtype)
    out = mm.sparse_attention(q, k, v, a)
    grads = torch.autograd.grad(out, (q, k, v), grad_outputs=w)
    assert out.dtype == dtype and all(x.dtype == dtype and x.shape == q.shape for x in grads)
    # stage by stage: each equals the float32 stage on its widened inputs, narrowed once
    col, off, nnz = a.col_indices().int(), a.crow_indices().int(), a.values().numel()
    scale = 1.0 / D ** 0.5
    s_t = mm.sampled_matmul(a, q.detach(), k.detach()).values()
    assert_same_bits(s_t, cmm.sddmm(col, off, nnz, S, S, q.detach().float(), k.detach().float()).to(dtype), "scores")
    p_t = mm.sparse_softmax(with_values(a, s_t), scale).values()
    p_32 = cmm.csr_softmax(s_t.float(), off, nnz, 1, S, scale, torch.empty(nnz, device=dev))
    assert_same_bits(p_t, p_32.to(dtype), "probabilities")
    # (the two products are the existing low-precision CSR kernels, whose own contract tests/test_gpu_spmm_lowp.py checks)
    o_t = cmm.naive_spmm_ex(p_t, col, off, nnz, S, S, v.detach(), torch.empty(S, D, device=dev, dtype=dtype), 0)
    assert_same_bits(out.detach(), o_t, "context")
    # the softmax gradient stage on what the product's backward hands it
    dp_t = cmm.sddmm(col, off, nnz, S, S, w, v.detach())
    ds_t = cmm.csr_softmax_backward(p_t, dp_t, off, nnz, 1, S, scale, torch.empty_like(p_t))
    ds_32 = cmm.csr_softmax_backward(p_t.float(), dp_t.float(), off, nnz, 1, S, scale, torch.empty(nnz, device=dev))
    assert_same_bits(ds_t, ds_32.to(dtype), "softmax gradient")
    dq_t = cmm.naive_spmm(ds_t, col, off, nnz, S, S, k.detach(), torch.empty(S, D, device=dev, dtype=dtype))
    assert_same_bits(grads[0], dq_t, "grad q")
    # the batched low-precision call raises the documented error
    b = device_pattern(dev, (2,), 64, 0.5, 84)
    x = torch.randn(2, 64, 16, device=dev).to(dtype)
    with pytest.raises(RuntimeError, match=r"a batched .* CSR pattern \(3-d\) is not supported \(float32 only\)"):
        mm.sparse_attention(x, x, x, b)
