"""matmuls.fused_sparse_attention on the MI355X: forward and the three gradients have the bits of matmuls.sparse_attention
(the three-kernel composition) in float32, bfloat16 and float16, 2-d and batched — a bfloat16 / float16 batch those of the
2-d sparse_attention item by item —, across the row-length edges of the lane forms and the streamed rows, for every head
size class, with special values; the float32 step is held to the e_dev ≤ 8 · e_ref rule, and autograd keeps no
nnz-sized tensor."""
import numpy as np
import pytest
import torch

from gpu_helpers import assert_same_bits
from sparse_attention_helpers import assert_under_rule, dense_mask, device_pattern, scaled_err

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
DTYPES = (torch.float32,) + LOWP


def csr_from_rows(rows_cols, M, K, dev):
    """A CSR tensor (values 1) from a list of per-row column arrays, kept in the order given (unsorted allowed)."""
    lens = [len(c) for c in rows_cols]
    crow = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
    col = torch.tensor(np.concatenate(rows_cols) if sum(lens) else np.zeros(0), dtype=torch.int64)
    return torch.sparse_csr_tensor(crow.to(dev), col.to(dev), torch.ones(len(col), device=dev), size=(M, K))


def pattern_of(lens, K, seed, dev, shuffle=True):
    g = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for n in lens:
        c = np.arange(K) if n == K else np.sort(g.choice(K, int(n), replace=False))
        rows.append(g.permutation(c) if shuffle else c)
    return csr_from_rows(rows, len(lens), K, dev)


def operands(dev, shape, dtype, seed):
    tg = torch.Generator(device=dev).manual_seed(seed)
    q, k, v = (torch.randn(shape, device=dev, generator=tg).to(dtype).requires_grad_(True) for _ in range(3))
    return q, k, v, torch.randn(shape, device=dev, generator=tg).to(dtype)


def step(fn, q, k, v, a, w, scale=None):
    """(out, dq, dk, dv) of one forward + backward."""
    out = fn(q, k, v, a, scale)
    return (out.detach(),) + torch.autograd.grad(out, (q, k, v), grad_outputs=w)


def assert_same_step(got, want, what):
    for name, g, w in zip(("out", "dq", "dk", "dv"), got, want):
        assert_same_bits(g, w, f"{what}: {name}")


def per_item(mm, q, k, v, a, w, scale=None):
    """The 2-d sparse_attention applied item by item to a batch: (out, dq, dk, dv) stacked."""
    S, D = a.shape[-2], q.shape[-1]
    crow, col = a.crow_indices().reshape(-1, S + 1), a.col_indices().reshape(crow_rows(a), -1)
    parts = []
    for i in range(crow.shape[0]):
        ai = torch.sparse_csr_tensor(crow[i].contiguous(), col[i].contiguous(), torch.ones(col.shape[1], device=col.device), size=(S, S))
        qi, ki, vi = (t.detach().reshape(-1, S, D)[i].clone().requires_grad_(True) for t in (q, k, v))
        parts.append(step(mm.sparse_attention, qi, ki, vi, ai, w.reshape(-1, S, D)[i], scale))
    return tuple(torch.stack(p).reshape(q.shape) for p in zip(*parts))


def crow_rows(a):
    return a.crow_indices().reshape(-1, a.shape[-2] + 1).shape[0]


EDGE_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)


@pytest.mark.parametrize("dtype", DTYPES)
def test_1_two_d_step_has_the_bits_of_the_composition(mm, dev, dtype):
    S, D = 300, 64
    assert mm.fused_attention_takes(dtype, D)
    g = np.random.Generator(np.random.PCG64(131))
    lens = g.integers(0, 301, size=S)
    lens[:len(EDGE_LENS)] = EDGE_LENS
    a = pattern_of(lens, S, 132, dev, shuffle=True)
    q, k, v, w = operands(dev, (S, D), dtype, 133)
    want = step(mm.sparse_attention, q, k, v, a, w)
    got = step(mm.fused_sparse_attention, q, k, v, a, w)
    assert got[0].dtype == dtype and got[0].shape == (S, D)
    assert_same_step(got, want, f"2-d {dtype}")
    assert_same_step(step(mm.fused_sparse_attention, q, k, v, a, w), got, f"2-d {dtype}, run to run")
    assert (got[0][0] == 0).all() and (got[1][0] == 0).all()  # the empty row


@pytest.mark.parametrize("dtype,D,kernel", [(torch.float32, 8, True), (torch.float32, 12, True), (torch.float32, 64, True),
                                           (torch.float32, 100, True), (torch.float32, 128, True), (torch.float32, 4, False),
                                           (torch.float32, 6, False), (torch.float32, 260, False), (torch.bfloat16, 8, True),
                                           (torch.bfloat16, 64, True), (torch.bfloat16, 120, True), (torch.float16, 8, True),
                                           (torch.float16, 64, True), (torch.float16, 120, True)])
def test_2_head_sizes(mm, dev, dtype, D, kernel):
    M, S = 97, 96  # a row of every length 0 … 96
    assert mm.fused_attention_takes(dtype, D) == kernel
    a = pattern_of(np.arange(M), S, 141, dev)
    tg = torch.Generator(device=dev).manual_seed(143 + D)
    q, w = (torch.randn(M, D, device=dev, generator=tg).to(dtype) for _ in range(2))
    k, v = (torch.randn(S, D, device=dev, generator=tg).to(dtype).requires_grad_(True) for _ in range(2))
    q.requires_grad_(True)
    assert_same_step(step(mm.fused_sparse_attention, q, k, v, a, w), step(mm.sparse_attention, q, k, v, a, w), f"D = {D} {dtype}")


def test_2_a_batched_low_precision_call_needs_a_head_size_the_kernel_takes(mm, dev):
    a = device_pattern(dev, (2,), 16, 0.5, 145)
    q, k, v, _ = operands(dev, (2, 16, 6), torch.bfloat16, 146)
    with pytest.raises(RuntimeError, match=r"fused_sparse_attention: a batched torch.bfloat16 pattern needs a head size that is a "
                                           r"multiple of 8 from 8 to 128, got 6"):
        mm.fused_sparse_attention(q, k, v, a)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_3_long_rows_are_streamed_with_the_same_bits(mm, cmm, dev, dtype):
    S, D = 4608, 8
    assert S < cmm.long_row_threshold()  # below the split of the composed 2-d product
    g = np.random.Generator(np.random.PCG64(151))
    lens = g.integers(0, 17, size=S)
    lens[5], lens[77], lens[4000] = S, 2049, 4097
    a = pattern_of(lens, S, 152, dev, shuffle=False)
    q, k, v, w = operands(dev, (S, D), dtype, 153)
    assert_same_step(step(mm.fused_sparse_attention, q, k, v, a, w), step(mm.sparse_attention, q, k, v, a, w),
                     f"long rows {dtype}")


def test_4_batched_float32(mm, dev):
    a = device_pattern(dev, (2, 3), 128, 0.2, 161)
    q, k, v, w = operands(dev, (2, 3, 128, 32), torch.float32, 162)
    got = step(mm.fused_sparse_attention, q, k, v, a, w)
    assert_same_step(got, step(mm.sparse_attention, q, k, v, a, w), "batched float32")
    # item 4 alone, as a 2-d call: the bits of its slice
    crow, col = a.crow_indices().reshape(6, -1)[4], a.col_indices().reshape(6, -1)[4]
    a4 = torch.sparse_csr_tensor(crow.contiguous(), col.contiguous(), torch.ones(col.numel(), device=dev), size=(128, 128))
    q4, k4, v4 = (t.detach().reshape(6, 128, 32)[4].clone().requires_grad_(True) for t in (q, k, v))
    alone = step(mm.fused_sparse_attention, q4, k4, v4, a4, w.reshape(6, 128, 32)[4])
    assert_same_step(alone, tuple(t.reshape(6, 128, 32)[4] for t in got), "item 4 alone")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("batch,S,keep,D", [((2,), 64, 0.5, 16), ((2, 2), 128, 0.3, 64)])
def test_5_batched_low_precision_equals_the_two_d_composition_item_by_item(mm, dev, dtype, batch, S, keep, D):
    assert mm.fused_attention_takes(dtype, D)
    a = device_pattern(dev, batch, S, keep, 171)
    q, k, v, w = operands(dev, batch + (S, D), dtype, 172)
    got = step(mm.fused_sparse_attention, q, k, v, a, w)
    assert got[0].dtype == dtype
    assert_same_step(got, per_item(mm, q, k, v, a, w), f"batched {dtype} {batch}")


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16))
def test_6_special_values(mm, dev, dtype):
    S, D = 64, 8
    g = np.random.Generator(np.random.PCG64(181))
    rows = [np.sort(g.choice(S, 12, replace=False)) for _ in range(S)]
    rows[9] = np.array([7])  # a row whose only entry is the −inf column
    if not any(7 in r for i, r in enumerate(rows) if i != 9):
        rows[3] = np.sort(np.unique(np.append(rows[3], 7)))
    a = csr_from_rows(rows, S, S, dev)
    tg = torch.Generator(device=dev).manual_seed(182)
    q = torch.rand(S, D, device=dev, generator=tg) + 0.5  # q > 0: a −inf row of k gives −inf scores, never NaN
    k = torch.randn(S, D, device=dev, generator=tg)
    k[7] = -float("inf")
    q[20, 3] = float("nan")
    v, w = torch.randn(S, D, device=dev, generator=tg), torch.randn(S, D, device=dev, generator=tg)
    q, k, v = (t.to(dtype).requires_grad_(True) for t in (q, k, v))
    w = w.to(dtype)
    got = step(mm.fused_sparse_attention, q, k, v, a, w)
    assert_same_step(got, step(mm.sparse_attention, q, k, v, a, w), f"special values {dtype}")
    out = got[0].float().cpu()
    bad = torch.isnan(out).any(-1)
    assert bad.nonzero().flatten().tolist() == [9, 20]  # exactly the all-−inf row and the NaN row
    assert torch.isfinite(out[~bad]).all()


def test_7_accuracy_float32(mm, dev):
    S, D = 512, 64
    a = device_pattern(dev, (), S, 50 / S, 191)
    q, k, v, w = operands(dev, (S, D), torch.float32, 192)
    mask, scale = dense_mask(a), 1.0 / D ** 0.5

    def cpu(dtype):
        xs = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (q, k, v)]
        s = ((xs[0] @ xs[1].T) * scale).masked_fill(~mask, -float("inf"))
        out = torch.softmax(s, -1) @ xs[2]
        return (out.detach(),) + torch.autograd.grad(out, xs, grad_outputs=w.cpu().to(dtype))

    r64, r32 = cpu(torch.float64), cpu(torch.float32)
    composed = step(mm.sparse_attention, q, k, v, a, w)
    fused = step(mm.fused_sparse_attention, q, k, v, a, w)
    for name, x64, x32, c, f in zip(("out", "dq", "dk", "dv"), r64, r32, composed, fused):
        e_ref = scaled_err(x32.numpy(), x64.numpy())
        # the composed path first: the margin is not new
        assert_under_rule(f"sparse_attention {name}", e_ref, scaled_err(c.cpu().numpy(), x64.numpy()))
        assert_under_rule(f"fused_sparse_attention {name}", e_ref, scaled_err(f.cpu().numpy(), x64.numpy()))


def saved_bytes(fn, q, k, v, a):
    """Bytes of the distinct storages autograd keeps for one forward, beyond q, k, v and the pattern's own tensors."""
    own = {t.untyped_storage().data_ptr() for t in (q, k, v, a.crow_indices(), a.col_indices(), a.values())}
    seen = {}

    def pack(t):
        parts = (t.crow_indices(), t.col_indices(), t.values()) if t.layout == torch.sparse_csr else (t,)
        for p in parts:
            st = p.untyped_storage()
            if st.data_ptr() not in own:
                seen[st.data_ptr()] = st.nbytes()
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = fn(q, k, v, a)
    del out
    return sum(seen.values())


def test_8_autograd_keeps_nothing_of_the_size_of_the_pattern(mm, dev):
    """Distinct storages saved by one forward, beyond q, k, v and the pattern's own tensors: the fused function at most 16
    bytes per row (it keeps 8: the maximum and the reciprocal sum), the composed one the scores and the probabilities —
    measured at exactly 8.00 bytes per entry (819200 B for 102400 entries), so its floor is asserted as ≥ 8·nnz: the two
    value arrays are all it keeps, every CSR result sits on the pattern's own index tensors."""
    S, D, nb = 512, 64, 4
    a = device_pattern(dev, (nb,), S, 50 / S, 201)
    nnz = a.values().numel()
    q, k, v, _ = operands(dev, (nb, S, D), torch.float32, 202)
    composed = saved_bytes(mm.sparse_attention, q, k, v, a)
    fused = saved_bytes(mm.fused_sparse_attention, q, k, v, a)
    print(f"saved beyond the operands: composed {composed} B ({composed / nnz:.2f} per entry), fused {fused} B "
          f"({fused / (nb * S):.2f} per row)")
    assert fused <= 16 * nb * S
    assert composed >= 8 * nnz  # scores and probabilities, 4 bytes per entry each: the count can tell the difference
