"""matmuls.fused_sparse_attention on the MI355X: forward and the three gradients have the bits of matmuls.sparse_attention
(the three-kernel composition) in float32, bfloat16 and float16, 2-d and batched — a bfloat16 / float16 batch those of the
2-d sparse_attention item by item —, across the row-length edges of the lane forms and the streamed rows, for every head
size class, with special values; the float32 step is held to the e_dev ≤ 8 · e_ref rule, and autograd keeps no
nnz-sized tensor.  Against dense masked attention in float64, under that rule, in all three dtypes: rectangular batches
(M ≠ K, so q's item stride differs from k's) at every lane-group width, and the row-length edges up to the streamed rows,
class of rows by class of rows.  Through the C ABI: every dense operand with a leading dimension and an item stride of
its own, NaN around the inputs and a sentinel around the outputs, and k, v shared by the batch (item stride 0)."""
import numpy as np
import pytest
import torch

from gpu_helpers import (SENTINEL, assert_outside_untouched, assert_same_bits, padded,
                         _sparse_attention_backward_through_the_c_abi, _sparse_attention_through_the_c_abi)
from sparse_attention_helpers import (assert_tensor_under_rule, assert_under_rule, assert_under_rule_by_rows, dense_mask,
                                      dense_step, device_pattern, scaled_err)

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


# --------------------------------------------------------------------------- #
# rectangular batches, leading dimensions and strides, row-length edges: against float64
# --------------------------------------------------------------------------- #

NAMES = ("out", "dq", "dk", "dv")
RECT_EDGE_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)


def rect_batch_pattern(dev, nb=3, M=70, K=200, seed=211):
    """A batched pattern [nb, M, K], M ≠ K; nb·M = 210 rows leave the last four-wave workgroup half full.  Every item holds
    the same multiset of row lengths (torch wants equal entry counts per item) — RECT_EDGE_LENS and random ones — at
    rows of its own, with columns of its own in shuffled order.  Returns (pattern, the items' 2-d patterns, the boolean
    CPU mask [nb, M, K] of the stored positions)."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.concatenate([RECT_EDGE_LENS, g.integers(0, K + 1, size=M - len(RECT_EDGE_LENS))])
    crows, cols, items = [], [], []
    mask = torch.zeros((nb, M, K), dtype=torch.bool)
    for i in range(nb):
        mine = g.permutation(lens)
        rows = [g.permutation(K)[:n] if n < K else g.permutation(K) for n in mine]
        crows.append(np.concatenate([[0], np.cumsum(mine)]))
        cols.append(np.concatenate(rows))
        items.append(csr_from_rows(rows, M, K, dev))
        for r, c in enumerate(rows):
            mask[i, r, torch.from_numpy(c)] = True
    crow, col = torch.tensor(np.stack(crows), dtype=torch.int64, device=dev), torch.tensor(np.stack(cols), dtype=torch.int64, device=dev)
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape, device=dev), size=(nb, M, K)), items, mask


def rect_operands(dev, lead, M, K, D, dtype, seed, q_times=1.0):
    """q, w [*lead, M, D] and k, v [*lead, K, D], drawn on the CPU (the same values wherever the test runs)."""
    tg = torch.Generator().manual_seed(seed)
    q, w = (torch.randn(lead + (M, D), generator=tg) for _ in range(2))
    k, v = (torch.randn(lead + (K, D), generator=tg) for _ in range(2))
    q = q * q_times
    q, k, v = (t.to(dtype).to(dev).requires_grad_(True) for t in (q, k, v))
    return q, k, v, w.to(dtype).to(dev)


def references(q, k, v, w, mask, scale):
    """(float64 reference, yardstick) of one step: the yardstick is the same expression in torch-CPU float32, for a
    bfloat16 / float16 step narrowed once after the scores, the probabilities and the product."""
    narrow = None if q.dtype == torch.float32 else q.dtype
    return dense_step(q, k, v, w, mask, scale, torch.float64), dense_step(q, k, v, w, mask, scale, torch.float32, narrow=narrow)


@pytest.mark.parametrize("dtype,D,scale", [(torch.float32, 8, None), (torch.float32, 24, None), (torch.float32, 72, None),
                                           (torch.float32, 128, None), (torch.float32, 24, 0.2), (torch.bfloat16, 8, None),
                                           (torch.bfloat16, 40, None), (torch.bfloat16, 120, None), (torch.float16, 8, None),
                                           (torch.float16, 40, None), (torch.float16, 120, None)])
def test_9_rectangular_batch_against_float64_and_item_by_item(mm, dev, dtype, D, scale):
    nb, M, K = 3, 70, 200
    assert mm.fused_attention_takes(dtype, D)
    a, items, mask = rect_batch_pattern(dev, nb, M, K)
    q, k, v, w = rect_operands(dev, (nb,), M, K, D, dtype, 212 + D)
    got = step(mm.fused_sparse_attention, q, k, v, a, w, scale)
    assert got[0].dtype == dtype and got[0].shape == (nb, M, D) and got[2].shape == (nb, K, D)
    r64, yard = references(q, k, v, w, mask, 1.0 / D ** 0.5 if scale is None else scale)
    for name, g, y, r in zip(NAMES, got, yard, r64):
        assert_tensor_under_rule(f"fused rectangular batch {dtype} D={D} scale={scale} {name}", g, y, r)
    for i in range(nb):
        qi, ki, vi = (t.detach()[i].clone().requires_grad_(True) for t in (q, k, v))
        alone = step(mm.fused_sparse_attention, qi, ki, vi, items[i], w[i], scale)
        assert_same_step(tuple(g[i] for g in got), alone, f"rectangular batch {dtype} D={D}, item {i} alone")
    empty = ~mask.any(-1)
    assert empty.sum() >= nb
    assert (got[0].cpu()[empty] == 0).all() and (got[1].cpu()[empty] == 0).all()


def c_abi_case(mm, cmm, capi, dev, dtype, D, step=8):
    """The rectangular batch of test_9 through the C ABI: every dense operand in a buffer of its own with its own leading
    dimension and item stride (operand number i: ld = D + step·(i + 1), stride = rows · ld + step·(i + 1); step = 4 puts
    rows of a 2-byte dtype on 8-byte boundaries only, the least the fused T entries take), NaN around the inputs,
    a sentinel around the outputs; every logical output has the bits of the packed call through custom_mm.  Then k, v
    shared by the batch: item stride 0 on one item equals the packed call on that item expanded."""
    nb, M, K = 3, 70, 200
    nan = float("nan")
    a, _, _ = rect_batch_pattern(dev, nb, M, K)
    offsets, columns, nnz, batch = mm._attention_pattern(a, dev, mm._csr_state(a))
    assert batch == nb and columns.numel() == nnz
    q, k, v, w = (t.detach() for t in rect_operands(dev, (nb,), M, K, D, dtype, 221 + D))
    scale = 1.0 / D ** 0.5

    def packed(k3, v3):
        out, dq = torch.full_like(q, nan), torch.full_like(q, nan)
        stats = torch.full((nb * M, 2), nan, device=dev)
        y, ds = torch.full((nnz,), nan, device=dev, dtype=dtype), torch.full((nnz,), nan, device=dev, dtype=dtype)
        cmm.sparse_attention_fwd(offsets, columns, nnz, nb, M, K, q, k3, v3, scale, out, stats)
        cmm.sparse_attention_bwd(offsets, columns, nnz, nb, M, K, q, k3, v3, w, stats, scale, dq, y, ds)
        return out, stats, dq, y, ds

    def strided(k3, v3, kv_stride, what):
        pq, pk, pv, pw = padded(q, 0, nan, step), padded(k3, 1, nan, step), padded(v3, 2, nan, step), padded(w, 4, nan, step)
        pout = padded(torch.full_like(q, SENTINEL), 3, SENTINEL, step)
        pdq = padded(torch.full_like(q, SENTINEL), 5, SENTINEL, step)
        if step * q.element_size() == 8:  # q, v, dout: rows off the 16-byte boundaries
            assert all((p.ld * q.element_size()) % 16 == 8 and (p.stride * q.element_size()) % 16 == 8 for p in (pq, pv, pw))
        stats = torch.full((nb * M, 2), nan, device=dev)
        y, ds = torch.full((nnz,), nan, device=dev, dtype=dtype), torch.full((nnz,), nan, device=dev, dtype=dtype)
        st = _sparse_attention_through_the_c_abi(capi, dtype, offsets, columns, nb, M, K, D, pq, pk, pv, scale, pout, stats,
                                                 kv_stride)
        assert st == 0, (what, st)
        st = _sparse_attention_backward_through_the_c_abi(capi, dtype, offsets, columns, nb, M, K, D, pq, pk, pv, pw, stats, scale,
                                                          pdq, y, ds, kv_stride)
        assert st == 0, (what, st)
        torch.cuda.synchronize()
        assert_outside_untouched(pout, f"{what}: out")
        assert_outside_untouched(pdq, f"{what}: dq")
        return pout.x, stats, pdq.x, y, ds

    def compare(got, want, what):
        for name, g, x in zip(("out", "stats", "dq", "y", "dS"), got, want):
            assert_same_bits(g, x, f"{what}: {name}")
            assert not torch.isnan(g.float()).any(), (what, name)  # both calls start from NaN: equal bits alone would pass

    compare(strided(k, v, None, "own ld and strides"), packed(k, v), f"{dtype} D={D}, own ld and strides")
    k1, v1 = k[1:2], v[1:2]  # one k, v for the whole batch
    compare(strided(k1, v1, 0, "shared k, v"), packed(k1.expand(nb, K, D).contiguous(), v1.expand(nb, K, D).contiguous()),
            f"{dtype} D={D}, strideK = strideV = 0")


def test_10_leading_dimensions_and_strides_float32(mm, cmm, capi, dev):
    c_abi_case(mm, cmm, capi, dev, torch.float32, 72)


@pytest.mark.parametrize("step", (8, 4))  # rows on 16-byte boundaries; rows of q, v, dout on 8-byte boundaries only
@pytest.mark.parametrize("dtype", LOWP)
def test_10_leading_dimensions_and_strides_low_precision(mm, cmm, capi, dev, dtype, step):
    c_abi_case(mm, cmm, capi, dev, dtype, 120, step)


EDGE_M, EDGE_K = 384, 4608
EDGE_CLASSES = (("lanes", tuple(range(131))), ("around 1024", (1023, 1024, 1025) * 3), ("1025-2048", (1500, 2047, 2048) * 3),
                ("streamed", (2049, 4097, 4608) * 3))


def edge_rows(seed=231):
    """The rows of the row-length edge pattern [384, 4608] as column arrays, and its classes {name: row indices}: "lanes"
    0 … 130 entries, "around 1024" (the backward's slice: 1023, 1024, 1025), "1025-2048" (the backward streams, the
    forward does not: 1500, 2047, 2048) and "streamed" (both stream: 2049, 4097, 4608 = K), every other row 1 … 16
    entries; the rows sit at shuffled positions.  Rows beyond 130 entries keep sorted columns, a third of the others are
    shuffled."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens, names = [], []
    for name, ls in EDGE_CLASSES:
        lens += list(ls)
        names += [name] * len(ls)
    rest = EDGE_M - len(lens)
    lens += list(g.integers(1, 17, size=rest))
    names += ["short"] * rest
    order = g.permutation(EDGE_M)
    lens, names = np.asarray(lens)[order], np.asarray(names)[order]
    rows = []
    for n in lens:
        c = np.arange(EDGE_K) if n == EDGE_K else np.sort(g.choice(EDGE_K, int(n), replace=False))
        rows.append(g.permutation(c) if n <= 130 and g.random() < 1 / 3 else c)
    classes = {name: np.nonzero(names == name)[0] for name, _ in EDGE_CLASSES}
    return rows, classes


def edge_case(dev, dtype, D):
    """(pattern, classes, q, k, v, w, float64 reference, yardstick) of the row-length edge case, with what the case relies
    on checked on the CPU: q is randn · 2, so the scores (scale 1/√D) have deviation 2 and a long row's spread is about
    20 — its probabilities far from one-hot: the sum and the rescaling matter."""
    rows, classes = edge_rows()
    a = csr_from_rows(rows, EDGE_M, EDGE_K, dev)
    q, k, v, w = rect_operands(dev, (), EDGE_M, EDGE_K, D, dtype, 232 + D, q_times=2.0)
    mask = torch.zeros((EDGE_M, EDGE_K), dtype=torch.bool)
    for r, c in enumerate(rows):
        mask[r, torch.from_numpy(np.asarray(c, np.int64))] = True
    scale = 1.0 / D ** 0.5
    r64, yard = references(q, k, v, w, mask, scale)
    assert all(len(c) >= 8 for c in classes.values())
    assert all(torch.isfinite(x).all() for x in r64)
    s64 = (scale * (q.detach().cpu().double() @ k.detach().cpu().double().T)).masked_fill(~mask, -float("inf"))
    long_rows = np.concatenate([classes[n] for n in ("around 1024", "1025-2048", "streamed")])
    p_long = torch.softmax(s64[long_rows], -1)
    assert p_long.max() < 0.9
    spread = (s64[long_rows].max(-1).values - s64[long_rows].masked_fill(~mask[long_rows], float("inf")).min(-1).values)
    assert 10 < spread.median() < 30, spread.median()
    for name in ("out", "dq"):
        i = NAMES.index(name)
        for cname, idx in classes.items():
            e = scaled_err(yard[i].double().numpy()[idx], r64[i].numpy()[idx])
            assert np.isfinite(e) and e > 0, (name, cname, e)
    return a, classes, q, k, v, w, r64, yard


@pytest.mark.parametrize("dtype,D", [(torch.float32, 72), (torch.bfloat16, 64), (torch.float16, 120)])
def test_11_row_length_edges_against_float64(mm, cmm, dev, dtype, D):
    assert EDGE_K < cmm.long_row_threshold()  # below the split of the composed 2-d product
    a, classes, q, k, v, w, r64, yard = edge_case(dev, dtype, D)
    got = step(mm.fused_sparse_attention, q, k, v, a, w)
    what = f"fused row-length edges {dtype} D={D}"
    for name, g, y, r in zip(NAMES, got, yard, r64):
        if name in ("out", "dq"):
            assert_under_rule_by_rows(f"{what} {name}", g, y, r, classes)
        else:
            assert_tensor_under_rule(f"{what} {name}", g, y, r)
    assert_same_step(got, step(mm.sparse_attention, q, k, v, a, w), what)
