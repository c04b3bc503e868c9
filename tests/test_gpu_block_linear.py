"""matmuls.block_sparse_linear / fc_layers.blockSparseLinear on the MI355X: y = x·Wᵀ + bias with W in kept 64 × 64 blocks,
d x, d values and d bias.

The contract (include/mi_spmm.h, mi_bsr_linear / mi_bsr_wgrad — DESIGN.md §3.16): every product on the MFMA with fp32
accumulators, ONE accumulator per output element from +0 through the kept blocks in ascending order, the bias added in
fp32, one rounding at the store — the instruction and the order of this package's dense low-precision product, with the
unkept blocks left out; the weight gradient with the deterministic split of the tokens.
  1. exact: integer operands in [−8, 8] keep every fp32 partial sum exact, so y, d x, d values and d bias are the float64
     results narrowed to T, bit for bit; an empty block row gives the bias (or +0), a never-kept block column +0 in d x;
  2. the split, exact: 4096 tokens, sums up to 2¹⁸ — a partial narrowed before the combine would fail;
  3. the same bits as cublas_mmul_bias / cublas_mmul / cublas_mmul_splitk on the densified W, and as cublasLinear;
  4. a long list (1, 2, 3, 40 kept blocks in one block row) within |C − E| ≤ u_T·|E| + k·2⁻²³·S (+ 2⁻²⁵ for fp16);
  5. invariance: leading dimensions, the checked alignment form, the order of the layout, repeated runs;
  6. unkept blocks are never read; 7. graph capture with the split inside; 8. memory.
Of these only 8 at 4096 tokens reaches the 128-token tile (custom_mm.bsr_linear_tile_tokens is the rule), and it asserts memory;
  9. the 128-token tile — 1, 3 and 5 (the position of a token, the checked form and its stores) there:
     tests/test_gpu_lowp_wide_tiles.py;
 10. malformed lists — a column outside the grid, an id outside the values, offsets outside [0, nnz]:
     tests/test_gpu_block_lists_malformed.py.
Here a layout row is a block row of W (out) and a layout column a block column (in).
"""
import ctypes
import sys

import pytest
import torch

from gpu_helpers import assert_same_bits

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ABS = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
NAMES = ("y", "d x", "d values", "d bias")
B = 64

FULL = [[0, 1, 2, 3]] * 4
DIAGONAL = [[0], [1], [2], [3]]
BAND_GLOBAL = [[0], [1, 0], [], [0, 2]]  # block row 2 empty, block column 3 never kept, row 1 unsorted
RECT_UNSORTED = [[3, 0, 4], [4, 1]]     # 2 × 5 blocks
HALF = [[0, 2], [3, 1], [0, 1], [2, 3]]  # 2 of 4 blocks per block row


def layout_from_rows(rows_cols, cols, dev, index_dtype=torch.int64):
    """A 2-d CSR block layout (values 1) from per-block-row column lists, kept in the order given (unsorted allowed)."""
    crow = [0]
    for c in rows_cols:
        crow.append(crow[-1] + len(c))
    col = [j for c in rows_cols for j in c]
    return torch.sparse_csr_tensor(torch.tensor(crow, dtype=index_dtype, device=dev), torch.tensor(col, dtype=index_dtype, device=dev),
                                   torch.ones(len(col), device=dev), size=(len(rows_cols), cols))


def entries(rows_cols):
    return [(i, j) for i, c in enumerate(rows_cols) for j in c]


def densify(values, rows_cols, cols):
    """W [out, in] in the dtype and on the device of values: block (O, I) of stored entry e is values[e], zeros elsewhere."""
    a = torch.zeros(len(rows_cols) * B, cols * B, dtype=values.dtype, device=values.device)
    for e, (i, j) in enumerate(entries(rows_cols)):
        a[i * B:(i + 1) * B, j * B:(j + 1) * B] = values[e]
    return a


def kept_blocks(full, rows_cols):
    """[n, 64, 64]: the blocks of a dense [out, in] at the stored entries."""
    return torch.stack([full[i * B:(i + 1) * B, j * B:(j + 1) * B] for i, j in entries(rows_cols)])


def ints(shape, dev, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype).to(dev)


def randn(shape, dev, dtype, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def step(mm, x, values, layout, bias, w):
    """(y, d x, d values[, d bias]) of one forward + backward on fresh leaves."""
    leaves = [x.detach().requires_grad_(True), values.detach().requires_grad_(True)]
    if bias is not None:
        leaves.append(bias.detach().requires_grad_(True))
    y = mm.block_sparse_linear(leaves[0], leaves[1], layout, leaves[2] if bias is not None else None)
    return (y.detach(),) + torch.autograd.grad(y, leaves, grad_outputs=w)


def assert_same_step(got, want, what):
    assert len(got) == len(want), what
    for name, g, w in zip(NAMES, got, want):
        assert_same_bits(g, w, f"{what}: {name}")


def f64_step(x, values, rows_cols, cols, bias, w):
    """(y, d x, d values[, d bias]) in float64 on the CPU, 2-d x."""
    W = densify(values.cpu().double(), rows_cols, cols)
    x64, w64 = x.cpu().double(), w.cpu().double()
    # (+ 0.0: every sum starts at +0 by contract, so a sum of −0 products is +0 — torch's own products may leave −0)
    y = x64 @ W.T + 0.0
    out = (y if bias is None else y + bias.cpu().double(), w64 @ W + 0.0, kept_blocks(w64.T @ x64, rows_cols) + 0.0)
    return out if bias is None else out + (w64.sum(0) + 0.0,)


def lists_of(mm, layout, dev, rows, cols):
    rec = mm._bsr_layout(layout, dev, mm._csr_state(layout))
    return rec["fwd"], mm._bsr_layout_transposed(rec, rows, cols)


# ---- 1. exact -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("name,rows,cols,index_dtype", [
    ("full", FULL, 4, torch.int64), ("diagonal", DIAGONAL, 4, torch.int64), ("band+global", BAND_GLOBAL, 4, torch.int64),
    ("rect-unsorted", RECT_UNSORTED, 5, torch.int32)])
def test_1_integer_operands_are_exact(mm, cmm, dev, dtype, with_bias, name, rows, cols, index_dtype):
    layout = layout_from_rows(rows, cols, dev, index_dtype)
    n, fout, fin = len(entries(rows)), len(rows) * B, cols * B
    values = ints((n, B, B), dev, dtype, 1)
    bias = ints((fout,), dev, dtype, 4) if with_bias else None
    (offsets, columns, ids, entry_row, _), (t_off, t_col, t_ids) = lists_of(mm, layout, dev, len(rows), cols)
    for T in (1, 8, 40, 64, 136, 200):
        x, w = ints((T, fin), dev, dtype, 2 + T), ints((T, fout), dev, dtype, 3 + T)
        want = tuple(v.to(dtype) for v in f64_step(x, values, rows, cols, bias, w))
        got = step(mm, x, values, layout, bias, w)
        assert_same_step(got, want, f"{name} T={T}")
        # the entries themselves, into outputs pre-filled with NaN: every element is written
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=dtype)  # noqa: E731
        y, dx, dvalues = nan(T, fout), nan(T, fin), nan(n, B, B)
        cmm.bsr_linear(offsets, columns, ids, n, values, x, bias, y, False)
        cmm.bsr_linear(t_off, t_col, t_ids, n, values, w, None, dx, True)
        cmm.bsr_wgrad(entry_row, columns, ids, n, w, x, dvalues)
        assert_same_step((y, dx, dvalues), want[:3], f"{name} T={T}, pre-filled")
        if name == "band+global":
            empty = bias[2 * B:3 * B].expand(T, B) if with_bias else torch.zeros(T, B, dtype=dtype)  # +0, not −0
            assert_same_bits(got[0][:, 2 * B:3 * B], empty, "the empty block row of W in y")
            assert_same_bits(got[1][:, 3 * B:4 * B], torch.zeros(T, B, dtype=dtype), "the never-kept block column in d x")


# ---- 2. the split of the tokens, exact -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_2_split_is_exact(mm, cmm, dev, dtype):
    rows, cols, T = HALF, 4, 4096
    layout = layout_from_rows(rows, cols, dev)
    n = len(entries(rows))
    (offsets, columns, ids, entry_row, _), _ = lists_of(mm, layout, dev, len(rows), cols)
    x, w = ints((T, cols * B), dev, dtype, 21), ints((T, len(rows) * B), dev, dtype, 22)
    want = (kept_blocks(w.cpu().double().T @ x.cpu().double(), rows) + 0.0).to(dtype)  # sums up to 2¹⁸: exact in fp32
    assert float(want.float().abs().max()) > 256  # beyond bfloat16's integers: a partial narrowed before the combine fails
    rule = cmm.bsr_wgrad_split_count(n, T)
    assert rule > 1
    got = {}
    for splits in (1, 2, 8, 0, rule):
        got[splits] = cmm.bsr_wgrad(entry_row, columns, ids, n, w, x, torch.full((n, B, B), float("nan"), device=dev, dtype=dtype), splits)
        assert_same_bits(got[splits], want, f"splits={splits}")
    assert_same_bits(got[0], got[rule], "splits = 0 is the rule's count")


# ---- 3. the same bits as the dense kernels ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("T", [40, 136])
@pytest.mark.parametrize("name,rows", [("full", FULL), ("half", HALF)])
def test_3_same_bits_as_the_dense_product(mm, cmm, dev, dtype, T, name, rows):
    fout = fin = 256
    layout = layout_from_rows(rows, 4, dev)
    values = randn((len(entries(rows)), B, B), dev, dtype, 31)
    x, w, bias = randn((T, fin), dev, dtype, 32), randn((T, fout), dev, dtype, 33), randn((fout,), dev, dtype, 34)
    W = densify(values, rows, 4)
    y, yb, dx, gw = (torch.full(s, float("nan"), device=dev, dtype=dtype) for s in ((T, fout), (T, fout), (T, fin), (fout, fin)))
    cmm.cublas_mmul(x, W, y, False, True)
    cmm.cublas_mmul_bias(x, W, bias, yb, False, True)
    cmm.cublas_mmul(w, W, dx, False, False)
    cmm.cublas_mmul(w, x, gw, True, False)
    assert_same_step(step(mm, x, values, layout, None, w), (y, dx, kept_blocks(gw, rows)), f"{name} T={T}")
    assert_same_step(step(mm, x, values, layout, bias, w)[:3], (yb, dx, kept_blocks(gw, rows)), f"{name} T={T} + bias")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("name,rows", [("full", FULL), ("half", HALF)])
def test_3_same_bits_as_the_dense_split(mm, cmm, dev, dtype, name, rows):
    T, fout, fin = 2048, 256, 256
    layout = layout_from_rows(rows, 4, dev)
    n = len(entries(rows))
    (offsets, columns, ids, entry_row, _), _ = lists_of(mm, layout, dev, len(rows), 4)
    x, w = randn((T, fin), dev, dtype, 35), randn((T, fout), dev, dtype, 36)
    for splits in (2, 8):
        gw = torch.full((fout, fin), float("nan"), device=dev, dtype=dtype)
        cmm.cublas_mmul_splitk(w, x, gw, True, False, splits=splits)
        got = cmm.bsr_wgrad(entry_row, columns, ids, n, w, x, torch.full((n, B, B), float("nan"), device=dev, dtype=dtype), splits)
        assert_same_bits(got, kept_blocks(gw, rows), f"{name} splits={splits}")


@pytest.mark.parametrize("dtype", LOWP)
def test_3_layer_against_cublas_linear(mm, cmm, dev, dtype):
    sys.modules.pop("fc_layers", None)
    import fc_layers
    rows, T = HALF, 136
    layout = layout_from_rows(rows, 4, dev)
    dense = fc_layers.cublasLinear(256, 256).to(dev).to(dtype)
    with torch.no_grad():  # zeros outside the layout
        dense.weight.copy_(densify(kept_blocks(dense.weight.detach(), rows), rows, 4))
    layer = fc_layers.blockSparseLinear.from_dense(dense.weight.detach(), layout, dense.bias.detach())
    assert layer.values.dtype == dtype and layer.values.device.type == "cuda"
    assert_same_bits(layer.dense_weight().detach(), dense.weight.detach(), "from_dense / dense_weight")
    x, w = randn((2, T // 2, 256), dev, dtype, 37), randn((2, T // 2, 256), dev, dtype, 38)
    got, want = [], []
    for m, res in ((layer, got), (dense, want)):
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        y.backward(w)
        res.extend([y.detach(), xi.grad, m.bias.grad])
    for name, g, e in zip(("y", "d x", "d bias"), got, want):
        assert_same_bits(g, e, f"layer: {name}")
    assert_same_bits(layer.values.grad, kept_blocks(dense.weight.grad, rows), "layer: d values")  # (136 tokens: no split either side)
    # a fresh layer with the full layout starts with cublasLinear's parameters
    fresh, ref = fc_layers.blockSparseLinear(256, 256, layout_from_rows(FULL, 4, "cpu")), fc_layers.cublasLinear(256, 256)
    assert torch.equal(fresh.dense_weight().detach(), ref.weight.detach()) and torch.equal(fresh.bias.detach(), ref.bias.detach())


# ---- 4. a long list -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("kept", [1, 2, 3, 40])
def test_4_long_list_within_the_bound(mm, dev, dtype, kept):
    """k terms per element: 64 per kept block and the bias for y, the 64 rows of the one block row for d x, the tokens for
    d values and d bias (column_sums: fp32 sums, one rounding)."""
    cols, T = 40, 72
    rows = [list(range(0, cols, cols // kept))[:kept]] if kept < cols else [list(range(cols))]
    layout = layout_from_rows(rows, cols, dev)
    values = randn((kept, B, B), dev, dtype, 41)
    x, w, bias = randn((T, cols * B), dev, dtype, 42), randn((T, B), dev, dtype, 43), randn((B,), dev, dtype, 44)
    got = step(mm, x, values, layout, bias, w)
    E = f64_step(x, values, rows, cols, bias, w)
    S = f64_step(x.abs(), values.abs(), rows, cols, bias.abs(), w.abs())
    for name, g, e, s, k in zip(NAMES, got, E, S, (B * kept + 1, B, T, T)):
        assert g.dtype == dtype and g.shape == e.shape, name
        tol = U[dtype] * e.abs() + k * 2.0 ** -23 * s + ABS[dtype]
        err = (g.cpu().double() - e).abs()
        print(f"{name} kept={kept} {dtype}: max err / tol = {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        bad = ~(err <= tol)
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} values outside the bound"


# ---- 5. invariance --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("T", [33, 136])
def test_5_leading_dimensions_and_repeats(mm, dev, dtype, T):
    rows, cols = RECT_UNSORTED, 5
    fout, fin = len(rows) * B, cols * B
    layout = layout_from_rows(rows, cols, dev)
    values = randn((len(entries(rows)), B, B), dev, dtype, 51)
    bias = randn((fout,), dev, dtype, 54)
    x, w = randn((2, 3, T, fin), dev, dtype, 52), randn((2, 3, T, fout), dev, dtype, 53)
    y, dx, dvalues, dbias = step(mm, x, values, layout, bias, w)
    assert y.shape == (2, 3, T, fout) and dx.shape == x.shape and dvalues.shape == values.shape and dbias.shape == bias.shape
    flat = step(mm, x.reshape(-1, fin), values, layout, bias, w.reshape(-1, fout))
    for i in range(2):
        for j in range(3):
            item = slice((i * 3 + j) * T, (i * 3 + j + 1) * T)
            assert_same_bits(y[i, j], flat[0][item], f"y of item {i, j}")
            assert_same_bits(dx[i, j], flat[1][item], f"d x of item {i, j}")
            # the position of a token: the item alone gives the same rows
            y1, dx1 = step(mm, x[i, j], values, layout, bias, w[i, j])[:2]
            assert_same_bits(y[i, j], y1, f"y of item {i, j} alone")
            assert_same_bits(dx[i, j], dx1, f"d x of item {i, j} alone")
    assert_same_bits(dvalues, flat[2], "d values against the flattened call")
    assert_same_step(step(mm, x, values, layout, bias, w), (y, dx, dvalues, dbias), "a second run")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("T", [33, 136])
def test_5_checked_form_and_layout_order(mm, dev, dtype, T):
    rows, cols = RECT_UNSORTED, 5
    fout, fin = len(rows) * B, cols * B
    layout = layout_from_rows(rows, cols, dev)
    values = randn((len(entries(rows)), B, B), dev, dtype, 55)
    bias = randn((fout,), dev, dtype, 58)
    x_big, w_big = randn((T, fin + 1), dev, dtype, 56), randn((T, fout + 1), dev, dtype, 57)
    x_view, w_view = x_big[:, 1:], w_big[:, 1:]  # 2-byte aligned rows, an odd leading dimension: the checked form
    assert x_view.data_ptr() % 16 != 0 and not x_view.is_contiguous() and x_view.stride(0) % 2 == 1
    want = step(mm, x_view.contiguous(), values, layout, bias, w_view.contiguous())
    assert_same_step(step(mm, x_view, values, layout, bias, w_view), want, "column-offset views")
    # the sorted twin of the layout, the values permuted to match
    order = sorted(range(len(entries(rows))), key=lambda e: entries(rows)[e])
    twin = layout_from_rows([sorted(c) for c in rows], cols, dev)
    got = step(mm, x_view.contiguous(), values[order].contiguous(), twin, bias, w_view.contiguous())
    assert_same_bits(got[0], want[0], "sorted twin: y")
    assert_same_bits(got[1], want[1], "sorted twin: d x")
    assert_same_bits(got[2], want[2][order], "sorted twin: d values")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("T", [33, 136])
def test_5_checked_stores_into_a_column_offset_view(mm, cmm, dev, dtype, T):
    """The element-wise stores of the checked form: y and d x written straight into column-offset views of wider buffers
    (2-byte aligned rows, an odd leading dimension) carry the bits of the contiguous call, and the column beside the view
    is not touched."""
    rows, cols = RECT_UNSORTED, 5
    fout, fin = len(rows) * B, cols * B
    layout = layout_from_rows(rows, cols, dev)
    n = len(entries(rows))
    values, bias = randn((n, B, B), dev, dtype, 55), randn((fout,), dev, dtype, 58)
    x, w = randn((T, fin), dev, dtype, 56), randn((T, fout), dev, dtype, 57)
    (offsets, columns, ids, _, _), (t_off, t_col, t_ids) = lists_of(mm, layout, dev, len(rows), cols)
    want = step(mm, x, values, layout, bias, w)
    y_big = torch.full((T, fout + 1), 7.0, device=dev, dtype=dtype)
    dx_big = torch.full((T, fin + 1), 7.0, device=dev, dtype=dtype)
    y_view, dx_view = y_big[:, 1:], dx_big[:, 1:]
    assert y_view.data_ptr() % 16 != 0 and y_view.stride(0) % 2 == 1 and dx_view.stride(0) % 2 == 1
    cmm.bsr_linear(offsets, columns, ids, n, values, x, bias, y_view, False)
    cmm.bsr_linear(t_off, t_col, t_ids, n, values, w, None, dx_view, True)
    assert_same_bits(y_view, want[0], "y into a column-offset view")
    assert_same_bits(dx_view, want[1], "d x into a column-offset view")
    assert bool((y_big[:, 0] == 7).all()) and bool((dx_big[:, 0] == 7).all()), "the column beside the view"


# ---- 6. unkept blocks are never read -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_6_unkept_blocks_are_never_read(mm, dev, dtype):
    rows, cols, T = BAND_GLOBAL, 4, 40
    layout = layout_from_rows(rows, cols, dev)
    n = len(entries(rows))
    buffer = randn((n + 2, B, B), dev, dtype, 61)
    buffer[n:] = float("nan")  # an unused tail of a larger buffer
    values = buffer[:n]
    x, w = randn((T, cols * B), dev, dtype, 62), randn((T, len(rows) * B), dev, dtype, 63)
    clean = step(mm, x, values, layout, None, w)
    assert all(bool(torch.isfinite(v.float()).all()) for v in clean)
    # block column 3 is kept by nobody: NaN in those columns of x reaches nothing
    x3 = x.clone()
    x3[:, 3 * B:] = float("nan")
    got = step(mm, x3, values, layout, None, w)
    assert_same_bits(got[0], clean[0], "NaN under the never-kept block column: y")
    assert_same_bits(got[2], clean[2], "NaN under the never-kept block column: d values")
    # block column 1 is kept by block row 1 alone: exactly that block row's 64 output columns
    x1 = x.clone()
    x1[:, B:2 * B] = float("nan")
    y = step(mm, x1, values, layout, None, w)[0]
    assert bool(torch.isnan(y[:, B:2 * B].float()).all()), "the block row that lists the column"
    for r in (0, 2, 3):
        assert_same_bits(y[:, r * B:(r + 1) * B], clean[0][:, r * B:(r + 1) * B], f"block row {r} does not list the column")
    # the columns of dY of the empty block row 2 meet no kept block
    w2 = w.clone()
    w2[:, 2 * B:3 * B] = float("nan")
    got = step(mm, x, values, layout, None, w2)
    assert_same_bits(got[1], clean[1], "NaN in dY of the empty block row: d x")
    assert_same_bits(got[2], clean[2], "NaN in dY of the empty block row: d values")


# ---- 7. graph capture ----------------------------------------------------------------------------------------------

def test_7_graph_capture_replays_the_eager_bits(mm, cmm, dev):
    rows, cols, T, dtype = HALF, 4, 2048, torch.bfloat16
    layout = layout_from_rows(rows, cols, dev)
    n = len(entries(rows))
    assert cmm.bsr_wgrad_split_count(n, T) > 1  # the split, with its workspace, is inside the capture
    values = randn((n, B, B), dev, dtype, 71).requires_grad_(True)
    bias = randn((len(rows) * B,), dev, dtype, 74).requires_grad_(True)
    x = randn((T, cols * B), dev, dtype, 72).requires_grad_(True)
    w = randn((T, len(rows) * B), dev, dtype, 73)

    def run():
        y = mm.block_sparse_linear(x, values, layout, bias)
        return (y,) + torch.autograd.grad(y, (x, values, bias), grad_outputs=w)

    eager = [v.detach().clone() for v in run()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for o in outs:
        o.detach().fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for name, o, e in zip(NAMES, outs, eager):
        assert_same_bits(o.detach(), e, f"graph replay: {name}")


# ---- 8. memory -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [256, 4096])
def test_8_no_dense_weight_and_no_transposed_activations(mm, cmm, built, dev, T):
    nb, keep, dtype = 32, 4, torch.bfloat16  # out = in = 2048: out × in in T is 8 MiB
    g = torch.Generator().manual_seed(81)
    rows = [torch.randperm(nb, generator=g)[:keep].tolist() for _ in range(nb)]
    layout = layout_from_rows(rows, nb, dev)
    n = nb * keep
    values = randn((n, B, B), dev, dtype, 82).requires_grad_(True)   # 1 MiB
    bias = randn((nb * B,), dev, dtype, 85).requires_grad_(True)
    x = randn((T, nb * B), dev, dtype, 83).requires_grad_(True)
    w = randn((T, nb * B), dev, dtype, 84)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    lib.mi_bsr_wgrad_workspace_bytes.restype = ctypes.c_size_t
    lib.mi_bsr_wgrad_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32]
    workspace = lib.mi_bsr_wgrad_workspace_bytes(n, cmm.bsr_wgrad_split_count(n, T))
    assert (workspace > 0) == (T == 4096)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = mm.block_sparse_linear(x, values, layout, bias)  # the first call on this layout: the index arrays are built here
    grads = torch.autograd.grad(y, (x, values, bias), grad_outputs=w)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = sum(v.numel() * v.element_size() for v in (y,) + grads)
    print(f"T={T}: peak {peak} bytes over the inputs, results {results} bytes, split workspace {workspace} bytes")
    # beyond the results: the O(n) index arrays and their sort, what the one-off device transpose's fixed workspace exceeds
    # the gradients by, and the split's fp32 partials — never an [in, T] or [out, T] copy of the activations (T·2048·2 bytes)
    assert results <= peak <= results + workspace + (1 << 20), (peak, results, workspace)
    if T == 256:
        assert peak < (nb * B) ** 2 * 2
    assert T * nb * B * 2 >= (1 << 20)  # a transposed copy would not fit the allowance
