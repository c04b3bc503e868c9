"""matmuls.block_sparse_mm on the MI355X: C = A·b with A in 64 × 64 blocks, d values and d b.

The contract (include/mi_spmm.h, mi_bsr_mm / mi_bsr_sddmm — DESIGN.md §3.15): every product on the MFMA with fp32
accumulators, ONE accumulator per output element from +0 through the kept blocks in ascending order, one rounding at the
store — the instruction and the order of this package's dense low-precision product, with the unkept blocks left out.
  1. exact: integer operands in [−8, 8] keep every fp32 partial sum exact, so out, d b and d values are the float64 results
     narrowed to T, bit for bit; an empty block row and a never-kept block column give exact zeros;
  2. the same bits as cublas_mmul (plain, transa, transb) on the densified A, randn operands;
  3. a long list (1, 2, 3, 40 kept blocks in one block row) within |C − E| ≤ u_T·|E| + k·2⁻²³·(|A|·|B|) (+ 2⁻²⁵ for fp16);
  4. invariance: batch position, the item-major flattening of d values, the checked alignment form, the order of the
     layout, repeated runs;
  5. unkept blocks are never read; 6. graph capture; 7. memory;
  8. 65 538 items, exact as in 1: the second pass of bsr_mm's item loop behind the 65 535-item grid cap.
Every shape here stays below 512 wide tiles and so takes the 64-column tile (custom_mm.bsr_mm_tile_n is the rule);
  9. the 128-column tile — 1, 2, 4 (items, the checked form) and 5 there: tests/test_gpu_lowp_wide_tiles.py;
 10. malformed lists — a column outside the grid, an id outside the values, offsets outside [0, nnz]:
     tests/test_gpu_block_lists_malformed.py.
"""
import pytest
import torch

from gpu_helpers import assert_same_bits

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ABS = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
NAMES = ("out", "d values", "d b")
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
    """A [M, K] in the dtype and on the device of values: block (I, J) of stored entry e is values[e], zeros elsewhere."""
    a = torch.zeros(len(rows_cols) * B, cols * B, dtype=values.dtype, device=values.device)
    for e, (i, j) in enumerate(entries(rows_cols)):
        a[i * B:(i + 1) * B, j * B:(j + 1) * B] = values[e]
    return a


def kept_blocks(full, rows_cols):
    """[n, 64, 64]: the blocks of a dense [M, K] at the stored entries."""
    return torch.stack([full[i * B:(i + 1) * B, j * B:(j + 1) * B] for i, j in entries(rows_cols)])


def ints(shape, dev, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype).to(dev)


def randn(shape, dev, dtype, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def step(mm, values, layout, b, w):
    """(out, d values, d b) of one forward + backward on fresh leaves."""
    values, b = values.detach().requires_grad_(True), b.detach().requires_grad_(True)
    out = mm.block_sparse_mm(values, layout, b)
    return (out.detach(),) + torch.autograd.grad(out, (values, b), grad_outputs=w)


def assert_same_step(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_same_bits(g, w, f"{what}: {name}")


def f64_step(values, rows_cols, cols, b, w):
    """(out, d values, d b) in float64 on the CPU, 2-d b."""
    a = densify(values.cpu().double(), rows_cols, cols)
    b64, w64 = b.cpu().double(), w.cpu().double()
    # (+ 0.0: every sum starts at +0 by contract, so a sum of −0 products is +0 — torch's own products may leave −0)
    return a @ b64 + 0.0, kept_blocks(w64 @ b64.T, rows_cols) + 0.0, a.T @ w64 + 0.0


# ---- 1. exact -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("name,rows,cols,index_dtype", [
    ("full", FULL, 4, torch.int64), ("diagonal", DIAGONAL, 4, torch.int64), ("band+global", BAND_GLOBAL, 4, torch.int64),
    ("rect-unsorted", RECT_UNSORTED, 5, torch.int32)])
def test_1_integer_operands_are_exact(mm, cmm, dev, dtype, name, rows, cols, index_dtype):
    layout = layout_from_rows(rows, cols, dev, index_dtype)
    n, M, K = len(entries(rows)), len(rows) * B, cols * B
    values = ints((n, B, B), dev, dtype, 1)
    rec = mm._bsr_layout(layout, dev, mm._csr_state(layout))
    offsets, columns, ids, entry_row, _ = rec["fwd"]
    t_off, t_col, t_ids = mm._bsr_layout_transposed(rec, len(rows), cols)
    for N in (1, 8, 40, 64, 136, 200):
        b, w = ints((K, N), dev, dtype, 2 + N), ints((M, N), dev, dtype, 3 + N)
        want = tuple(x.to(dtype) for x in f64_step(values, rows, cols, b, w))
        got = step(mm, values, layout, b, w)
        assert_same_step(got, want, f"{name} N={N}")
        # the entries themselves, into outputs pre-filled with NaN: every element is written
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=dtype)  # noqa: E731
        out, dvalues, db = nan(1, M, N), nan(n, B, B), nan(1, K, N)
        cmm.bsr_mm(offsets, columns, ids, n, values, b[None], out, False)
        cmm.bsr_sddmm(entry_row, columns, ids, n, w[None], b[None], dvalues)
        cmm.bsr_mm(t_off, t_col, t_ids, n, values, w[None], db, True)
        assert_same_step((out[0], dvalues, db[0]), want, f"{name} N={N}, pre-filled")
        if name == "band+global":
            zero = torch.zeros(B, N, dtype=dtype)
            assert_same_bits(got[0][2 * B:3 * B], zero, "the empty block row of out")  # +0, not −0
            assert_same_bits(got[2][3 * B:4 * B], zero, "the never-kept block column in d b")


# ---- 2. the same bits as the dense product ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [40, 136])
@pytest.mark.parametrize("name,rows", [("full", FULL), ("half", HALF)])
def test_2_same_bits_as_the_dense_product(mm, cmm, dev, dtype, N, name, rows):
    M = K = 256
    layout = layout_from_rows(rows, 4, dev)
    values = randn((len(entries(rows)), B, B), dev, dtype, 11)
    b, w = randn((K, N), dev, dtype, 12), randn((M, N), dev, dtype, 13)
    a = densify(values, rows, 4)
    out, da, db = (torch.full(s, float("nan"), device=dev, dtype=dtype) for s in ((M, N), (M, K), (K, N)))
    cmm.cublas_mmul(a, b, out, False, False)
    cmm.cublas_mmul(w, b, da, False, True)
    cmm.cublas_mmul(a, w, db, True, False)
    assert_same_step(step(mm, values, layout, b, w), (out, kept_blocks(da, rows), db), f"{name} N={N}")


# ---- 3. a long list -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("kept", [1, 2, 3, 40])
def test_3_long_list_within_the_bound(mm, dev, dtype, kept):
    cols, N = 40, 72
    rows = [list(range(0, cols, cols // kept))[:kept]] if kept < cols else [list(range(cols))]
    layout = layout_from_rows(rows, cols, dev)
    values = randn((kept, B, B), dev, dtype, 21)
    b, w = randn((cols * B, N), dev, dtype, 22), randn((B, N), dev, dtype, 23)
    got = step(mm, values, layout, b, w)
    E = f64_step(values, rows, cols, b, w)
    S = f64_step(values.abs(), rows, cols, b.abs(), w.abs())
    for name, g, e, s, k in zip(NAMES, got, E, S, (B * kept, N, B)):
        assert g.dtype == dtype and g.shape == e.shape, name
        tol = U[dtype] * e.abs() + k * 2.0 ** -23 * s + ABS[dtype]
        err = (g.cpu().double() - e).abs()
        print(f"{name} kept={kept} {dtype}: max err / tol = {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        bad = ~(err <= tol)
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} values outside the bound"


# ---- 4. invariance --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [40, 33])
def test_4_batch_items_and_the_flattening(mm, dev, dtype, N):
    rows, cols = RECT_UNSORTED, 5
    M, K = len(rows) * B, cols * B
    layout = layout_from_rows(rows, cols, dev)
    values = randn((len(entries(rows)), B, B), dev, dtype, 31)
    b, w = randn((2, 3, K, N), dev, dtype, 32), randn((2, 3, M, N), dev, dtype, 33)
    out, dvalues, db = step(mm, values, layout, b, w)
    assert out.shape == (2, 3, M, N) and db.shape == b.shape and dvalues.shape == values.shape
    for i in range(2):
        for j in range(3):
            o1, _, db1 = step(mm, values, layout, b[i, j], w[i, j])
            assert_same_bits(out[i, j], o1, f"out of item {i, j}")
            assert_same_bits(db[i, j], db1, f"d b of item {i, j}")
    # d values: the single call on the operands flattened item-major to [·, batch · N]
    flat = lambda x: x.reshape(6, -1, N).permute(1, 0, 2).reshape(-1, 6 * N).contiguous()  # noqa: E731
    _, dv1, _ = step(mm, values, layout, flat(b), flat(w))
    assert_same_bits(dvalues, dv1, "d values of the batch against the flattened call")
    assert_same_step(step(mm, values, layout, b, w), (out, dvalues, db), "a second run")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [40, 136])
def test_4_checked_form_and_layout_order(mm, dev, dtype, N):
    rows, cols = RECT_UNSORTED, 5
    M, K = len(rows) * B, cols * B
    layout = layout_from_rows(rows, cols, dev)
    values = randn((len(entries(rows)), B, B), dev, dtype, 41)
    b_big, w_big = randn((2, K, N + 1), dev, dtype, 42), randn((2, M, N + 1), dev, dtype, 43)
    b_view, w_view = b_big[..., 1:], w_big[..., 1:]  # 2-byte aligned rows, an odd leading dimension: the checked form
    assert b_view.data_ptr() % 16 != 0 and not b_view.is_contiguous()
    want = step(mm, values, layout, b_view.contiguous(), w_view.contiguous())
    assert_same_step(step(mm, values, layout, b_view, w_view), want, "column-offset views")
    # the sorted twin of the layout, the values permuted to match
    order = sorted(range(len(entries(rows))), key=lambda e: entries(rows)[e])
    twin = layout_from_rows([sorted(c) for c in rows], cols, dev)
    got = step(mm, values[order].contiguous(), twin, b_view.contiguous(), w_view.contiguous())
    assert_same_bits(got[0], want[0], "sorted twin: out")
    assert_same_bits(got[1], want[1][order], "sorted twin: d values")
    assert_same_bits(got[2], want[2], "sorted twin: d b")


# ---- 5. unkept blocks are never read -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_5_unkept_blocks_are_never_read(mm, dev, dtype):
    rows, cols, N = BAND_GLOBAL, 4, 40
    layout = layout_from_rows(rows, cols, dev)
    n = len(entries(rows))
    buffer = randn((n + 2, B, B), dev, dtype, 51)
    buffer[n:] = float("nan")  # an unused tail of a larger buffer
    values = buffer[:n]
    b, w = randn((cols * B, N), dev, dtype, 52), randn((len(rows) * B, N), dev, dtype, 53)
    clean = step(mm, values, layout, b, w)
    assert all(bool(torch.isfinite(x.float()).all()) for x in clean)
    # block column 3 is kept by nobody: NaN there reaches nothing
    b3 = b.clone()
    b3[3 * B:] = float("nan")
    got = step(mm, values, layout, b3, w)
    assert_same_bits(got[0], clean[0], "NaN under a never-kept block column: out")
    assert_same_bits(got[1], clean[1], "NaN under a never-kept block column: d values")
    # block column 1 is kept by block row 1 alone
    b1 = b.clone()
    b1[B:2 * B] = float("nan")
    out = step(mm, values, layout, b1, w)[0]
    assert bool(torch.isnan(out[B:2 * B].float()).all()), "the block row that lists the column"
    for r in (0, 2, 3):
        assert_same_bits(out[r * B:(r + 1) * B], clean[0][r * B:(r + 1) * B], f"block row {r} does not list the column")
    # likewise d b = Aᵀ·dC: NaN in the rows of dC of block row 1 reaches the block columns 0 and 1 it keeps, no other
    w1 = w.clone()
    w1[B:2 * B] = float("nan")
    db = step(mm, values, layout, b, w1)[2]
    assert bool(torch.isnan(db[:2 * B].float()).all())
    assert_same_bits(db[2 * B:], clean[2][2 * B:], "block columns block row 1 does not keep")


# ---- 6. graph capture ----------------------------------------------------------------------------------------------

def test_6_graph_capture_replays_the_eager_bits(mm, dev):
    rows, cols, N = HALF, 4, 136
    layout = layout_from_rows(rows, cols, dev)
    values = randn((len(entries(rows)), B, B), dev, torch.bfloat16, 61)
    b = randn((3, cols * B, N), dev, torch.bfloat16, 62)
    eager = mm.block_sparse_mm(values, layout, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mm.block_sparse_mm(values, layout, b)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mm.block_sparse_mm(values, layout, b)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(out, eager, "graph replay")


# ---- 7. memory -----------------------------------------------------------------------------------------------------

def test_7_nothing_of_size_m_by_k_is_allocated(mm, dev):
    nb, keep, N, dtype = 32, 4, 256, torch.bfloat16  # M = K = 2048: M × K in T is 8 MiB
    g = torch.Generator().manual_seed(71)
    rows = [torch.randperm(nb, generator=g)[:keep].tolist() for _ in range(nb)]
    layout = layout_from_rows(rows, nb, dev)
    values = randn((nb * keep, B, B), dev, dtype, 72).requires_grad_(True)   # 1 MiB
    b = randn((nb * B, N), dev, dtype, 73).requires_grad_(True)              # 1 MiB
    w = randn((nb * B, N), dev, dtype, 74)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = mm.block_sparse_mm(values, layout, b)  # the first call on this layout: the index arrays are built here
    dvalues, db = torch.autograd.grad(out, (values, b), grad_outputs=w)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    results = sum(x.numel() * x.element_size() for x in (out, dvalues, db))  # 3 MiB
    print(f"peak {peak} bytes over the inputs, results {results} bytes")
    # beyond the results: the O(n) index arrays and their sort (n = 128: KiB), and whatever the one-off device transpose's
    # fixed 2 MiB workspace, alive beside `out` alone, exceeds the two gradients by — far below 1 MiB
    assert results <= peak <= results + (1 << 20), (peak, results)
    assert peak < (nb * B) ** 2 * 2


# ---- 8. beyond 65 535 items -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LOWP)
def test_8_beyond_65535_items_is_exact(mm, dev, dtype):
    """65 538 items of b [128, 8]: bsr_mm's grid holds 65 535 of them, the rest come in the second pass of its item loop
    (forward and d b); d values sums over every item.  Operands in {−1, 0, 1}: the 524 304-term sums of d values stay exact
    in fp32, so contract 1 holds — the float64 results (on the device: 0.54 GB per operand) narrowed to T, bit for bit."""
    rows, cols, items, N = [[1], [0, 1]], 2, 65538, 8
    layout = layout_from_rows(rows, cols, dev)
    g = torch.Generator(device=dev).manual_seed(81)
    draw = lambda *shape: torch.randint(-1, 2, shape, device=dev, generator=g).to(dtype)  # noqa: E731
    values, b, w = draw(len(entries(rows)), B, B), draw(items, cols * B, N), draw(items, len(rows) * B, N)
    got = step(mm, values, layout, b, w)
    a = densify(values.double(), rows, cols)
    b64, w64 = b.double(), w.double()
    by_rows = lambda x: x.permute(1, 0, 2).reshape(x.shape[1], -1)  # noqa: E731  [rows, items · N]
    by_items = lambda x: x.reshape(x.shape[0], items, N).permute(1, 0, 2).contiguous()  # noqa: E731  and back
    b64, w64 = by_rows(b64), by_rows(w64)
    want = (by_items(a @ b64) + 0.0, kept_blocks(w64 @ b64.T, rows) + 0.0, by_items(a.T @ w64) + 0.0)
    for name, r, x in zip(NAMES, got, want):
        assert r.shape == x.shape, name
        assert torch.equal(r.view(torch.int16), x.to(dtype).view(torch.int16)), f"{dtype} {name} of {items} items"
    assert got[1].abs().max() > 256  # sums long enough for the store's rounding to matter
