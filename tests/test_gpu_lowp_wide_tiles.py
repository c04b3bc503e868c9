"""The 128-wide tiles of the three matrix-core products on the MI355X: block_sparse_mm (bsr_mm_kernel at BN = 128),
block_sparse_linear (bsr_linear_kernel at BM = 128) and the dense low-precision product (gemm_lowp_kernel at 128 × 128).

The contracts (include/mi_spmm.h) promise that the bits of an output element never depend on
the tile the launcher picks.  The launchers pick by the shape alone, through rules a test can ask: custom_mm.bsr_mm_tile_n,
bsr_linear_tile_tokens and gemm_lowp_tile_n.  Every test here first asserts that its full shape takes 128 and that each
narrow twin it compares against takes 64 — a retuned threshold fails these tests instead of blinding them.
  * exact: integer operands in [−8, 8] keep every fp32 partial sum exact, so every result is the float64 result (CPU, computed
    once per unit and shared by both dtypes) narrowed to T, bit for bit — in the 16-byte form and in the checked form;
  * tile invariance: randn operands, an item / a slice of tokens run alone at the 64 tile gives the bits of the big call,
    and the block-sparse products give the bits of the dense product on the densified operand;
  * a NaN under a never-kept block column changes nothing at the wide tile.
All comparisons are bit for bit.  The layout is 5 × 7 blocks with an empty block row, an unsorted row, a never-kept block
column and a row of four blocks; its transposed list has 7 rows, so neither grid is a multiple of 8 workgroups.
"""
import ctypes
import functools

import pytest
import torch

from gpu_helpers import SENTINEL, Padded, assert_same_bits

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
B = 64
NAN = float("nan")

WIDE = [[0, 3], [6, 1, 4], [], [0, 2, 3, 6], [1]]  # block row 2 empty, row 1 unsorted, block column 5 never kept, row 3 keeps 4
ROWS, COLS = len(WIDE), 7
EMPTY_ROW, UNKEPT_COL = 2, 5
INDEX = {torch.bfloat16: torch.int64, torch.float16: torch.int32}  # both index dtypes, one per value dtype


def layout_from_rows(rows_cols, cols, dev, index_dtype=torch.int64):
    """A 2-d CSR block layout (values 1) from per-block-row column lists, kept in the order given (unsorted allowed)."""
    crow = [0]
    for c in rows_cols:
        crow.append(crow[-1] + len(c))
    col = [j for c in rows_cols for j in c]
    return torch.sparse_csr_tensor(torch.tensor(crow, dtype=index_dtype, device=dev), torch.tensor(col, dtype=index_dtype, device=dev),
                                   torch.ones(len(col), device=dev), size=(len(rows_cols), cols))


ENTRIES = [(i, j) for i, c in enumerate(WIDE) for j in c]
NNZ = len(ENTRIES)


def densify(values):
    """[320, 448] in the dtype and on the device of values: block (I, J) of stored entry e is values[e], zeros elsewhere."""
    a = torch.zeros(ROWS * B, COLS * B, dtype=values.dtype, device=values.device)
    for e, (i, j) in enumerate(ENTRIES):
        a[i * B:(i + 1) * B, j * B:(j + 1) * B] = values[e]
    return a


def kept_blocks(full):
    """[n, 64, 64]: the blocks of a dense [320, 448] at the stored entries."""
    return torch.stack([full[i * B:(i + 1) * B, j * B:(j + 1) * B] for i, j in ENTRIES])


def ints(shape, seed):
    """Integers in [−8, 8] as float64 on the CPU: exact in bfloat16 and in float16."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).double()


def randn(shape, dev, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(dev)


def nan_like(*shape, dev, dtype):
    return torch.full(shape, NAN, device=dev, dtype=dtype)


def offset_view(x):
    """x as a column-offset view of a NaN buffer one column wider: rows on 2-byte boundaries, a leading dimension that is no
    multiple of 8 at the widths used here (198, 321, 449) — the checked form."""
    big = torch.full(x.shape[:-1] + (x.shape[-1] + 1,), NAN, device=x.device, dtype=x.dtype)
    big[..., 1:] = x
    view = big[..., 1:]
    assert view.data_ptr() % 16 != 0 and not view.is_contiguous()
    return view


def lists_of(mm, layout, dev):
    rec = mm._bsr_layout(layout, dev, mm._csr_state(layout))
    return rec["fwd"], mm._bsr_layout_transposed(rec, ROWS, COLS)


# ---- block_sparse_mm: bsr_mm_kernel<·, ·, 128, ·> ----------------------------------------------------------------------

ITEMS, M, K = 52, ROWS * B, COLS * B
MM_NAMES = ("out", "d values", "d b")


def mm_step(mm, values, layout, b, w):
    """(out, d values, d b) of one forward + backward on fresh leaves."""
    values, b = values.detach().requires_grad_(True), b.detach().requires_grad_(True)
    out = mm.block_sparse_mm(values, layout, b)
    return (out.detach(),) + torch.autograd.grad(out, (values, b), grad_outputs=w)


def assert_mm_tiles(cmm, N, items, tile):
    assert cmm.bsr_mm_tile_n(M, N, items) == tile, f"out: {M // B} blocks x N={N} x {items} items"
    assert cmm.bsr_mm_tile_n(K, N, items) == tile, f"d b: {K // B} blocks x N={N} x {items} items"


@functools.lru_cache(maxsize=None)
def mm_exact_case(N):
    """Integer operands of the 52-item product and its float64 results on the CPU; the longest sum, of d values, has
    52·N terms of at most 64 each: below 2²⁴, exact in fp32."""
    values, b, w = ints((NNZ, B, B), 1), ints((ITEMS, K, N), 2 + N), ints((ITEMS, M, N), 3 + N)
    a = densify(values)
    flat = lambda x: x.permute(1, 0, 2).reshape(x.shape[1], -1)  # noqa: E731  [rows, items · N], item-major
    # (+ 0.0: every sum starts at +0 by contract, so a sum of −0 products is +0 — torch's own products may leave −0)
    want = (a @ b + 0.0, kept_blocks(flat(w) @ flat(b).T) + 0.0, a.T @ w + 0.0)
    assert float(want[1].abs().max()) < 2 ** 24
    return values, b, w, want


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [200, 197])
def test_block_mm_wide_tile_is_exact(mm, cmm, dev, dtype, N):
    """N = 200: the 16-byte form; N = 197 through column-offset views: the checked form, 2-byte aligned.  Two column tiles,
    the second ragged (72 / 69 columns)."""
    assert_mm_tiles(cmm, N, ITEMS, 128)
    values, b, w, want = mm_exact_case(N)
    want = tuple(x.to(dtype) for x in want)
    values, b, w = (x.to(dtype).to(dev) for x in (values, b, w))
    if N % 8:
        b, w = offset_view(b), offset_view(w)
    layout = layout_from_rows(WIDE, COLS, dev, INDEX[dtype])
    got = mm_step(mm, values, layout, b, w)
    for name, g, e in zip(MM_NAMES, got, want):
        assert_same_bits(g, e, f"N={N}: {name}")
    zero = torch.zeros(ITEMS, B, N, dtype=dtype)  # +0, not −0
    assert_same_bits(got[0][:, EMPTY_ROW * B:(EMPTY_ROW + 1) * B], zero, "the empty block row of out")
    assert_same_bits(got[2][:, UNKEPT_COL * B:(UNKEPT_COL + 1) * B], zero, "the never-kept block column in d b")
    # the entries themselves, into outputs pre-filled with NaN: every element is written
    (offsets, columns, ids, entry_row, n), (t_off, t_col, t_ids) = lists_of(mm, layout, dev)
    out, dvalues, db = nan_like(ITEMS, M, N, dev=dev, dtype=dtype), nan_like(n, B, B, dev=dev, dtype=dtype), nan_like(ITEMS, K, N, dev=dev, dtype=dtype)
    cmm.bsr_mm(offsets, columns, ids, n, values, b, out, False)
    cmm.bsr_sddmm(entry_row, columns, ids, n, w, b, dvalues)
    cmm.bsr_mm(t_off, t_col, t_ids, n, values, w, db, True)
    for name, g, e in zip(MM_NAMES, (out, dvalues, db), want):
        assert_same_bits(g, e, f"N={N}, pre-filled: {name}")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [200, 197])
def test_block_mm_wide_tile_has_the_bits_of_the_narrow_tile_and_of_the_dense_product(mm, cmm, dev, dtype, N):
    assert_mm_tiles(cmm, N, ITEMS, 128)
    assert_mm_tiles(cmm, N, 1, 64)
    assert cmm.gemm_lowp_tile_n(M, N, 1) == 64 and cmm.gemm_lowp_tile_n(K, N, 1) == 64
    layout = layout_from_rows(WIDE, COLS, dev, INDEX[dtype])
    values = randn((NNZ, B, B), dev, dtype, 11)
    b, w = randn((ITEMS, K, N), dev, dtype, 12), randn((ITEMS, M, N), dev, dtype, 13)
    if N % 8:
        b, w = offset_view(b), offset_view(w)
    out, _, db = mm_step(mm, values, layout, b, w)
    a = densify(values)
    for i in (0, 17, 51):
        o1, _, db1 = mm_step(mm, values, layout, b[i], w[i])  # one item: 10 / 14 workgroups, the 64 tile
        assert_same_bits(out[i], o1, f"out of item {i} alone")
        assert_same_bits(db[i], db1, f"d b of item {i} alone")
        dense_out, dense_db = nan_like(M, N, dev=dev, dtype=dtype), nan_like(K, N, dev=dev, dtype=dtype)
        cmm.cublas_mmul(a, b[i], dense_out, False, False)
        cmm.cublas_mmul(a, w[i], dense_db, True, False)
        assert_same_bits(out[i], dense_out, f"out of item {i} against the dense product")
        assert_same_bits(db[i], dense_db, f"d b of item {i} against the dense product")


@pytest.mark.parametrize("dtype", LOWP)
def test_block_mm_wide_tile_never_reads_an_unkept_block_column(mm, cmm, dev, dtype):
    N = 200
    assert_mm_tiles(cmm, N, ITEMS, 128)
    layout = layout_from_rows(WIDE, COLS, dev, INDEX[dtype])
    values = randn((NNZ, B, B), dev, dtype, 21)
    b, w = randn((ITEMS, K, N), dev, dtype, 22), randn((ITEMS, M, N), dev, dtype, 23)
    clean = mm_step(mm, values, layout, b, w)
    assert all(bool(torch.isfinite(x.float()).all()) for x in clean)
    poisoned = b.clone()
    poisoned[:, UNKEPT_COL * B:(UNKEPT_COL + 1) * B] = NAN
    got = mm_step(mm, values, layout, poisoned, w)
    assert_same_bits(got[0], clean[0], "NaN under the never-kept block column: out")
    assert_same_bits(got[1], clean[1], "NaN under the never-kept block column: d values")


# ---- block_sparse_linear: bsr_linear_kernel<·, ·, 128, ·, ·> -----------------------------------------------------------

TOKENS, FOUT, FIN = 13147, ROWS * B, COLS * B  # 103 token tiles of 128, the last of 91; 5·103 = 515 and 7·103 = 721 workgroups
LIN_NAMES = ("y", "d x", "d values", "d bias")
SLICES = (slice(0, 200), slice(6400, 6600), slice(12947, 13147))


def lin_step(mm, x, values, layout, bias, w):
    """(y, d x, d values[, d bias]) of one forward + backward on fresh leaves."""
    leaves = [x.detach().requires_grad_(True), values.detach().requires_grad_(True)]
    if bias is not None:
        leaves.append(bias.detach().requires_grad_(True))
    y = mm.block_sparse_linear(leaves[0], leaves[1], layout, leaves[2] if bias is not None else None)
    return (y.detach(),) + torch.autograd.grad(y, leaves, grad_outputs=w)


def assert_linear_tiles(cmm, tokens, tile):
    assert cmm.bsr_linear_tile_tokens(FOUT, tokens) == tile, f"y: {FOUT // B} blocks x {tokens} tokens"
    assert cmm.bsr_linear_tile_tokens(FIN, tokens) == tile, f"d x: {FIN // B} blocks x {tokens} tokens"


@functools.lru_cache(maxsize=None)
def linear_exact_case():
    """Integer operands of the 13147-token layer and its float64 results on the CPU (y without the bias); the longest sum,
    of d values, has 13147 terms of at most 64 each: below 2²⁴, exact in fp32."""
    values, x, w, bias = ints((NNZ, B, B), 31), ints((TOKENS, FIN), 32), ints((TOKENS, FOUT), 33), ints((FOUT,), 34)
    W = densify(values)
    want = (x @ W.T + 0.0, w @ W + 0.0, kept_blocks(w.T @ x) + 0.0, w.sum(0) + 0.0)
    assert float(want[2].abs().max()) < 2 ** 24
    return values, x, w, bias, want


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("form", ["vec", "checked"])
def test_block_linear_wide_tile_is_exact(mm, cmm, dev, dtype, with_bias, form):
    assert_linear_tiles(cmm, TOKENS, 128)
    assert (ROWS * -(-TOKENS // 128)) % 8 == 3 and TOKENS % 128 == 91  # the XCD remap's remainder, a ragged last token tile
    values, x, w, bias, want = linear_exact_case()
    want = (want[0] + bias if with_bias else want[0],) + want[1:3] + ((want[3],) if with_bias else ())
    want = tuple(v.to(dtype) for v in want)
    values, x, w = (v.to(dtype).to(dev) for v in (values, x, w))
    bias = bias.to(dtype).to(dev) if with_bias else None
    if form == "checked":
        x, w = offset_view(x), offset_view(w)
        assert x.stride(0) % 8 != 0 and w.stride(0) % 8 != 0
    layout = layout_from_rows(WIDE, COLS, dev, INDEX[dtype])
    got = lin_step(mm, x, values, layout, bias, w)
    assert len(got) == len(want)
    for name, g, e in zip(LIN_NAMES, got, want):
        assert_same_bits(g, e, f"{form}: {name}")
    cols = slice(EMPTY_ROW * B, (EMPTY_ROW + 1) * B)
    empty = bias.cpu()[cols].expand(TOKENS, B) if with_bias else torch.zeros(TOKENS, B, dtype=dtype)  # +0, not −0
    assert_same_bits(got[0][:, cols], empty, "the empty block row of W in y")
    assert_same_bits(got[1][:, UNKEPT_COL * B:(UNKEPT_COL + 1) * B], torch.zeros(TOKENS, B, dtype=dtype), "the never-kept block column in d x")
    # the entries themselves, into outputs pre-filled with NaN (checked: column-offset views, the element-wise stores)
    (offsets, columns, ids, entry_row, n), (t_off, t_col, t_ids) = lists_of(mm, layout, dev)
    pad = 1 if form == "checked" else 0
    y_big, dx_big = nan_like(TOKENS, FOUT + pad, dev=dev, dtype=dtype), nan_like(TOKENS, FIN + pad, dev=dev, dtype=dtype)
    y, dx, dvalues = y_big[:, pad:], dx_big[:, pad:], nan_like(n, B, B, dev=dev, dtype=dtype)
    assert form == "vec" or (y.data_ptr() % 16 != 0 and y.stride(0) % 8 != 0 and dx.stride(0) % 8 != 0)
    cmm.bsr_linear(offsets, columns, ids, n, values, x, bias, y, False)
    cmm.bsr_linear(t_off, t_col, t_ids, n, values, w, None, dx, True)
    cmm.bsr_wgrad(entry_row, columns, ids, n, w, x, dvalues)
    for name, g, e in zip(LIN_NAMES, (y, dx, dvalues), want):
        assert_same_bits(g, e, f"{form}, pre-filled: {name}")
    if with_bias:  # the transposed lists with the bias epilogue: no caller in the package, an instantiation all the same
        bias_in = ints((FIN,), 35)
        dx.fill_(NAN)
        cmm.bsr_linear(t_off, t_col, t_ids, n, values, w, bias_in.to(dtype).to(dev), dx, True)
        assert_same_bits(dx, (linear_exact_case()[4][1] + bias_in).to(dtype), f"{form}, pre-filled: d x + a bias")
    if pad:
        assert bool(torch.isnan(y_big[:, 0].float()).all()) and bool(torch.isnan(dx_big[:, 0].float()).all()), "the column beside the view"


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("form", ["vec", "checked"])
def test_block_linear_wide_tile_has_the_bits_of_the_narrow_tile_and_of_the_dense_product(mm, cmm, dev, dtype, with_bias, form):
    assert_linear_tiles(cmm, TOKENS, 128)
    assert_linear_tiles(cmm, 200, 64)
    layout = layout_from_rows(WIDE, COLS, dev, INDEX[dtype])
    values = randn((NNZ, B, B), dev, dtype, 41)
    x, w = randn((TOKENS, FIN), dev, dtype, 42), randn((TOKENS, FOUT), dev, dtype, 43)
    bias = randn((FOUT,), dev, dtype, 44) if with_bias else None
    W = densify(values)
    dense_y, dense_dx = nan_like(TOKENS, FOUT, dev=dev, dtype=dtype), nan_like(TOKENS, FIN, dev=dev, dtype=dtype)
    if with_bias:
        cmm.cublas_mmul_bias(x, W, bias, dense_y, False, True)
    else:
        cmm.cublas_mmul(x, W, dense_y, False, True)
    cmm.cublas_mmul(w, W, dense_dx, False, False)
    if form == "checked":
        x, w = offset_view(x), offset_view(w)
    y, dx = lin_step(mm, x, values, layout, bias, w)[:2]
    assert_same_bits(y, dense_y, "y against the dense product")
    assert_same_bits(dx, dense_dx, "d x against the dense product")
    for s in SLICES:
        y1, dx1 = lin_step(mm, x[s], values, layout, bias, w[s])[:2]  # 200 tokens: 10 / 14 workgroups, the 64 tile
        assert_same_bits(y[s], y1, f"y of tokens {s.start}:{s.stop} alone")
        assert_same_bits(dx[s], dx1, f"d x of tokens {s.start}:{s.stop} alone")


# ---- the dense product: gemm_lowp_kernel<·, ·, ·, 128, 128, ·> ---------------------------------------------------------

G_ITEMS, G_M, G_N, G_K, ALONE = 60, 300, 290, 72, 37  # 3 · 3 · 60 = 540 tiles of 128 × 128; ragged 64-tile and 32-step of k
SUFFIX = {torch.bfloat16: "bf16", torch.float16: "f16"}
FORMS = [(ta, tb, vec) for ta in (False, True) for tb in (False, True) for vec in (True, False)]


def placed(x, vec, fill, dev):
    """[items, rows, cols] on the device inside a buffer of its own, everything else `fill`.  vec: a 16-byte aligned base, the
    leading dimension and the item stride multiples of 8 — the 16-byte form; else a 2-byte offset, an odd leading dimension
    and an item stride that is no multiple of 8 — the checked form."""
    items, rows, cols = x.shape
    ld = (cols + 15) // 8 * 8 if vec else cols + 1 + cols % 2
    stride = rows * ld + (8 if vec else 1)
    offset = 0 if vec else 1
    buf = torch.full((offset + items * stride + 8,), fill, dtype=x.dtype, device=dev)
    view = buf[offset:].as_strided((items, rows, cols), (stride, ld, 1))
    view.copy_(x)
    assert (view.data_ptr() % 16 == 0 and ld % 8 == 0 and stride % 8 == 0) if vec else (view.data_ptr() % 16 == 2 and ld % 2 == 1 and stride % 8 != 0)
    return Padded(buf, view, ld, stride)


def assert_padding_untouched(p, what):
    """Every element of the buffer of `p` outside its logical region (which may start at an offset) is still SENTINEL."""
    inside = torch.zeros(p.buf.shape, dtype=torch.bool, device=p.buf.device)
    inside.as_strided(p.x.shape, p.x.stride(), p.x.storage_offset()).fill_(True)
    rest = p.buf[~inside]
    assert rest.numel() == p.buf.numel() - p.x.numel()
    assert_same_bits(rest, torch.full_like(rest, SENTINEL), f"{what}: outside the logical region")


def placed_vector(x, vec, dev):
    buf = torch.full((x.numel() + 9,), NAN, dtype=x.dtype, device=dev)
    view = buf[0 if vec else 1:][:x.numel()]
    view.copy_(x)
    return view


def gemm_through_the_c_abi(capi, dtype, ta, tb, a, b, bias, c, items=G_ITEMS):
    """mi_gemm_T / mi_gemm_bias_T on the first `items` items of Padded operands; returns the status."""
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    head, tail = [ctypes.c_int, ctypes.c_int, i32, i32, i32, vp, i64, i64, vp, i64, i64], [vp, i64, i64, i32, vp]
    at = lambda p: p.x.data_ptr()  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    if bias is None:
        fn = getattr(capi, f"mi_gemm_{SUFFIX[dtype]}")
        fn.argtypes = head + tail
        return fn(int(ta), int(tb), G_M, G_N, G_K, at(a), a.ld, a.stride, at(b), b.ld, b.stride, at(c), c.ld, c.stride, items, stream)
    fn = getattr(capi, f"mi_gemm_bias_{SUFFIX[dtype]}")
    fn.argtypes = head + [vp] + tail
    return fn(int(ta), int(tb), G_M, G_N, G_K, at(a), a.ld, a.stride, at(b), b.ld, b.stride, bias.data_ptr(), at(c), c.ld, c.stride,
              items, stream)


@functools.lru_cache(maxsize=None)
def gemm_exact_case():
    """Integer operands [60, 300, 72] and [60, 72, 290] with a bias [290], and the float64 products on the CPU."""
    a, b, bias = ints((G_ITEMS, G_M, G_K), 51), ints((G_ITEMS, G_K, G_N), 52), ints((G_N,), 53)
    return a, b, bias, a @ b + 0.0


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("operands", ["integers", "randn"])
def test_dense_wide_tile_every_transpose_and_alignment_form(cmm, capi, dev, dtype, with_bias, operands):
    """All four storage transposes × (16-byte form, checked form) of one batched product — with the bias epilogue and
    without — at the 128 × 128 tile: the same bits in all eight, and in item 37 run alone at the 128 × 64 tile.  Integer
    operands: the float64 product narrowed to T.  The operands lie in NaN-filled buffers with leading dimensions and item
    strides of their own (the contiguous C of custom_mm.cublas_bmm has n = 290 columns, no multiple of 8: only the C-ABI
    reaches the 16-byte form at this shape); the padding of C must stay untouched."""
    assert cmm.gemm_lowp_tile_n(G_M, G_N, G_ITEMS) == 128 and cmm.gemm_lowp_tile_n(G_M, G_N, 1) == 64
    if operands == "integers":
        a, b, bias, want = gemm_exact_case()
        want = (want + bias if with_bias else want).to(dtype)
        a, b, bias = a.to(dtype), b.to(dtype), bias.to(dtype)
    else:
        a, b, bias = (randn(s, "cpu", dtype, 54 + i) for i, s in enumerate(((G_ITEMS, G_M, G_K), (G_ITEMS, G_K, G_N), (G_N,))))
        want = None
    first = None
    for ta, tb, vec in FORMS:
        what = f"{'T' if ta else 'N'}{'T' if tb else 'N'} {'vec' if vec else 'checked'}"
        pa = placed(a.transpose(1, 2) if ta else a, vec, NAN, dev)
        pb = placed(b.transpose(1, 2) if tb else b, vec, NAN, dev)
        pbias = placed_vector(bias, vec, dev) if with_bias else None
        pc = placed(torch.zeros(G_ITEMS, G_M, G_N, dtype=dtype), vec, SENTINEL, dev)
        pc.x.fill_(NAN)
        assert gemm_through_the_c_abi(capi, dtype, ta, tb, pa, pb, pbias, pc) == 0, what
        assert_padding_untouched(pc, what)
        got = pc.x.cpu()
        if want is not None:
            assert_same_bits(got, want, f"{what}: against float64")
        if first is None:
            first = got
        assert_same_bits(got, first, f"{what}: against NN vec")
        alone = placed(torch.zeros(1, G_M, G_N, dtype=dtype), vec, SENTINEL, dev)
        alone.x.fill_(NAN)
        item = lambda p: Padded(p.buf, p.x[ALONE:], p.ld, p.stride)  # noqa: E731
        assert gemm_through_the_c_abi(capi, dtype, ta, tb, item(pa), item(pb), pbias, alone, items=1) == 0, what
        assert_padding_untouched(alone, f"{what}: item {ALONE} alone")
        assert_same_bits(alone.x[0], first[ALONE], f"{what}: item {ALONE} alone, the 128 x 64 tile")
    # the binding's own path to the same kernels: contiguous operands (n = 290: the checked form)
    if not with_bias:
        c = nan_like(G_ITEMS, G_M, G_N, dev=dev, dtype=dtype)
        cmm.cublas_bmm(a.to(dev), b.to(dev), c, 3, False, False)
        assert_same_bits(c, first, "custom_mm.cublas_bmm")
