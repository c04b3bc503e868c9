"""Malformed block lists under the block-sparse kernels on the MI355X (include/mi_spmm.h, mi_bsr_mm / mi_bsr_sddmm /
mi_bsr_linear / mi_bsr_wgrad): "A listed column outside the grid or an entry id outside the values is skipped, offsets are
clamped to [0, nnz]: a malformed list cannot make a kernel read outside the operands".  The binding checks dtypes, sizes
and contiguity only, so hand-made int32 lists reach the kernels as they are — the front end, which builds well-formed
lists, is not involved.

The lists (tests/block_lists_malformed.py) are off by ONE position everywhere, and live NaN-filled memory lies there: one
sentinel block on each side of values, one block of 64 rows (bsr_mm / bsr_sddmm) or 64 columns (bsr_linear / bsr_wgrad) on
each side of every dense operand, two well-formed entries in front of columns / ids and three behind.  A kernel that lost a
guard reads NaN or an extra entry and fails the comparison; it cannot leave an allocation
(tests/test_block_lists_malformed_host.py walks the lists with each guard removed).
  * bsr_mm (plain, trans_a) and bsr_linear (plain, trans_w, with bias): the bits of the same entry on the cleaned list — the
    list read literally by a few lines of Python — and no NaN;
  * bsr_sddmm and bsr_wgrad (one range, and two ranges of 64 tokens): an entry outside the grid stores a +0 block, an entry
    with an id outside the values writes nothing (the sentinel blocks around dvalues keep their bits), every other block has
    the bits of the clean run.
A 4 × 4 block grid, widths 40 and 136, both alignment forms."""
import pytest
import torch

import block_lists_malformed as L
from gpu_helpers import SENTINEL, assert_same_bits

pytestmark = pytest.mark.gpu

LOWP = (torch.bfloat16, torch.float16)
B = 64
DIM = L.BLOCKS * B
NAN = float("nan")


def randn(shape, dev, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(dev)


def i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


def inside(head, body, tail, dev):
    """`body + tail` as a contiguous int32 view behind `head` in one buffer."""
    view = i32(head + body + tail, dev)[len(head):]
    assert view.is_contiguous() and view.numel() == len(body) + len(tail)
    return view


def row_lists(dev):
    """(malformed, clean): (offsets, columns, ids, nnz) of the row list as it stands and as it reads."""
    bad = (i32(L.OFFSETS, dev), inside(L.COLUMNS_HEAD, L.COLUMNS, L.COLUMNS_TAIL, dev), inside(L.IDS_HEAD, L.IDS, L.IDS_TAIL, dev), L.NNZ)
    off, col, idx = L.cleaned(L.OFFSETS, L.COLUMNS + L.COLUMNS_TAIL, L.IDS + L.IDS_TAIL, L.NNZ, L.BLOCKS, L.NVALUES)
    assert (off, col, idx) == L.CLEAN
    return bad, (i32(off, dev), i32(col, dev), i32(idx, dev), len(col))


def between_sentinels(dev, dtype, seed, fill):
    """(buffer [NVALUES + 2, 64, 64], its view [1 : NVALUES + 1]): random blocks between two blocks of `fill`; the view is
    contiguous and 16-byte aligned."""
    buffer = randn((L.NVALUES + 2, B, B), dev, dtype, seed)
    buffer[0] = buffer[-1] = fill
    view = buffer[1:L.NVALUES + 1]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buffer, view


def row_padded(x, form):
    """[items, DIM, N] as a view of a NaN buffer with one block of 64 rows on each side (checked: and one column in front)."""
    pad = 0 if form == "vec" else 1
    big = torch.full((x.shape[0], DIM + 2 * B, x.shape[2] + pad), NAN, device=x.device, dtype=x.dtype)
    view = big[:, B:-B, pad:]
    view.copy_(x)
    assert (view.data_ptr() % 16 == 0) == (form == "vec")
    return view


def col_padded(x, form):
    """[T, DIM] as a view of a NaN buffer with one block of 64 columns on each side (checked: 65 in front, an odd leading
    dimension)."""
    pad = 0 if form == "vec" else 1
    big = torch.full((x.shape[0], DIM + 2 * B + pad), NAN, device=x.device, dtype=x.dtype)
    view = big[:, B + pad:B + pad + DIM]
    view.copy_(x)
    assert (view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0) == (form == "vec")
    return view


def finite(x):
    return bool(torch.isfinite(x.float()).all())


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [40, 136])
@pytest.mark.parametrize("form", ["vec", "checked"])
def test_bsr_mm_reads_a_malformed_list_as_the_clean_list(cmm, dev, dtype, N, form):
    bad, clean = row_lists(dev)
    _, values = between_sentinels(dev, dtype, 1, NAN)
    b = row_padded(randn((2, DIM, N), dev, dtype, 2 + N), form)
    for trans_a in (False, True):
        got, want = (torch.full((2, DIM, N), NAN, device=dev, dtype=dtype) for _ in range(2))
        cmm.bsr_mm(*bad, values, b, got, trans_a)
        cmm.bsr_mm(*clean, values, b, want, trans_a)
        assert finite(want) and finite(got), f"trans_a={trans_a}: NaN reached the output"
        assert_same_bits(got, want, f"trans_a={trans_a}")
        assert_same_bits(got[:, B:2 * B], torch.zeros(2, B, N, dtype=dtype), "the row with lo > hi is empty: +0")
        assert bool((got[:, :B] != 0).any()) and bool((got[:, 3 * B:] != 0).any())


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("T", [40, 136])
@pytest.mark.parametrize("form", ["vec", "checked"])
def test_bsr_linear_reads_a_malformed_list_as_the_clean_list(cmm, dev, dtype, T, form):
    bad, clean = row_lists(dev)
    _, values = between_sentinels(dev, dtype, 11, NAN)
    x = col_padded(randn((T, DIM), dev, dtype, 12 + T), form)
    bias = randn((DIM,), dev, dtype, 13)
    for trans_w, with_bias in ((False, False), (True, False), (False, True)):
        got, want = (torch.full((T, DIM), NAN, device=dev, dtype=dtype) for _ in range(2))
        cmm.bsr_linear(*bad, values, x, bias if with_bias else None, got, trans_w)
        cmm.bsr_linear(*clean, values, x, bias if with_bias else None, want, trans_w)
        what = f"trans_w={trans_w} bias={with_bias}"
        assert finite(want) and finite(got), f"{what}: NaN reached the output"
        assert_same_bits(got, want, what)
        empty = bias.cpu()[B:2 * B].expand(T, B) if with_bias else torch.zeros(T, B, dtype=dtype)
        assert_same_bits(got[:, B:2 * B], empty, f"{what}: the row with lo > hi is empty")


def entry_lists(dev):
    """(malformed, clean): (entry_row, columns, ids, nnz) of the entry list as it stands, and of its computed entries."""
    rows_tail, cols_tail, ids_tail = L.E_TAIL
    bad = (i32(L.E_ROWS + rows_tail, dev), i32(L.E_COLS + cols_tail, dev), i32(L.E_IDS + ids_tail, dev), L.E_NNZ)
    clean = tuple(i32([entry[k] for entry in L.E_COMPUTED], dev) for k in range(3)) + (len(L.E_COMPUTED),)
    return bad, clean


def check_sampled(run, dev, dtype, what):
    """run(list, dvalues) on the malformed and on the clean entry list, each into NaN blocks between two SENTINEL blocks."""
    bad, clean = entry_lists(dev)
    (got_buffer, got), (want_buffer, want) = (between_sentinels(dev, dtype, 21, SENTINEL) for _ in range(2))
    got.fill_(NAN)
    want.fill_(NAN)
    run(bad, got)
    run(clean, want)
    computed = [e for _, _, e in L.E_COMPUTED]
    assert finite(want[computed]) and bool(torch.isnan(want[L.E_ZERO + L.E_UNLISTED].float()).all())
    expect = want.clone()
    expect[L.E_ZERO] = 0.0  # an entry outside the grid: a +0 block
    assert_same_bits(got, expect, what)
    edges = torch.full((2, B, B), SENTINEL, dtype=dtype)
    assert_same_bits(got_buffer[[0, -1]], edges, f"{what}: the blocks before and after dvalues")
    assert_same_bits(want_buffer[[0, -1]], edges, f"{what}: the blocks before and after dvalues, clean run")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("N", [40, 136])
@pytest.mark.parametrize("form", ["vec", "checked"])
def test_bsr_sddmm_zeroes_entries_outside_the_grid_and_skips_ids_outside_the_values(cmm, dev, dtype, N, form):
    dc = row_padded(randn((2, DIM, N), dev, dtype, 31 + N), form)
    b = row_padded(randn((2, DIM, N), dev, dtype, 32 + N), form)
    check_sampled(lambda lst, dvalues: cmm.bsr_sddmm(*lst, dc, b, dvalues), dev, dtype, f"N={N}")


@pytest.mark.parametrize("dtype", LOWP)
@pytest.mark.parametrize("T,splits", [(40, 1), (136, 1), (128, 2)])
@pytest.mark.parametrize("form", ["vec", "checked"])
def test_bsr_wgrad_zeroes_entries_outside_the_grid_and_skips_ids_outside_the_values(cmm, dev, dtype, T, splits, form):
    dy = col_padded(randn((T, DIM), dev, dtype, 41 + T), form)
    x = col_padded(randn((T, DIM), dev, dtype, 42 + T), form)
    check_sampled(lambda lst, dvalues: cmm.bsr_wgrad(*lst, dy, x, dvalues, splits), dev, dtype, f"T={T} splits={splits}")
