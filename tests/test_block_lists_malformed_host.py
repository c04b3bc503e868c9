"""The malformed block lists of tests/test_gpu_block_lists_malformed.py without a GPU: the lists have every feature the
guards of the block-sparse kernels exist for, their literal reading is the list the GPU test compares against, and — on a
host model of the kernels' list walk — a kernel that LOST one guard would still stay inside the live, NaN-filled memory the
GPU test places around every operand: such a kernel fails the GPU test by reading NaN or one extra well-formed entry, never
by leaving an allocation."""
import pytest

import block_lists_malformed as L


def test_the_row_list_has_every_malformation_and_reads_as_the_clean_list():
    assert L.OFFSETS[0] == -2 and L.OFFSETS[-1] == L.NNZ + 3 and len(L.OFFSETS) == L.BLOCKS + 1
    assert any(lo > hi for lo, hi in zip(L.OFFSETS[1:-1], L.OFFSETS[2:-1]))  # an interior pair: an empty row
    assert len(L.COLUMNS) == len(L.IDS) == L.NNZ and len(L.COLUMNS_TAIL) == len(L.IDS_TAIL) == L.TAIL == L.OFFSETS[-1] - L.NNZ
    assert len(L.COLUMNS_HEAD) == len(L.IDS_HEAD) == L.HEAD == -L.OFFSETS[0]
    assert {-1, L.BLOCKS} <= set(L.COLUMNS) <= set(range(-1, L.BLOCKS + 1))   # off by one position, nothing wilder
    assert {-1, L.NVALUES} <= set(L.IDS) <= set(range(-1, L.NVALUES + 1))
    clean = L.cleaned(L.OFFSETS, L.COLUMNS + L.COLUMNS_TAIL, L.IDS + L.IDS_TAIL, L.NNZ, L.BLOCKS, L.NVALUES)
    assert clean == L.CLEAN
    # the walk with every guard in force loads exactly the clean list: a bad first entry, a bad last entry and two bad
    # entries in a row are passed over
    off, col, idx = L.CLEAN
    for row in range(L.BLOCKS):
        loaded = L.walk(row)
        assert [(c, e) for _, c, e in loaded] == list(zip(col[off[row]:off[row + 1]], idx[off[row]:off[row + 1]])), row
    assert L.walk(1) == [] and len(L.walk(3)) == 1 and L.walk(3)[0][0] == 7


def test_the_entry_list_has_every_malformation():
    assert len(L.E_ROWS) == len(L.E_COLS) == len(L.E_IDS) == L.E_NNZ
    for values, bound in ((L.E_ROWS, L.BLOCKS), (L.E_COLS, L.BLOCKS), (L.E_IDS, L.NVALUES)):
        assert {-1, bound} <= set(values) <= set(range(-1, bound + 1))
    inside = lambda v, bound: 0 <= v < bound  # noqa: E731
    computed, zero = [], []
    for r, c, e in zip(L.E_ROWS, L.E_COLS, L.E_IDS):
        if not inside(e, L.NVALUES):
            continue  # nothing written
        (computed if inside(r, L.BLOCKS) and inside(c, L.BLOCKS) else zero).append((r, c, e))
    assert computed == L.E_COMPUTED and [e for _, _, e in zero] == L.E_ZERO
    written = [e for _, _, e in computed + zero]
    assert len(set(written)) == len(written) and sorted(written + L.E_UNLISTED) == list(range(L.NVALUES))


@pytest.mark.parametrize("lost", sorted(L.ALL_GUARDS))
def test_a_kernel_without_one_guard_reads_nan_or_an_extra_entry_inside_the_allocations(lost):
    """The GPU test keeps HEAD well-formed entries in front of columns / ids and TAIL behind, one NaN block of 64 rows
    (columns) on each side of every dense operand and one NaN block on each side of values.  Without the guard `lost` the
    walk stays inside those, and what it loads differs from the clean list: the GPU test would fail on values, not fault."""
    guards = L.ALL_GUARDS - {lost}
    differs = False
    for row in range(L.BLOCKS):
        loaded = L.walk(row, guards)
        for p, c, e in loaded:
            assert -L.HEAD <= p < L.NNZ + L.TAIL, "columns / ids are read inside their buffers"
            assert -1 <= c <= L.BLOCKS, "the dense operand is read inside its one-block padding"
            assert -1 <= e <= L.NVALUES, "values are read inside the sentinel blocks"
        differs = differs or loaded != L.walk(row)
        if lost == "column":
            assert all(0 <= e < L.NVALUES for _, _, e in loaded)
        if lost == "id":
            assert all(0 <= c < L.BLOCKS for _, c, _ in loaded)
    assert differs
    extra = [x for row in range(L.BLOCKS) for x in L.walk(row, guards) if x not in L.walk(row)]
    if lost == "column":   # NaN rows (columns) of the dense operand's padding, on both sides
        assert {c for _, c, _ in extra} == {-1, L.BLOCKS}
    elif lost == "id":     # the NaN sentinel blocks of values, on both sides
        assert {e for _, _, e in extra} == {-1, L.NVALUES}
    else:                  # well-formed entries in front of / behind the list: finite, but extra products
        assert all(0 <= c < L.BLOCKS and 0 <= e < L.NVALUES for _, c, e in extra)
        assert {p for p, _, _ in extra} == ({-2, -1} if lost == "offset below 0" else {L.NNZ, L.NNZ + 1, L.NNZ + 2})
