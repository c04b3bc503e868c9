"""The hand-made malformed block lists of tests/test_gpu_block_lists_malformed.py, the literal reading of a list that the
kernels promise (include/mi_spmm.h: "A listed column outside the grid or an entry id outside the values is skipped, offsets
are clamped to [0, nnz]"), and a host model of the kernels' list walk with each guard switchable
(tests/test_block_lists_malformed_host.py).

Every out-of-range value is off by ONE position, and the GPU test keeps live, NaN-filled memory there: were a guard
missing, the kernel would read a NaN block (or an extra well-formed entry) and the comparison would fail — it could not
leave its allocations.  The host model checks exactly that for each guard."""

BLOCKS = 4        # the block grid is 4 × 4: every operand is 256 wide
NVALUES = 7       # blocks of values / dvalues; the bad ids are −1 and NVALUES

# ---- the row lists of bsr_mm / bsr_linear: offsets [BLOCKS + 1], columns and ids [NNZ + TAIL] ---------------------------
NNZ, TAIL, HEAD = 9, 3, 2
OFFSETS = [-2, 3, 2, 6, NNZ + TAIL]          # first offset below 0, an interior pair with lo > hi (row 1), last beyond nnz
COLUMNS = [0, -1, 2, BLOCKS, 1, 3, 0, 2, BLOCKS]
IDS = [0, 1, 2, 3, -1, 4, NVALUES, 5, 1]
#          │           │   │       │           └ row 3 ends with a column one past the grid
#          │           │   │       └ row 3 starts with an id one past the values
#          │           │   └ id −1
#          │           └ column one past the grid
#          └ column −1
COLUMNS_TAIL, IDS_TAIL = [0, 1, 2], [0, 1, 2]   # well-formed, beyond nnz: never read
COLUMNS_HEAD, IDS_HEAD = [1, 3], [3, 4]         # well-formed, in front of the arrays (the GPU test passes views): never read
CLEAN = ([0, 2, 2, 4, 5], [0, 2, 2, 3, 2], [0, 2, 2, 4, 5])  # what the list says, read literally: offsets, columns, ids

# ---- the entry lists of bsr_sddmm / bsr_wgrad: one workgroup per entry p < E_NNZ ---------------------------------------
E_NNZ = 8
E_ROWS = [0, -1, 1, BLOCKS, 2, 3, 1, 2]
E_COLS = [1, 0, BLOCKS, 2, -1, 3, 0, 2]
E_IDS = [0, 1, 2, 3, 4, -1, NVALUES, 5]
E_TAIL = ([3, 3, 0], [0, 1, 2], [1, 2, 3])      # (rows, columns, ids) beyond nnz: never read
E_COMPUTED = [(0, 1, 0), (2, 2, 5)]             # (row, column, id) of the entries inside the grid and the values
E_ZERO = [1, 2, 3, 4]                           # ids whose entry lies outside the grid: a +0 block
E_UNLISTED = [6]                                # never written


def cleaned(offsets, columns, ids, nnz, blocks, nvalues):
    """The well-formed list a malformed one stands for: offsets clamped to [0, nnz], entries with a column outside
    [0, blocks) or an id outside [0, nvalues) dropped."""
    off, col, idx = [0], [], []
    for r in range(len(offsets) - 1):
        for p in range(max(offsets[r], 0), min(offsets[r + 1], nnz)):
            if 0 <= columns[p] < blocks and 0 <= ids[p] < nvalues:
                col.append(columns[p])
                idx.append(ids[p])
        off.append(len(col))
    return off, col, idx


ALL_GUARDS = frozenset({"offset below 0", "offset beyond nnz", "column", "id"})


def walk(row, guards=ALL_GUARDS):
    """Host model of the list walk of bsr_mm_kernel / bsr_linear_kernel for one list row (the offset clamps, next_entry) on
    the arrays above, with the guards in `guards` in force: the (position, column, id) of every entry the kernel would load
    operands for.  Positions index COLUMNS_HEAD + COLUMNS + COLUMNS_TAIL from −HEAD."""
    col = dict(enumerate(COLUMNS_HEAD + COLUMNS + COLUMNS_TAIL, -HEAD))
    idx = dict(enumerate(IDS_HEAD + IDS + IDS_TAIL, -HEAD))
    lo, hi = OFFSETS[row], OFFSETS[row + 1]
    if "offset below 0" in guards:
        lo = max(lo, 0)
    if "offset beyond nnz" in guards:
        hi = min(hi, NNZ)
    loaded = []
    for p in range(lo, hi):
        if "column" in guards and not 0 <= col[p] < BLOCKS:
            continue
        if "id" in guards and not 0 <= idx[p] < NVALUES:
            continue
        loaded.append((p, col[p], idx[p]))
    return loaded
