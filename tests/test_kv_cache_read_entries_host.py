"""The 28 C entries that READ the KV cache on the matrix cores — 8 decode, 4 decode over lists, 16 prefill (unsplit and
split) — refuse the same faults, and answer the same empty calls, in the same way, by ctypes on the built library.  Two
tables: the cache faults of test_kv_cache_entries_host.py, sent through the 20 entries that file does not reach, and the
refusals that are not about the cache, one fault a row, with the pairs that show which refusal wins.  The expected statuses
are those of decode_entry and prefill_entry before their shared lines were moved beside the cache checks.

The addresses are made up and nothing may dereference them: EVERY row ends in a refusal, or in an empty call (items == 0 or
T == 0) that returns before the first HIP call — no row is a valid call, and the test checks that rule itself.  Where "this is
accepted" can be shown at all, it is shown by running on into a later refusal with a status of its own: the second table's
argument lists of the entries that take a workspace name two chunks / two parts and a workspace of 0 bytes, so that a list
without a fault is refused last of all with MI_ENOMEM.  The unsplit prefill entries have no such last refusal: their rows
are refusals only."""
import ctypes
import re
from pathlib import Path

import pytest

from test_kv_cache_entries_host import (CACHE, EINVAL, ENOMEM, ERANGE, F32, FAULTS, FP8, I32, I64, LENS, LIST, OK, PAGED, PTR, Q,
                                        SCALES, SIZES, STREAM, SZ, TABLE, VP, WIDTH, signature, valid)

DECODE, LISTS, PREFILL, SPLIT = "decode", "lists", "prefill", "split"
ALL = (DECODE, LISTS, PREFILL, SPLIT)
LAYOUT = (DECODE, PREFILL, SPLIT)  # the entries that take a CSR layout
WS = (DECODE, LISTS, SPLIT)        # … a workspace
BOTH_PREFILL = (PREFILL, SPLIT)

OUT = [("out", VP), ("ldo", I64), ("strideO", I64), ("lse", VP)]
WORKSPACE = [("workspace", VP), ("workspace_bytes", SZ)]


def read_signature(family, paged, fp8):
    """The parameter list of a reading entry, in the header's order."""
    table, scales = (TABLE if paged else []), (SCALES if fp8 else [])
    if family == DECODE:
        return signature("decode", paged, fp8)
    if family == LISTS:
        return ([("block_ids", VP), ("block_counts", VP), ("K", I32)] + SIZES + table + WIDTH + Q + CACHE + LENS +
                [("group", I32), ("chunk", I32), ("scale", F32)] + OUT + WORKSPACE + STREAM)
    return (LIST + SIZES + table + WIDTH + [("q", VP), ("ldq", I64), ("headQ", I64), ("batchQ", I64)] + CACHE + LENS +
            [("new_lens", VP), ("new_lens_count", I32), ("group", I32), ("scale", F32)] + scales + OUT +
            ([("split", I32)] + WORKSPACE if family == SPLIT else []) + STREAM)


def read_valid(paged):
    """valid() of the cache table with what the lists and the prefill entries add: lists of one entry, no new_lens, parts
    of one entry (Smax = 64: one chunk, one part — no workspace)."""
    a = valid(paged)
    a.update(block_ids=PTR, block_counts=PTR, K=1, new_lens_count=0, split=1)
    return a


# what the second table's argument lists add: two chunks / two parts and a workspace of 0 bytes, so that the list without a
# fault is refused with MI_ENOMEM by the last check ahead of the launch
LAST_REFUSAL = {
    DECODE: dict(Smax=128, table_ld=8, workspace=PTR, workspace_bytes=0),
    LISTS: dict(K=2, workspace=PTR, workspace_bytes=0),
    SPLIT: dict(Smax=128, table_ld=8, workspace=PTR, workspace_bytes=0),
    PREFILL: {},
}
# the bytes of those workspaces: [items 1][T 1][chunks 2][group 1][D + 2] floats; [items · group 1][tiles 2][parts 2][64][D + 2]
NEED = {DECODE: 2 * 34 * 4, LISTS: 2 * 34 * 4, SPLIT: 2 * 2 * 64 * 34 * 4}

ENTRIES = ([(DECODE, f"mi_block_attention_decode{p}{f}_{t}", bool(p), bool(f))
            for p in ("", "_paged") for f in ("", "_fp8") for t in ("bf16", "f16")] +
           [(LISTS, f"mi_block_attention_decode_lists{p}_{t}", bool(p), False) for p in ("", "_paged") for t in ("bf16", "f16")] +
           [(fam, f"mi_block_attention_prefill{s}{p}{f}_{t}", bool(p), bool(f))
            for fam, s in ((PREFILL, ""), (SPLIT, "_split")) for p in ("", "_paged") for f in ("", "_fp8") for t in ("bf16", "f16")])
NEW_ENTRIES = [e for e in ENTRIES if e[0] != DECODE]  # the 20 the cache table does not reach in its own file

# (name, the families it goes to, PAGED / FP8 / None, what it changes, the status — one literal, or a dict by family)
REFUSALS = [
    ("no fault: the workspace of 0 bytes", WS, None, {}, ENOMEM),
    ("group 0", ALL, None, dict(group=0), EINVAL),
    ("group 17", (DECODE, LISTS), None, dict(group=17), EINVAL),
    ("chunk 0", (DECODE, LISTS), None, dict(chunk=0), EINVAL),
    ("split 0", (SPLIT,), None, dict(split=0), EINVAL),
    ("D 48", ALL, None, dict(D=48, ldq=48, ldo=48, ldk=48, ldv=48), EINVAL),
    ("Smax 96", ALL, None, dict(Smax=96, table_ld=8), EINVAL),
    ("nnz -1", LAYOUT, None, dict(nnz=-1), EINVAL),
    ("nnz 2^31", LAYOUT, None, dict(nnz=2 ** 31), ERANGE),
    ("items · T · K = 2^32", (LISTS,), None, dict(items=65536, T=65536, K=1), ERANGE),
    ("items 65536", (DECODE, LISTS), None, dict(items=65536), EINVAL),
    ("T 65536", (DECODE, LISTS), None, dict(T=65536), EINVAL),
    ("layouts 0", LAYOUT, None, dict(layouts=0), EINVAL),
    ("heads 0", ALL, None, dict(heads=0), EINVAL),
    ("items % heads", ALL, None, dict(items=3, heads=2), EINVAL),
    ("lens_count 0", ALL, None, dict(lens_count=0), EINVAL),
    ("lens_count no divisor", ALL, None, dict(items=3, heads=3, lens_count=2), EINVAL),
    ("null rowptr", LAYOUT, None, dict(rowptr=None), EINVAL),
    ("null col", LAYOUT, None, dict(col=None), EINVAL),
    ("null block_ids", (LISTS,), None, dict(block_ids=None), EINVAL),
    ("null k_lens", ALL, None, dict(k_lens=None), EINVAL),
    ("k_lens off by 2 bytes", ALL, None, dict(k_lens=PTR + 2), EINVAL),
    ("null lse", ALL, None, dict(lse=None), EINVAL),
    ("lse off by 2 bytes", ALL, None, dict(lse=PTR + 2), EINVAL),
    ("null q", ALL, None, dict(q=None), EINVAL),
    ("q off by 8 bytes", ALL, None, dict(q=PTR + 8), EINVAL),
    ("null out", ALL, None, dict(out=None), EINVAL),
    ("out off by 8 bytes", ALL, None, dict(out=PTR + 8), EINVAL),
    ("ldq < D", (DECODE, LISTS), None, dict(ldq=16), EINVAL),
    ("ldq < D, T 2", BOTH_PREFILL, None, dict(ldq=16, T=2), EINVAL),
    # (one token has no second row: its ldq is not looked at — shown where a later refusal exists)
    ("ldq < D, T 1", (SPLIT,), None, dict(ldq=16), ENOMEM),
    ("ldo < D", ALL, None, dict(ldo=16), EINVAL),
    ("strideQ 4", (DECODE, LISTS), None, dict(strideQ=4), EINVAL),
    ("headQ 4", BOTH_PREFILL, None, dict(headQ=4), EINVAL),
    ("batchQ 4", BOTH_PREFILL, None, dict(batchQ=4), EINVAL),
    ("strideO 4", ALL, None, dict(strideO=4), EINVAL),
    ("new_lens off by 2 bytes", BOTH_PREFILL, None, dict(new_lens=PTR + 2, new_lens_count=1), EINVAL),
    ("new_lens_count 2 for 3 batch items", BOTH_PREFILL, None, dict(items=3, new_lens=PTR, new_lens_count=2), EINVAL),
    ("K 0", (LISTS,), None, dict(K=0), EINVAL),
    ("K -1", (LISTS,), None, dict(K=-1), EINVAL),
    ("null block_counts", (LISTS,), None, dict(block_counts=None), EINVAL),
    ("block_ids off by 2 bytes", (LISTS,), None, dict(block_ids=PTR + 2), EINVAL),
    ("block_counts off by 2 bytes", (LISTS,), None, dict(block_counts=PTR + 2), EINVAL),
    ("null workspace", WS, None, dict(workspace=None), EINVAL),
    ("workspace off by 8 bytes", WS, None, dict(workspace=PTR + 8), EINVAL),
    ("workspace one byte short", WS, None, dict(workspace_bytes="need - 1"), ENOMEM),
    # which refusal wins, where the entries decide it
    ("page 24 + items 0", ALL, PAGED, dict(page=24, items=0), EINVAL),
    ("2 scales for 3 heads + T 0", ALL, FP8, dict(items=3, heads=3, k_scale_count=2, T=0), EINVAL),
    ("nnz 2^31 + items 0", LAYOUT, None, dict(nnz=2 ** 31, items=0), ERANGE),
    ("items 65536 + T 0", (DECODE, LISTS), None, dict(items=65536, T=0), EINVAL),
    ("null k + the workspace of 0 bytes", WS, None, dict(k=None), EINVAL),
    ("null q + the workspace of 0 bytes", WS, None, dict(q=None), EINVAL),
    # the empty calls, answered before a pointer is looked at
    ("items 0", ALL, None, dict(items=0, q=None, out=None, lse=None, k_lens=None, rowptr=None, col=None, workspace=None), OK),
    ("T 0", ALL, None, dict(T=0, q=None, out=None, lse=None, k_lens=None, rowptr=None, col=None, workspace=None), OK),
]


def cache_rows(family, paged, fp8):
    """The cache table's rows for an entry: (title, arguments, status).  A row whose status is a dict by family shows "this
    is accepted" by two chunks and a workspace too small; the lists get their two chunks from K = 2, the split entries their
    two parts from the row's Smax = 128, and the unsplit prefill entries, which have no workspace, leave such a row out."""
    for title, where, change, status in FAULTS:
        if (where == PAGED and not paged) or (where == FP8 and not fp8):
            continue
        args = read_valid(paged)
        if isinstance(status, dict):
            status = status.get("decode")
            if status is None or family == PREFILL or (family == LISTS and "nnz" in change):  # (the lists have no nnz)
                continue
            args.update(K=2)
        args.update(change)
        yield title, args, status


def refusal_rows(family, paged, fp8):
    for title, families, where, change, status in REFUSALS:
        if family not in families or (where == PAGED and not paged) or (where == FP8 and not fp8):
            continue
        args = read_valid(paged)
        args.update(LAST_REFUSAL[family])
        assert set(change) <= set(args), title
        args.update(change)
        if args["workspace_bytes"] == "need - 1":
            args["workspace_bytes"] = NEED[family] - 1
        yield title, args, status.get(family) if isinstance(status, dict) else status


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    return ctypes.CDLL(str(built / "libmi_spmm.so"))


def test_the_tables_name_every_reading_entry():
    header = (Path(__file__).resolve().parent.parent / "include" / "mi_spmm.h").read_text()
    declared = set(re.findall(r"\bint\s+(mi_block_attention_(?:decode|prefill)\w*)\(", header))
    assert declared == {name for _, name, _, _ in ENTRIES} and len(ENTRIES) == 28 and len(NEW_ENTRIES) == 20
    assert [f for f, _, _, _ in ENTRIES].count(DECODE) == 8 and [f for f, _, _, _ in ENTRIES].count(LISTS) == 4


@pytest.mark.parametrize("family,name,paged,fp8", ENTRIES, ids=[e[1] for e in ENTRIES])
def test_no_row_is_a_valid_call(family, name, paged, fp8):
    """The rule of this file: a row that expects MI_OK is an empty call."""
    rows = list(refusal_rows(family, paged, fp8)) + (list(cache_rows(family, paged, fp8)) if family != DECODE else [])
    for title, args, status in rows:
        assert status in (EINVAL, ERANGE, ENOMEM) or (status == OK and (args["items"] == 0 or args["T"] == 0)), f"{name}, {title}"


def send(lib, family, name, paged, fp8, rows):
    sig = read_signature(family, paged, fp8)
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [t for _, t in sig], ctypes.c_int
    sent = 0
    for title, args, expect in rows:
        assert expect != OK or args["items"] == 0 or args["T"] == 0, title
        got = fn(*[args[n] for n, _ in sig])
        assert got == expect, f"{name}, {title}: status {got}, expected {expect}"
        sent += 1
    return sent


@pytest.mark.parametrize("family,name,paged,fp8", NEW_ENTRIES, ids=[e[1] for e in NEW_ENTRIES])
def test_cache_faults_and_empty_calls(lib, family, name, paged, fp8):
    assert send(lib, family, name, paged, fp8, cache_rows(family, paged, fp8)) >= 9


@pytest.mark.parametrize("family,name,paged,fp8", ENTRIES, ids=[e[1] for e in ENTRIES])
def test_refusals_that_are_not_about_the_cache(lib, family, name, paged, fp8):
    assert send(lib, family, name, paged, fp8, refusal_rows(family, paged, fp8)) >= 30
