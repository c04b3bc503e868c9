"""The KV-cache family's C entries refuse the same cache faults, and answer the same empty calls, in the same way: one
table of faults sent through all 22 entries that take a cache — 8 decode, 6 append, 8 rope + append — by ctypes on the
built library.  Every argument list here returns before the first HIP call (the pointers are made-up addresses that
nothing dereferences), so the test needs no GPU.  The expected statuses are those of the three units' entry functions
before their cache checks were moved into csrc/kv_cache_device.h."""
import ctypes

import pytest

OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
PTR = 0x10000  # a made-up 16-byte aligned address

I32, I64, VP, F32, SZ = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t

SIZES = [("items", I32), ("heads", I32), ("T", I32), ("Smax", I32)]
TABLE = [("block_table", VP), ("table_ld", I64), ("pages", I32), ("page", I32)]
WIDTH = [("D", I32)]
SOURCES = [(n, t) for s in ("kn", "vn") for n, t in ((s[0] + "_new", VP), ("ld" + s, I64), ("head" + s, I64), ("batch" + s, I64))]
CACHE = [("k", VP), ("ldk", I64), ("headK", I64), ("outerK", I64), ("v", VP), ("ldv", I64), ("headV", I64), ("outerV", I64)]
LENS = [("k_lens", VP), ("lens_count", I32)]
SCALES = [("k_scale", VP), ("k_scale_count", I32), ("v_scale", VP), ("v_scale_count", I32)]
STREAM = [("stream", VP)]
LIST = [("rowptr", VP), ("col", VP), ("nnz", I64), ("layouts", I32)]
Q = [("q", VP), ("ldq", I64), ("strideQ", I64)]
ROPE_Q = [("q_heads", I32), ("q", VP), ("ldq", I64), ("headQ", I64), ("batchQ", I64),
          ("q_out", VP), ("ldqo", I64), ("headQo", I64), ("batchQo", I64)]
ROPE_TABLES = [("k_out", VP), ("ldko", I64), ("headKo", I64), ("batchKo", I64), ("cos", VP), ("sin", VP), ("table_rows", I32),
               ("ld", I64), ("rotary_dim", I32), ("interleaved", I32)]


def signature(family, paged, fp8):
    """The parameter list of an entry, in the header's order."""
    table, scales = (TABLE if paged else []), (SCALES if fp8 else [])
    if family == "decode":
        return (LIST + SIZES + table + WIDTH + Q + CACHE + LENS + [("group", I32), ("chunk", I32), ("scale", F32)] + scales +
                [("out", VP), ("ldo", I64), ("strideO", I64), ("lse", VP), ("workspace", VP), ("workspace_bytes", SZ)] + STREAM)
    if family == "append":
        return SIZES + table + WIDTH + SOURCES + CACHE + LENS + scales + STREAM
    return SIZES + table + WIDTH + ROPE_Q + SOURCES + ROPE_TABLES + CACHE + LENS + [("new_lens", VP)] + scales + STREAM


def valid(paged):
    """The smallest valid argument list: one item, one head, one token, D = 32, 64 rows — paged: 4 pages of 16."""
    rows = 16 if paged else 64
    a = dict(items=1, heads=1, T=1, Smax=64, D=32, block_table=PTR, table_ld=4, pages=4, page=16, stream=None,
             k=PTR, ldk=32, headK=rows * 32, outerK=rows * 32, v=PTR, ldv=32, headV=rows * 32, outerV=rows * 32,
             k_lens=PTR, lens_count=1, k_scale=PTR, k_scale_count=1, v_scale=PTR, v_scale_count=1,
             k_new=PTR, ldkn=32, headkn=32, batchkn=32, v_new=PTR, ldvn=32, headvn=32, batchvn=32,
             rowptr=PTR, col=PTR, nnz=1, layouts=1, q=PTR, ldq=32, strideQ=32, group=1, chunk=1, scale=1.0,
             out=PTR, ldo=32, strideO=32, lse=PTR, workspace=None, workspace_bytes=0,
             q_heads=1, headQ=32, batchQ=32, q_out=PTR, ldqo=32, headQo=32, batchQo=32,
             k_out=None, ldko=32, headKo=0, batchKo=0, cos=PTR, sin=PTR, table_rows=64, ld=16, rotary_dim=32, interleaved=0,
             new_lens=None)
    return a


ENTRIES = ([("decode", f"mi_block_attention_decode{p}{f}_{t}", bool(p), bool(f))
            for p in ("", "_paged") for f in ("", "_fp8") for t in ("bf16", "f16")] +
           [("append", f"mi_kv_append{p}_b16", bool(p), False) for p in ("", "_paged")] +
           [("append", f"mi_kv_append{p}_fp8_{t}", bool(p), True) for p in ("", "_paged") for t in ("bf16", "f16")] +
           [("rope", f"mi_rope_kv_append{p}{f}_{t}", bool(p), bool(f))
            for p in ("", "_paged") for f in ("", "_fp8") for t in ("bf16", "f16")])

ANY, PAGED, FP8 = "any", "paged", "fp8"
# (name, the entries it goes to, what it changes in the valid list, the status) — the status is one literal for every entry
# the row goes to, or a dict by family
FAULTS = [
    ("page 8", PAGED, dict(page=8), EINVAL),
    ("page 24", PAGED, dict(page=24), EINVAL),
    ("page 0", PAGED, dict(page=0), EINVAL),
    ("pages -1", PAGED, dict(pages=-1), EINVAL),
    ("Smax % page", PAGED, dict(page=128), EINVAL),
    ("null table", PAGED, dict(block_table=None), EINVAL),
    ("table off by 2 bytes", PAGED, dict(block_table=PTR + 2), EINVAL),
    ("table_ld < Smax / page", PAGED, dict(table_ld=3), EINVAL),
    ("null k", ANY, dict(k=None), EINVAL),
    ("k off by 8 bytes", ANY, dict(k=PTR + 8), EINVAL),
    ("null v", ANY, dict(v=None), EINVAL),
    ("ldk < D", ANY, dict(ldk=16), EINVAL),
    ("ldv < D", ANY, dict(ldv=16), EINVAL),
    ("head stride 4", ANY, dict(headK=4), EINVAL),
    ("outer stride 4 of v", ANY, dict(outerV=4), EINVAL),
    ("head stride 8 of bytes", FP8, dict(headK=8), EINVAL),
    ("2 scales for 3 heads", FP8, dict(items=3, heads=3, k_scale_count=2), EINVAL),
    ("2 v scales for 3 heads", FP8, dict(items=3, heads=3, v_scale_count=2), EINVAL),
    ("scale off by 2 bytes", FP8, dict(k_scale=PTR + 2), EINVAL),
    ("v scale off by 2 bytes", FP8, dict(v_scale=PTR + 2), EINVAL),
    # the empty calls: answered before a pointer is looked at …
    ("items 0", ANY, dict(items=0, k=None, v=None, block_table=None, k_lens=None), OK),
    ("T 0", ANY, dict(T=0, k=None, v=None, block_table=None, k_lens=None), OK),
    # … but after the cache's form
    ("items 0, page 24", PAGED, dict(items=0, page=24), EINVAL),
    ("T 0, 2 scales for 3 heads", FP8, dict(T=0, items=3, heads=3, k_scale_count=2), EINVAL),
    # A cache that is not touched may be null.  The appends then launch nothing.  The decode and rope entries would still
    # launch, so their rows run on into a later refusal with a status of its own — a thread count beyond int32, the
    # workspace of two chunks too small — which a null k that is looked at never reaches.
    ("Smax 0", ANY, dict(Smax=0, k=None, v=None, block_table=None), dict(append=OK)),
    ("pages 0", PAGED, dict(pages=0, k=None, v=None), dict(append=OK)),
    ("Smax 0, beyond int32", ANY, dict(Smax=0, k=None, v=None, block_table=None, T=2 ** 30), dict(append=ERANGE, rope=ERANGE)),
    ("pages 0, beyond int32", PAGED, dict(pages=0, k=None, v=None, T=2 ** 30), dict(append=ERANGE, rope=ERANGE)),
    ("null k, beyond int32", ANY, dict(k=None, T=2 ** 30), dict(append=EINVAL, rope=EINVAL)),
    ("pages 0, two chunks", PAGED, dict(pages=0, k=None, v=None, Smax=128, table_ld=8, workspace=PTR), dict(decode=ENOMEM)),
    # the decode entries alone do not touch the cache of an empty list either
    ("nnz 0, two chunks", ANY, dict(nnz=0, k=None, v=None, Smax=128, table_ld=8, workspace=PTR), dict(decode=ENOMEM)),
    ("null k, two chunks", ANY, dict(k=None, Smax=128, table_ld=8, workspace=PTR), dict(decode=EINVAL)),
]


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    return ctypes.CDLL(str(built / "libmi_spmm.so"))


def test_the_table_names_every_cache_entry():
    import re
    from pathlib import Path
    header = (Path(__file__).resolve().parent.parent / "include" / "mi_spmm.h").read_text()
    declared = set(re.findall(r"\bint (mi_(?:block_attention_decode|kv_append|rope_kv_append)\w*)\(", header))
    assert declared == {name for _, name, _, _ in ENTRIES} and len(ENTRIES) == 22


@pytest.mark.parametrize("family,name,paged,fp8", ENTRIES, ids=[e[1] for e in ENTRIES])
def test_cache_faults_and_empty_calls(lib, family, name, paged, fp8):
    sig = signature(family, paged, fp8)
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [t for _, t in sig], ctypes.c_int
    sent = 0
    for title, where, change, status in FAULTS:
        if (where == PAGED and not paged) or (where == FP8 and not fp8):
            continue
        expect = status.get(family) if isinstance(status, dict) else status
        if expect is None:
            continue
        args = valid(paged)
        assert set(change) <= set(args), title
        args.update(change)
        got = fn(*[args[n] for n, _ in sig])
        assert got == expect, f"{name}, {title}: status {got}, expected {expect}"
        sent += 1
    assert sent >= 11
