"""The tile-level key-block selection and the prefill over lists without a GPU: select_key_blocks_tiles and
block_sparse_attention_prefill_selected[_paged][_fp8] — every refusal with its exception type, before the device; the *_takes
functions and block_attention_prefill_tiles; the tile, candidate and forced rules against a dense computation written here,
through the float64 stand-in tests/fake_custom_mm_block_select_tiles.py; the operands handed to the bindings uncopied; and the
ten new entries of the C ABI: declared, exported, MI_EINVAL before any HIP call — one fault a row, with made-up addresses that
nothing may dereference (every row is a refusal or an empty call), as in test_kv_cache_read_entries_host.py."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_kv_cache_entries_host import CACHE, EINVAL, ERANGE, FAULTS, FP8, I32, I64, LENS, OK, PAGED, PTR, SCALES, SIZES, STREAM, TABLE, VP, WIDTH
from test_kv_cache_read_entries_host import ALL, BOTH_PREFILL, LAYOUT, OUT, PREFILL, REFUSALS, read_valid

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
NAN = float("nan")
F32 = ctypes.c_float

LISTS_ENTRIES = [(f"mi_block_attention_lists_prefill{p}{f}_{t}", bool(p), bool(f))
                 for p in ("", "_paged") for f in ("", "_fp8") for t in SUFFIXES]
SELECT_ENTRIES = [f"mi_block_select_tiles_{t}" for t in SUFFIXES]


# ---- the C ABI -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    return ctypes.CDLL(str(built / "libmi_spmm.so"))


def test_header_declares_and_library_exports_the_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in [e[0] for e in LISTS_ENTRIES] + SELECT_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
    assert len(LISTS_ENTRIES) == 8


def lists_signature(paged, fp8):
    """The parameter list of a prefill-over-lists entry, in the header's order: the prefill entries' with the lists as the head."""
    table, scales = (TABLE if paged else []), (SCALES if fp8 else [])
    return ([("block_ids", VP), ("block_counts", VP), ("K", I32)] + SIZES + table + WIDTH +
            [("q", VP), ("ldq", I64), ("headQ", I64), ("batchQ", I64)] + CACHE + LENS +
            [("new_lens", VP), ("new_lens_count", I32), ("group", I32), ("scale", F32)] + scales + OUT + STREAM)


# what the lists add to the reading entries' refusals: one fault a row
LISTS_REFUSALS = [
    ("K 0", dict(K=0), EINVAL),
    ("K -1", dict(K=-1), EINVAL),
    ("null block_ids", dict(block_ids=None), EINVAL),
    ("null block_counts", dict(block_counts=None), EINVAL),
    ("block_ids off by 2 bytes", dict(block_ids=PTR + 2), EINVAL),
    ("block_counts off by 2 bytes", dict(block_counts=PTR + 2), EINVAL),
    ("items · X · K = 2^31", dict(items=2 ** 15, T=64, K=2 ** 15), ERANGE),   # X = 2 tiles
    ("K 0 + items 0", dict(K=0, items=0), EINVAL),
]


def lists_rows(paged, fp8):
    """(title, arguments, status): the cache faults, the prefill entries' refusals that are not about the layout, the lists' own."""
    for title, where, change, status in FAULTS:
        if (where == PAGED and not paged) or (where == FP8 and not fp8) or isinstance(status, dict):
            continue
        yield title, {**read_valid(paged), **change}, status
    for title, families, where, change, status in REFUSALS:
        if PREFILL not in families or families == LAYOUT or (where == PAGED and not paged) or (where == FP8 and not fp8):
            continue
        assert families in (ALL, BOTH_PREFILL), title
        yield title, {**read_valid(paged), **change}, status.get(PREFILL) if isinstance(status, dict) else status
    for title, change, status in LISTS_REFUSALS:
        yield title, {**read_valid(paged), **change}, status


@pytest.mark.parametrize("name,paged,fp8", LISTS_ENTRIES, ids=[e[0] for e in LISTS_ENTRIES])
def test_lists_entries_refuse_before_any_hip_call(lib, name, paged, fp8):
    sig = lists_signature(paged, fp8)
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = [t for _, t in sig], ctypes.c_int
    sent = 0
    for title, args, expect in lists_rows(paged, fp8):
        assert expect in (EINVAL, ERANGE) or (expect == OK and (args["items"] == 0 or args["T"] == 0)), f"{name}, {title}: no row is a valid call"
        got = fn(*[args[n] for n, _ in sig])
        assert got == expect, f"{name}, {title}: status {got}, expected {expect}"
        sent += 1
    assert sent >= 35


@pytest.mark.parametrize("s", SUFFIXES)
def test_select_tiles_entry_validates_before_any_hip_call(lib, s):
    base = dict(items=8, heads=2, T=100, Smax=512, D=64, group=4, q=PTR, ldq=64, headQ=64, batchQ=8 * 64, bounds=PTR, lens=PTR,
                lens_count=4, new_lens=None, new_lens_count=0, K=4, sink=1, local=2, ids=PTR, counts=PTR, scores=None)
    fn = getattr(lib, f"mi_block_select_tiles_{s}")
    fn.argtypes, fn.restype = 6 * [I32] + [VP, I64, I64, I64, VP, VP, I32, VP, I32] + 3 * [I32] + 4 * [VP], ctypes.c_int

    def select(**kw):
        a = {**base, **kw}
        return fn(a["items"], a["heads"], a["T"], a["Smax"], a["D"], a["group"], a["q"], a["ldq"], a["headQ"], a["batchQ"], a["bounds"],
                  a["lens"], a["lens_count"], a["new_lens"], a["new_lens_count"], a["K"], a["sink"], a["local"], a["ids"], a["counts"],
                  a["scores"], None)

    cap = lib.mi_block_select_max_blocks()
    for kw in ({"K": 0}, {"K": -1}, {"sink": -1}, {"local": 0}, {"sink": 2, "local": 3}, {"K": 2}, {"group": 0}, {"group": 17},
               {"D": 48}, {"Smax": 500}, {"Smax": (cap + 1) * 64}, {"items": 65536}, {"heads": 3}, {"heads": 0}, {"lens_count": 3},
               {"lens": None}, {"lens": PTR + 2}, {"ids": None}, {"ids": PTR + 2}, {"counts": None}, {"counts": PTR + 1},
               {"scores": PTR + 2}, {"q": None}, {"q": PTR + 8}, {"ldq": 60}, {"headQ": 4}, {"batchQ": 12}, {"bounds": None},
               {"bounds": PTR + 8}, {"T": -1}, {"new_lens": PTR + 2, "new_lens_count": 1}, {"new_lens": PTR, "new_lens_count": 2},
               {"new_lens": PTR, "new_lens_count": 0}, {"new_lens": PTR, "new_lens_count": 8}):
        assert select(**kw) == EINVAL, kw
    assert select(items=0, q=None) == OK and select(T=0, lens=None) == OK
    assert select(items=0, K=0) == EINVAL and select(T=0, sink=3, local=2) == EINVAL


# ---- matmuls on the real extension: refusals before the device ---------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def test_takes_and_tiles(real):
    for dtype in (torch.bfloat16, torch.float16):
        for D in (32, 64, 96, 128):
            assert real.select_key_blocks_tiles_takes(dtype, D, 1, 0) and real.select_key_blocks_tiles_takes(dtype, D, 16, 16384)
            assert real.block_attention_prefill_selected_takes(dtype, D) and real.block_attention_prefill_selected_fp8_takes(dtype, D)
            assert real.block_attention_prefill_selected_paged_takes(dtype, D, 16) and real.block_attention_prefill_selected_paged_fp8_takes(dtype, D, 128)
    assert not real.select_key_blocks_tiles_takes(torch.float16, 64, 17, 8) and not real.select_key_blocks_tiles_takes(torch.float16, 64, 0, 8)
    assert not real.select_key_blocks_tiles_takes(torch.float16, 64, 4, 16385) and not real.select_key_blocks_tiles_takes(torch.float32, 64, 4, 8)
    assert not real.select_key_blocks_tiles_takes(torch.float16, 48, 4, 8) and not real.select_key_blocks_tiles_takes(torch.float16, 64, True, 8)
    assert not real.block_attention_prefill_selected_takes(torch.float32, 64) and not real.block_attention_prefill_selected_takes(torch.float16, 48)
    assert not real.block_attention_prefill_selected_paged_takes(torch.float16, 64, 8) and not real.block_attention_prefill_selected_paged_fp8_takes(torch.float16, 64, 24)
    assert [real.block_attention_prefill_tiles(T) for T in (1, 60, 64, 65, 100, 128, 130, 2048)] == [2, 2, 2, 3, 3, 3, 4, 33]
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="block_attention_prefill_tiles: T must be an int >= 1"):
            real.block_attention_prefill_tiles(bad)


def test_select_tiles_refusals_come_before_the_device_with_their_type(real):
    f = real.select_key_blocks_tiles
    what = "select_key_blocks_tiles: "
    q, bounds, lens = torch.rand(2, 8, 100, 64).bfloat16(), torch.rand(2, 2, 4, 2, 64).bfloat16(), torch.tensor([100, 256])
    for K, kw, msg in ((0, {}, "K must be a positive int32"), (-3, {}, "K must be a positive int32"), (2 ** 31, {}, "K must be a positive int32"),
                       (4, {"sink": -1}, "sink must be >= 0"), (4, {"local": 0}, "local must be >= 1"),
                       (2, {}, "sink \\+ local = 3 forced blocks do not fit K = 2"), (4, {"sink": 3}, "sink \\+ local = 5 forced blocks do not fit K = 4"),
                       (4.0, {}, "K must be an int"), (True, {}, "K must be an int"), (4, {"sink": 1.0}, "sink must be an int"),
                       (4, {"local": None}, "local must be an int")):
        with pytest.raises(ValueError, match=what + msg):
            f(q, bounds, lens, K, **kw)
    with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16"):
        f(q.float(), bounds, lens, 4)
    with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but bounds is torch.float16"):
        f(q, bounds.half(), lens, 4)
    with pytest.raises(ValueError, match=what + r"q must be \[B, Hq, T, D\] and bounds \[B, Hkv, Smax/64, 2, D\]"):
        f(q, bounds[0], lens, 4)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(q[..., :48], bounds[..., :48], lens, 4)
    for bad in (torch.rand(3, 2, 4, 2, 64), torch.rand(2, 3, 4, 2, 64), torch.rand(2, 2, 4, 3, 64), torch.rand(2, 2, 4, 2, 32),
                torch.rand(2, 0, 4, 2, 64), bounds.repeat(1, 1, 2, 1, 1)[:, :, ::2]):
        with pytest.raises(ValueError, match=what + r"q of shape \(2, 8, 100, 64\) needs contiguous bounds"):
            f(q, bad.bfloat16() if bad.is_contiguous() else bad, lens, 4)
    with pytest.raises(ValueError, match=what + "34 query heads over 2 k / v heads is a group of 17"):
        f(torch.rand(2, 34, 1, 64).bfloat16(), bounds, lens, 4)
    with pytest.raises(ValueError, match=what + "q must hold T >= 1 new tokens"):
        f(q[:, :, :0], bounds, lens, 4)
    with pytest.raises(ValueError, match=what + "16385 blocks per item exceed the 16384"):
        f(torch.rand(1, 1, 1, 32).bfloat16(), torch.empty(1, 1, 16385, 2, 32).bfloat16(), torch.tensor(5), 4)
    with pytest.raises(ValueError, match=what + "k_lens is required"):
        f(q, bounds, None, 4)
    with pytest.raises(ValueError, match=what + "new_lens must be an int32 or int64 tensor"):
        f(q, bounds, lens, 4, new_lens=torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match=what + r"new_lens must have shape \(2,\)"):
        f(q, bounds, lens, 4, new_lens=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match=what + "new_lens must be None or a dense tensor"):
        f(q, bounds, lens, 4, new_lens=[1, 2])
    with pytest.raises(ValueError, match=what + "q's head stride must be a multiple of 8 elements"):
        f(torch.rand(2, 8 * 68).bfloat16().as_strided((2, 8, 1, 64), (8 * 68, 68, 64, 1)), bounds, lens, 4)
    with pytest.raises(TypeError):  # keyword only
        f(q, bounds, lens, 4, 1, 2)
    with pytest.raises(RuntimeError, match=what + r"q, bounds, k_lens must be device \(HIP\) tensors"):
        f(q, bounds, lens, 4)
    with pytest.raises(RuntimeError, match=what + r"q, bounds, k_lens, new_lens must be device \(HIP\) tensors"):  # a strided q is taken
        f(torch.rand(2, 100, 8, 64).bfloat16().transpose(1, 2), bounds, torch.tensor(3), 9, sink=0, local=1, new_lens=torch.tensor([3, 0]),
          return_scores=True)


def test_prefill_selected_refusals_come_before_the_device_with_their_type(real):
    f, fp = real.block_sparse_attention_prefill_selected, real.block_sparse_attention_prefill_selected_paged
    what = "block_sparse_attention_prefill_selected: "
    q, k, lens = torch.rand(2, 8, 100, 64).bfloat16(), torch.rand(2, 2, 256, 64).bfloat16(), torch.tensor([100, 256])
    ids, counts = torch.zeros(2, 2, 3, 4, dtype=torch.int32), torch.ones(2, 2, 3, dtype=torch.int32)
    for bad in (ids.long(), ids.float(), None, ids.tolist()):
        with pytest.raises(ValueError, match=what + "block_ids must be a dense int32 tensor"):
            f(q, k, k, bad, counts, lens)
    with pytest.raises(ValueError, match=what + "block_counts must be a dense int32 tensor"):
        f(q, k, k, ids, counts.long(), lens)
    for bad in (ids[0], ids[:, :1], torch.zeros(2, 2, 100, 4, dtype=torch.int32), ids[..., :0], torch.zeros(2, 2, 3, 8, dtype=torch.int32)[..., ::2]):
        with pytest.raises(ValueError, match=what + r"block_ids must be a contiguous \[B, Hkv, ceil\(T/64\) \+ 1, K\] = \[2, 2, 3, K >= 1\]"):
            f(q, k, k, bad, counts, lens)
    for bad in (counts[0], torch.ones(2, 2, 100, dtype=torch.int32), torch.ones(2, 2, 6, dtype=torch.int32)[..., ::2]):
        with pytest.raises(ValueError, match=what + r"block_counts must be a contiguous \[B, Hkv, ceil\(T/64\) \+ 1\] = \[2, 2, 3\]"):
            f(q, k, k, ids, bad, lens)
    with pytest.raises(ValueError, match=what + "q must be bfloat16 or float16"):
        f(q.float(), k, k, ids, counts, lens)
    with pytest.raises(RuntimeError, match=what + "q is torch.bfloat16 but v is torch.float16"):
        f(q, k, k.half(), ids, counts, lens)
    with pytest.raises(ValueError, match=what + "head size D must be 32, 64, 96 or 128, got 48"):
        f(q[..., :48], k[..., :48], k[..., :48], ids, counts, lens)
    with pytest.raises(ValueError, match=what + r"q of shape \(2, 8, 100, 64\) needs k \(2, 'Hkv', 'Smax', 64\) with Hkv a divisor of 8"):
        f(q, torch.rand(2, 3, 256, 64).bfloat16(), k, ids, counts, lens)
    with pytest.raises(ValueError, match=what + "v must be a dense tensor with k's shape"):
        f(q, k, k[:, :, :128], ids, counts, lens)
    with pytest.raises(ValueError, match=what + "Smax = 200 must be a multiple of 64"):
        f(q, k[:, :, :200], k[:, :, :200], ids, counts, lens)
    with pytest.raises(ValueError, match=what + "k's row stride must be a multiple of 8 elements and at least D = 64, got 68"):
        f(q, torch.rand(2, 2, 256, 68).bfloat16()[..., :64], k, ids, counts, lens)
    with pytest.raises(ValueError, match=what + r"k_lens must have shape \(2,\)"):
        f(q, k, k, ids, counts, torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match=what + r"new_lens must have shape \(2,\)"):
        f(q, k, k, ids, counts, lens, new_lens=torch.tensor([1]))
    with pytest.raises(ValueError, match=what + "q's head stride must be a multiple of 8 elements"):
        f(torch.rand(2, 8 * 68).bfloat16().as_strided((2, 8, 1, 64), (8 * 68, 68, 64, 1)), k, k, ids[:, :, :2].contiguous(),
          counts[:, :, :2].contiguous(), lens)
    with pytest.raises(TypeError):  # no split: a list has K entries
        f(q, k, k, ids, counts, lens, split=4)
    with pytest.raises(RuntimeError, match=what + r"q, k, v, block_ids, block_counts, k_lens must be device \(HIP\) tensors"):
        f(q, k, k, ids, counts, lens)
    # a group of 17 is taken (any G ≥ 1), as is a strided q
    with pytest.raises(RuntimeError, match=what + r"q, k, v, block_ids, block_counts, k_lens, new_lens must be device"):
        f(torch.rand(2, 100, 34, 64).bfloat16().transpose(1, 2), k, k, ids, counts, lens, new_lens=torch.tensor([5, 0]))
    what = "block_sparse_attention_prefill_selected_paged: "
    pool, table = torch.rand(20, 2, 16, 64).bfloat16(), torch.arange(32, dtype=torch.int32).reshape(2, 16) % 20
    with pytest.raises(ValueError, match=what + "the pool's pages must hold a power of two >= 16 keys, got page = 24"):
        pp = torch.rand(20, 2, 24, 64).bfloat16()
        fp(q, pp, pp, table, ids, counts, lens)
    with pytest.raises(ValueError, match=what + "Smax = 240 must be a multiple of 64"):
        fp(q, pool, pool, table[:, :15], ids, counts, lens)
    with pytest.raises(RuntimeError, match=what + r"q, k_pages, v_pages, block_table, block_ids, block_counts, k_lens must be device"):
        fp(q, pool, pool, table, ids, counts, lens)
    what = "block_sparse_attention_prefill_selected_fp8: "
    k8 = torch.zeros(2, 2, 256, 64).to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match=what):
        real.block_sparse_attention_prefill_selected_fp8(q, k, k, ids, counts, lens)  # a 2-byte cache
    with pytest.raises(RuntimeError, match=what + r"q, k, v, block_ids, block_counts, k_lens must be device"):
        real.block_sparse_attention_prefill_selected_fp8(q, k8, k8, ids, counts, lens, k_scale=0.5)


def test_bindings_refuse_host_tensors_and_keywords(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    q, k = torch.rand(1, 2, 1, 32).bfloat16(), torch.rand(1, 1, 64, 32).bfloat16()
    lens, lse = torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 1)
    bounds = torch.empty(1, 1, 1, 2, 32).bfloat16()
    ids, counts = torch.zeros(1, 1, 2, 2, dtype=torch.int32), torch.ones(1, 1, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_select_tiles(q, bounds, lens, None, 2, 0, 1, ids, counts, None)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_lists_prefill(ids, counts, q, k, k, lens, None, 1.0, torch.empty_like(q), lse)
    with pytest.raises(TypeError):  # positional only
        custom_mm.block_select_tiles(q, bounds, lens, None, K=2, sink=0, local=1, block_ids=ids, block_counts=counts, scores=None)
    for name in ("block_attention_lists_prefill_paged", "block_attention_lists_prefill_fp8", "block_attention_lists_prefill_paged_fp8"):
        assert callable(getattr(custom_mm, name))


# ---- wiring on CPU tensors, float64 stand-in arithmetic ----------------------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_select_tiles as fake
    saved = {k: sys.modules.get(k) for k in ("custom_mm", "matmuls")}
    sys.modules["custom_mm"] = fake
    sys.modules.pop("matmuls", None)
    matmuls = importlib.import_module("matmuls")
    fake.calls.clear()
    yield matmuls, fake
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def _tile_reference(q, bounds, lens, new_lens, K, sink, local):
    """The contract, written out densely in float64, token by token and block by block: tiles from positions, candidates J ≤ r,
    the Quest sum Σ_d max(q·lo, q·hi) per (token, head), the max over both, forced blocks, the order, −1s."""
    B, Hq, T, D = q.shape
    Hkv, blocks = bounds.shape[1], bounds.shape[2]
    G, X = Hq // Hkv, -(-T // 64) + 1
    ids, counts = np.full((B, Hkv, X, K), -1, np.int64), np.zeros((B, Hkv, X), np.int64)
    scores = np.full((B, Hkv, X, blocks), -np.inf)
    for b in range(B):
        klen = min(max(int(lens[b]), 0), blocks * 64)
        new = T if new_lens is None else min(max(int(new_lens[b]), 0), T)
        base = (klen - T) // 64
        for t in range(T):
            pos = klen - T + t
            if pos < 0 or t < T - new:
                continue
            r = pos // 64
            x = r - base
            assert 0 <= x < X and r < blocks
            for h in range(Hkv):
                for J in range(r + 1):
                    lo, hi = bounds[b, h, J, 0].double(), bounds[b, h, J, 1].double()
                    s = max(float(torch.maximum(q[b, h * G + g, t].double() * lo, q[b, h * G + g, t].double() * hi).sum()) for g in range(G))
                    scores[b, h, x, J] = max(scores[b, h, x, J], s)
        for x in range(X):
            r = base + x
            for h in range(Hkv):
                if not np.isfinite(scores[b, h, x]).any():
                    continue
                cand = list(range(r + 1))
                forced = {J for J in cand if J < sink} | {J for J in cand if J > r - local}
                rest = sorted((J for J in cand if J not in forced), key=lambda J: (-scores[b, h, x, J], J))
                n = min(K, len(cand))
                chosen = sorted(forced | set(rest[:n - len(forced)]))
                assert len(chosen) == n
                ids[b, h, x, :n], counts[b, h, x] = chosen, n
    return ids, counts, scores


@pytest.mark.parametrize("T", [1, 60, 64, 100, 130])
def test_tile_rules_and_operands_uncopied(mm, T):
    """Integer operands: the float64 stand-in and the dense computation agree exactly.  k_lens no multiples of 64, an item
    shorter than the chunk (slots with pos < 0), new_lens with a 0 (an item without a token) and a partial one."""
    matmuls, fake = mm
    g = torch.Generator().manual_seed(11 + T)
    B, Hkv, G, D, blocks = 3, 2, 3, 32, 12
    q = torch.randint(-4, 5, (B, T, Hkv * G, D), generator=g).half().transpose(1, 2)   # [B, Hq, T, D] through its own strides
    lo = torch.randint(-8, 9, (B, Hkv, blocks, D), generator=g)
    hi = lo + torch.randint(0, 4, (B, Hkv, blocks, D), generator=g)
    bounds = torch.stack([lo, hi], 3).half()
    lens = torch.tensor([T // 2 + 1, 450, 707])
    for b, n in enumerate(lens.tolist()):
        bounds[b, :, (n - 1) // 64 + 1:] = NAN     # bounds of non-candidates are never read
    for new_lens in (None, torch.tensor([T, 0, (T + 1) // 2])):
        for K, sink, local in ((3, 1, 2), (4, 0, 1), (5, 2, 1), (14, 1, 2)):
            ids, counts, scores = matmuls.select_key_blocks_tiles(q, bounds, lens, K, sink=sink, local=local, new_lens=new_lens,
                                                                  return_scores=True)
            name, call = fake.calls[-1]
            assert name == "block_select_tiles" and call["q_ptr"] == q.data_ptr() and call["q_stride"] == tuple(q.stride())
            assert call["bounds_ptr"] == bounds.data_ptr() and (call["K"], call["sink"], call["local"]) == (K, sink, local)
            assert (call["new_lens"] is None) == (new_lens is None) and call["new_lens_dtype"] in (None, torch.int32)
            r_ids, r_counts, r_scores = _tile_reference(q, bounds, lens, new_lens, K, sink, local)
            assert tuple(ids.shape) == (B, Hkv, matmuls.block_attention_prefill_tiles(T), K) and ids.dtype == torch.int32
            assert np.array_equal(ids.numpy(), r_ids) and np.array_equal(counts.numpy(), r_counts), (T, K, sink, local)
            assert np.array_equal(scores.numpy().astype(np.float64), r_scores)
            if new_lens is not None:
                assert counts[1].eq(0).all() and ids[1].eq(-1).all()                # an item without a token
    two = matmuls.select_key_blocks_tiles(q, bounds, lens, 3)
    assert len(two) == 2 and not fake.calls[-1][1]["scores"]
