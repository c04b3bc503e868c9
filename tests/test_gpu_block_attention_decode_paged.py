"""matmuls.block_sparse_attention_decode_paged on the MI355X: the decode call of §3.18 over a pool of
pages [P, Hkv, page, D] and a block table [B, W].  The contract is on bits: for a pool and a table whose seen entries are in
range, out and lse are those of block_sparse_attention_decode with the same chunk on the cache gathered here to
[B, Hkv, Smax, D] — whatever P, the placement of the pages and the page size.  Beside it the project's rule e_dev ≤ 8 · e_ref
against dense masked attention in float64 (the helpers of tests/test_gpu_block_attention_decode.py), which is what pins the
invisible keys of an out-of-range table entry.

Smax = 512, B · Hkv ≤ 8, chunk=2 unless stated.  Pools: P = B · W + 3 pages, the logical → physical map a seeded
permutation (physical neighbours are not logical neighbours), unreferenced pages NaN.  Long lists (64 entries: the tiles of
the in-loop look-ahead, holes met in a wave's third turn and later) live in tests/test_gpu_block_attention_decode_long.py."""
import ctypes

import pytest
import torch

from gpu_helpers import SENTINEL, assert_outside_untouched, assert_same_bits, padded
from test_gpu_block_attention_decode import (ROWS, SMAX, check_rule, layout_from_rows, lens_tensor, operands, poison_unseen,
                                             visible)

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAGES = [16, 32, 64, 128, 256]
WIDTHS = [32, 64, 96, 128]


def fresh_table(B, W, P, seed, dev):
    """int32 [B, W]: distinct pool pages under a seeded permutation of the P pages."""
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))
    return perm[:B * W].reshape(B, W).to(torch.int32).to(dev)


def scatter(pool, table, x):
    """Writes the cache x [B, Hkv, Smax, D] into the pool [P, Hkv, page, D] (any strides) at the table's pages."""
    B, Hkv, smax, D = x.shape
    page = pool.shape[2]
    W = smax // page
    pool[table.long().reshape(-1)] = x.reshape(B, Hkv, W, page, D).permute(0, 2, 1, 3, 4).reshape(B * W, Hkv, page, D)


def paged(k, v, page, seed, extra=3):
    """(k_pages, v_pages, table) holding k, v [B, Hkv, Smax, D]: P = B · W + extra, unreferenced pages NaN."""
    B, Hkv, smax, D = k.shape
    W = smax // page
    P = B * W + extra
    table = fresh_table(B, W, P, seed, k.device)
    pools = []
    for x in (k, v):
        pool = torch.full((P, Hkv, page, D), NAN, device=x.device, dtype=x.dtype)
        scatter(pool, table, x)
        pools.append(pool)
    return pools[0], pools[1], table


def gathered(pool, table):
    """The test's own contiguous cache [B, Hkv, Smax, D] of a pool and a table; the keys of an entry outside the pool: zeros."""
    B, W = table.shape
    P, Hkv, page, D = pool.shape
    valid = (table >= 0) & (table < P)
    pages = pool[table.long().clamp(0, max(P - 1, 0)).reshape(-1)].reshape(B, W, Hkv, page, D)
    pages = torch.where(valid[:, :, None, None, None], pages, torch.zeros((), device=pool.device, dtype=pool.dtype))
    return pages.permute(0, 2, 1, 3, 4).reshape(B, Hkv, W * page, D).contiguous()


def same_as_contiguous(mm, what, q, kp, vp, table, layout, lens, **kw):
    """The paged call; asserts the bits of the contiguous call on the gathered cache; returns (out, lse)."""
    out, lse = mm.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens, return_lse=True, **kw)
    want = mm.block_sparse_attention_decode(q, gathered(kp, table), gathered(vp, table), layout, lens, return_lse=True, **kw)
    assert not out.requires_grad
    assert_same_bits(out, want[0], f"{what}: the paged call against the contiguous call on the gathered cache")
    assert_same_bits(lse, want[1], f"{what}: lse")
    return out, lse


# ---- 1. bit equality with the contiguous call: every page size, every D, both dtypes ---------------------------------------

@pytest.mark.parametrize("page,D,dtype", [(page, D, (torch.bfloat16, torch.float16)[(i + j) % 2])
                                          for i, page in enumerate(PAGES) for j, D in enumerate(WIDTHS)])
def test_1_the_bits_of_the_contiguous_call(mm, dev, page, D, dtype):
    """pos = 511: the 8-entry list in four chunks of two; pos = 199: three entries and two empty trailing chunks (test 1 of
    the contiguous file).  Pages of 16 and 32 keys: a tile spans 4 and 2 pages; 64: one; 128 and 256: a part of one."""
    B, Hkv, G, T, k_lens = 2, 2, 4, 1, [512, 200]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 600 + D + page)
    kp, vp, table = paged(k, v, page, 601 + page)
    assert torch.equal(gathered(kp, table), k)
    out, lse = same_as_contiguous(mm, f"page {page} D={D} {dtype}", q, kp, vp, table, layout, lens_tensor(k_lens, dev), chunk=2)
    check_rule(f"paged form page={page} {dtype} D={D}", out, q, k, v, visible([ROWS], B, Hkv, T, k_lens), G, lse)


# ---- 2. nothing outside is read ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [16, 128])
@pytest.mark.parametrize("form", ["PHSD", "PSHD"])
def test_2_nothing_outside_is_read(mm, dev, form, page):
    """NaN in every unreferenced page, in every key no token sees and between the rows (row stride D + 8 in a buffer of
    NaN), for [P, Hkv, page, D] and the transposed view of [P, page, Hkv, D]; the table entries of logical pages wholly
    beyond pos are −1 and P + 5: finite, under the rule, the bits of the call on contiguous pools; no copy."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 2, 64, torch.float16, [130, 449]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 641 + page)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    W = SMAX // page
    P = B * W + 3
    table = fresh_table(B, W, P, 642 + page, dev)

    def strided(x):
        shape = (P, Hkv, page, D + 8) if form == "PHSD" else (P, page, Hkv, D + 8)
        buf = torch.full(shape, NAN, device=dev, dtype=dtype)
        view = buf[..., :D] if form == "PHSD" else buf[..., :D].transpose(1, 2)
        scatter(view, table, poison_unseen(x, vis))
        return view

    ks, vs = strided(k), strided(v)
    assert not ks.is_contiguous() and ks.stride(2) > D and ks.shape == (P, Hkv, page, D)
    beyond = [(b, lp) for b in range(B) for lp in range(W) if lp * page > k_lens[b] - 1]
    assert len(beyond) >= 2
    for i, (b, lp) in enumerate(beyond):
        table[b, lp] = (-1, P + 5)[i % 2]
    lens = lens_tensor(k_lens, dev)
    ptrs = (ks.data_ptr(), vs.data_ptr(), table.data_ptr())
    out, lse = mm.block_sparse_attention_decode_paged(q, ks, vs, table, layout, lens, chunk=2, return_lse=True)
    assert (ks.data_ptr(), vs.data_ptr(), table.data_ptr()) == ptrs
    check_rule(f"poisoned {form} pool, page {page}", out, q, k, v, vis, G, lse)
    clone = mm.block_sparse_attention_decode_paged(q, ks.contiguous(), vs.contiguous(), table, layout, lens, chunk=2, return_lse=True)
    assert_same_bits(out, clone[0], f"{form}: the strided pool against its contiguous clone")
    assert_same_bits(lse, clone[1], f"{form}: lse")


# ---- 3. invalid entries hide their keys -------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [16, 64])
def test_3_invalid_entries_hide_their_keys(mm, dev, page):
    """One seen logical page per item carries −1, another P (the first value past the pool); the pages they named before are
    NaN now.  The result is under the rule with those keys removed from the mask; the item whose entries are all invalid
    gives zero rows and lse −inf."""
    B, Hkv, G, T, D, dtype, k_lens = 3, 2, 4, 2, 64, torch.bfloat16, [512, 200, 300]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 661 + page)
    kp, vp, table = paged(k, v, page, 662 + page)
    P = kp.shape[0]
    vis = visible([ROWS], B, Hkv, T, k_lens)
    hidden = [(0, 100 // page, -1), (0, 400 // page, P), (1, 70 // page, P), (1, 195 // page, -1)]  # (item, logical page, entry)
    for b, lp, entry in hidden:
        assert vis[b, :, :, lp * page:(lp + 1) * page].any(), "a page with seen keys"
        kp[int(table[b, lp])] = NAN
        vp[int(table[b, lp])] = NAN
        table[b, lp] = entry
        vis[b, :, :, lp * page:(lp + 1) * page] = False
    table[2] = torch.tensor([-1, P, P + 7, -2 ** 31] * (table.shape[1] // 4), dtype=torch.int32, device=dev)
    vis[2] = False
    out, lse = mm.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens_tensor(k_lens, dev), chunk=2, return_lse=True)
    check_rule(f"hidden pages, page {page}", out, q, k, v, vis, G, lse)
    assert (out[2] == 0).all() and (lse[2] == -float("inf")).all() and torch.isfinite(lse[:2]).all()
    # an empty pool: every entry is invalid
    out, lse = mm.block_sparse_attention_decode_paged(q, kp[:0], vp[:0], table, layout, lens_tensor(k_lens, dev), chunk=2, return_lse=True)
    assert (out == 0).all() and (lse == -float("inf")).all()


# ---- 4. shared pages and independence -----------------------------------------------------------------------------------------

def test_4_two_items_share_the_pages_of_a_common_prefix(mm, dev):
    B, Hkv, G, T, D, dtype, page, k_lens = 2, 2, 4, 1, 96, torch.float16, 32, [512, 333]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 671)
    k[1, :, :128], v[1, :, :128] = k[0, :, :128], v[0, :, :128]
    kp, vp, table = paged(k, v, page, 672)
    shared = 128 // page
    for b_lp in range(shared):  # item 1's own copies of the prefix are dropped: it reads item 0's pages
        kp[int(table[1, b_lp])] = NAN
        vp[int(table[1, b_lp])] = NAN
    table[1, :shared] = table[0, :shared]
    assert torch.equal(gathered(kp, table), k)
    out, lse = same_as_contiguous(mm, "a shared prefix", q, kp, vp, table, layout, lens_tensor(k_lens, dev), chunk=2)
    check_rule("a shared prefix", out, q, k, v, visible([ROWS], B, Hkv, T, k_lens), G, lse)


def test_4_an_item_of_a_batch_is_the_call_on_it_alone(mm, dev):
    """… its table row a [1, W] slice or a slice of a wider table; an int64 table; a pool that grew."""
    B, Hkv, G, T, D, dtype, page, k_lens = 6, 1, 4, 2, 128, torch.bfloat16, 16, [512, 65, 300, 1, 129, 448]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 681)
    kp, vp, table = paged(k, v, page, 682)
    W, P = table.shape[1], kp.shape[0]
    lens = lens_tensor(k_lens, dev)
    out, lse = same_as_contiguous(mm, "batch of 6", q, kp, vp, table, layout, lens, chunk=2)
    wider = torch.full((B, W + 5), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    wider[:, :W] = table
    for b in range(B):
        for what, row in (("a [1, W] slice", table[b:b + 1]), ("a strided slice", wider[b:b + 1, :W])):
            one = mm.block_sparse_attention_decode_paged(q[b:b + 1], kp, vp, row, layout, lens[b:b + 1], chunk=2, return_lse=True)
            assert_same_bits(out[b:b + 1], one[0], f"item {b} alone, its table row {what}")
            assert_same_bits(lse[b:b + 1], one[1], f"item {b} alone, its table row {what}: lse")
    whole = mm.block_sparse_attention_decode_paged(q, kp, vp, wider[:, :W], layout, lens, chunk=2)
    assert_same_bits(whole, out, "the table as a slice of a wider one")
    long_table = mm.block_sparse_attention_decode_paged(q, kp, vp, table.long(), layout, lens, chunk=2, return_lse=True)
    assert_same_bits(long_table[0], out, "an int64 table")
    assert_same_bits(long_table[1], lse, "an int64 table: lse")
    grown = [torch.cat([x, torch.full((11,) + tuple(x.shape[1:]), NAN, device=dev, dtype=dtype)]) for x in (kp, vp)]
    bigger = mm.block_sparse_attention_decode_paged(q, grown[0], grown[1], table, layout, lens, chunk=2, return_lse=True)
    assert grown[0].shape[0] == P + 11
    assert_same_bits(bigger[0], out, "a pool that grew")
    assert_same_bits(bigger[1], lse, "a pool that grew: lse")


# ---- 5. groups and tokens across boundaries ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 5, 16])
def test_5_group_sizes_and_three_tokens_across_page_tile_and_row_boundaries(mm, dev, G):
    """k_lens 1, 64, 65, 130, 512, 0 with T = 3 over pages of 16 keys: tokens that do not exist, tokens on both sides of a
    page, a 64-tile and a layout row."""
    B, Hkv, T, D, dtype, page, k_lens = 6, 1, 3, 64, torch.bfloat16, 16, [1, 64, 65, 130, 512, 0]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 690 + G)
    kp, vp, table = paged(k, v, page, 691 + G)
    out, lse = same_as_contiguous(mm, f"G={G} T=3", q, kp, vp, table, layout, lens_tensor(k_lens, dev, torch.int64), chunk=2)
    check_rule(f"paged G={G} T=3", out, q, k, v, visible([ROWS], B, Hkv, T, k_lens), G, lse)
    assert (out[5] == 0).all() and (lse[5] == -float("inf")).all()
    assert_same_bits(out[0, :, 2], v[0, 0, 0].expand(G, D), "one visible key: its value row")


# ---- 6. the split ---------------------------------------------------------------------------------------------------------------

def test_6_every_chunk_size_the_default_and_block_128(mm, dev):
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 3, 128, torch.bfloat16, [512, 258]
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 701)
    lens = lens_tensor(k_lens, dev)
    kp, vp, table = paged(k, v, 16, 702)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    for chunk in (1, 3, 8):  # 8 is one chunk: the walk stores out itself, no combine launch
        out, lse = same_as_contiguous(mm, f"chunk={chunk}", q, kp, vp, table, layout, lens, chunk=chunk)
        check_rule(f"paged chunk={chunk}", out, q, k, v, vis, G, lse)
    default = mm.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens)
    assert_same_bits(default, mm.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens, chunk=mm._decode_chunk(SMAX, D)),
                     "chunk=None")
    assert_same_bits(default, mm.block_sparse_attention_decode(q, k, v, layout, lens), "chunk=None against the contiguous call")
    rows128 = [[0], [1, 0], [0, 2, 1], [2, 3, 0]]
    expanded = [[x for c in rows128[i // 2] for x in (2 * c, 2 * c + 1)] for i in range(8)]  # sub-block order
    kp, vp, table = paged(k, v, 128, 703)
    coarse = mm.block_sparse_attention_decode_paged(q, kp, vp, table, layout_from_rows(rows128, dev), lens, block=128, chunk=2, return_lse=True)
    fine = same_as_contiguous(mm, "the expanded layout", q, kp, vp, table, layout_from_rows(expanded, dev), lens, block=64, chunk=2)
    assert_same_bits(coarse[0], fine[0], "block = 128 against the expanded layout")
    assert_same_bits(coarse[1], fine[1], "block = 128 against the expanded layout: lse")
    check_rule("paged block = 128", coarse[0], q, k, v, visible([rows128], B, Hkv, T, k_lens, block=128), G, coarse[1])


# ---- 7. graph capture while pages are allocated ----------------------------------------------------------------------------------

def test_7_one_graph_replayed_while_pages_are_allocated(mm, dev):
    """One capture over pages of 16 keys.  Before every replay k_lens is incremented in place, the new key / value row is
    written into the pool, and when a length crosses into a new logical page (16 → 17 for item 0, 64 → 65 for item 1) the
    table slot is written in place from −1 to a fresh pool page: the replay has the bits of the eager paged call and of the
    contiguous call on the gathered state."""
    B, Hkv, G, T, D, dtype, page = 2, 2, 4, 1, 64, torch.float16, 16
    W, P = SMAX // page, 12
    layout = layout_from_rows(ROWS, dev)
    g = torch.Generator(device=dev).manual_seed(711)
    rand = lambda *shape: torch.randn(shape, device=dev, generator=g).to(dtype)  # noqa: E731
    q = rand(B, Hkv * G, T, D)
    kp, vp = (torch.full((P, Hkv, page, D), NAN, device=dev, dtype=dtype) for _ in range(2))
    table = torch.full((B, W), -1, dtype=torch.int32, device=dev)
    free = [7, 2, 9, 0, 11, 4, 5, 1, 10, 3, 8, 6]
    host_lens = [15, 63]
    for b, n in enumerate(host_lens):  # the state before the first step: ceil(n / page) pages per item, n rows written
        for lp in range((n + page - 1) // page):
            table[b, lp] = free.pop(0)
        for j in range(n):
            kp[int(table[b, j // page]), :, j % page] = rand(Hkv, D)
            vp[int(table[b, j // page]), :, j % page] = rand(Hkv, D)
    lens = lens_tensor(host_lens, dev, torch.int64)
    run = lambda: mm.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens, chunk=2, return_lse=True)  # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        out, lse = run()
    ptrs = (kp.data_ptr(), vp.data_ptr(), table.data_ptr())
    previous, allocated = None, 0
    for step in range(3):
        host_lens = [n + 1 for n in host_lens]
        with torch.no_grad():
            lens += 1
            for b, n in enumerate(host_lens):
                lp = (n - 1) // page
                if (n - 1) % page == 0:  # the new key opens a logical page
                    assert int(table[b, lp]) == -1
                    table[b, lp] = free.pop(0)
                    allocated += 1
                kp[int(table[b, lp]), :, (n - 1) % page] = rand(Hkv, D)
                vp[int(table[b, lp]), :, (n - 1) % page] = rand(Hkv, D)
            q.copy_(rand(*q.shape))
        assert lens.tolist() == host_lens and (kp.data_ptr(), vp.data_ptr(), table.data_ptr()) == ptrs
        want = run()
        kc, vc = gathered(kp, table), gathered(vp, table)
        contiguous = mm.block_sparse_attention_decode(q, kc, vc, layout, lens, chunk=2, return_lse=True)
        out.fill_(NAN)
        lse.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(out, want[0], f"replay {step}, k_lens {host_lens}: the eager paged call")
        assert_same_bits(lse, want[1], f"replay {step}: lse")
        assert_same_bits(out, contiguous[0], f"replay {step}: the contiguous call on the gathered state")
        assert_same_bits(lse, contiguous[1], f"replay {step}: the contiguous call, lse")
        check_rule(f"paged replay {step}", out, q, torch.nan_to_num(kc), torch.nan_to_num(vc), visible([ROWS], B, Hkv, T, host_lens), G)
        assert previous is None or not torch.equal(previous, out)
        previous = out.clone()
    assert host_lens == [18, 66] and allocated == 2


# ---- 8. the C ABI ---------------------------------------------------------------------------------------------------------------

def _paged_entry(capi, dtype):
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    fn = getattr(capi, "mi_block_attention_decode_paged_" + {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype])
    fn.argtypes = [vp, vp, i64] + 5 * [i32] + [vp, i64, i32, i32] + [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + \
        [vp, i32, i32, i32, f32] + [vp, i64, i64, vp, vp, sz, vp]
    fn.restype = ctypes.c_int
    capi.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    capi.mi_block_attention_decode_workspace_bytes.restype = sz
    return fn


@pytest.mark.parametrize("dtype,D,page", [(torch.bfloat16, 128, 16), (torch.float16, 32, 128)])
def test_8_c_abi_refusals_and_one_padded_call(mm, capi, dev, dtype, D, page):
    """MI_EINVAL / MI_ENOMEM without a launch (the outputs keep their sentinel), then one call on operands with leading
    dimensions and strides of their own — NaN around q and the pool, values outside the pool in the table's padding columns,
    SENTINEL around out, lse and the workspace —: the bits of the call through matmuls, nothing outside touched."""
    B, Hkv, G, T, k_lens, chunk = 2, 2, 5, 2, [130, 512], 2
    items, Hq, W = B * Hkv, Hkv * G, SMAX // page
    layout = layout_from_rows(ROWS, dev)
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 721 + D)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    kp, vp, table = paged(poison_unseen(k, vis), poison_unseen(v, vis), page, 722 + D)
    P = kp.shape[0]
    lens = lens_tensor(k_lens, dev)
    want = mm.block_sparse_attention_decode_paged(q, kp, vp, table, layout, lens, chunk=chunk, return_lse=True)
    assert torch.isfinite(want[0].float()).all()
    offsets, columns, nnz, L = mm._block_layout(layout, dev, 1, mm._csr_state(layout))["fwd"]
    fn = _paged_entry(capi, dtype)
    pq = padded(q.reshape(items * G, T, D), 0, NAN)
    pk, pv = (padded(x.reshape(P * Hkv, page, D), i, NAN) for i, x in ((1, kp), (2, vp)))
    ptable = torch.full((B, W + 3), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    ptable[:, :W] = table
    pout = padded(torch.full((items * G, T, D), SENTINEL, device=dev, dtype=dtype), 3, SENTINEL)
    lse_buf = torch.full((B * Hq * T + 16,), SENTINEL, device=dev)
    lse = lse_buf[8:8 + B * Hq * T]
    ws_bytes = capi.mi_block_attention_decode_workspace_bytes(items, T, G, D, SMAX, chunk)
    assert ws_bytes == items * T * 4 * G * (D + 2) * 4
    ws_buf = torch.full((ws_bytes + 32,), 0xAB, device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / D ** 0.5

    def call(group=G, chunk=chunk, D=D, q_ptr=pq.buf.data_ptr(), ldk=pk.ld, ws_bytes=ws_bytes, table_ptr=ptable.data_ptr(),
             table_ld=W + 3, pages=P, page=page):
        return fn(offsets.data_ptr(), columns.data_ptr(), nnz, L, items, Hkv, T, SMAX, table_ptr, table_ld, pages, page, D, q_ptr,
                  pq.ld, pq.stride, pk.buf.data_ptr(), ldk, pk.stride, Hkv * pk.stride, pv.buf.data_ptr(), pv.ld, pv.stride,
                  Hkv * pv.stride, lens.data_ptr(), B, group, chunk, scale, pout.buf.data_ptr(), pout.ld, pout.stride, lse.data_ptr(),
                  ws_buf.data_ptr() + 16, ws_bytes, stream)

    for kw in ({"group": 0}, {"group": 17}, {"D": 48}, {"chunk": 0}, {"q_ptr": pq.buf.data_ptr() + 2}, {"ldk": pk.ld + 4},
               {"page": 24}, {"page": 8}, {"page": 1024}, {"pages": -1}, {"table_ptr": ptable.data_ptr() + 2}, {"table_ptr": None},
               {"table_ld": W - 1}):
        assert call(**kw) == -1, kw   # MI_EINVAL
    assert call(ws_bytes=ws_bytes - 1) == -4  # MI_ENOMEM
    torch.cuda.synchronize()
    assert_same_bits(pout.buf, torch.full_like(pout.buf, SENTINEL), "a refused call launches nothing")
    assert call() == 0
    torch.cuda.synchronize()
    assert_outside_untouched(pout, "out")
    assert_same_bits(pout.x.reshape(B, Hq, T, D), want[0], f"{dtype} D={D} page={page} through the C ABI: out")
    assert_same_bits(lse.reshape(B, Hq, T), want[1], "through the C ABI: lse")
    rest = torch.cat([lse_buf[:8], lse_buf[8 + B * Hq * T:]])
    assert_same_bits(rest, torch.full_like(rest, SENTINEL), "around lse")
    guard = torch.cat([ws_buf[:16], ws_buf[16 + ws_bytes:]])
    assert (guard == 0xAB).all(), "around the workspace"
    assert torch.isfinite(pout.x.float()).all()
