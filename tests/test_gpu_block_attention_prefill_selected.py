"""matmuls.block_sparse_attention_prefill_selected and its paged / fp8 forms on the GPU: the prefill walk over
the caller's lists, one list per (k / v head, position tile) in the place of a layout row.

The contract is bit for bit: out and lse are those of block_sparse_attention_prefill with split=None and a (B, Hkv) layout whose
row r lists the same blocks in the same order.  From it: paged = contiguous on the gathered cache, fp8 without scales = the
2-byte call on the widened cache, a chunk of 100 tokens = chunks of 60 and 40 where the lists of the shared rows agree.  What
a CSR tensor cannot hold — a block listed twice — is checked under the project's accuracy rule (e_dev ≤ 8 · e_ref against
float64, lse within 1e-5) on a cache that holds the block twice.  Smax = 1024: 16 blocks; no layout row above 11 holds a token,
so block 15 in a layout row stands for a −1 of the list (both are skipped by the same statement)."""
import pytest
import torch

from gpu_helpers import assert_same_bits
from test_gpu_block_attention_decode import check_rule, lens_tensor, operands
from test_gpu_block_attention_decode_fp8 import codes, fp8, pools, wide
from test_gpu_block_attention_decode_paged import gathered, paged

pytestmark = pytest.mark.gpu

NAN = float("nan")
SMAX, BLOCKS, KB = 1024, 16, 64
K_SLOTS = 6
WIDTHS = [32, 64, 96, 128]


def clamp(n, lo, hi):
    return min(max(int(n), lo), hi)


def tiles_of(T):
    return -(-T // KB) + 1


def row_of(k_len, T, x):
    return (clamp(k_len, 0, SMAX) - T) // KB + x


def hand_lists(B, Hkv, T, k_lens, seed, duplicate=False):
    """(ids [B, Hkv, X, 6], counts [B, Hkv, X]) on the CPU.  Tile x of item b is layout row r; l0 … l4 are distinct blocks below
    r in a shuffled order (−1 where r has fewer).  Six patterns: the diagonal block first; −1 in the middle; entries above r
    (r + 1 and 13); a count above K; a negative count (an empty list: zero rows); a count that cuts the row.  duplicate: l0 is
    listed twice."""
    X = tiles_of(T)
    g = torch.Generator().manual_seed(seed)
    ids = torch.empty((B, Hkv, X, K_SLOTS), dtype=torch.int32)
    counts = torch.empty((B, Hkv, X), dtype=torch.int32)
    for b in range(B):
        for h in range(Hkv):
            for x in range(X):
                r = row_of(k_lens[b], T, x)
                low = torch.randperm(max(r, 0), generator=g).tolist()[:5] if 0 < r <= BLOCKS else []
                l = low + [-1] * (5 - len(low))
                p = (b * Hkv + h + x) % 6
                if duplicate:
                    lst, n = [l[0], r, l[1], l[0], l[2], -1], 6
                else:
                    lst, n = [([r, l[0], l[1], l[2], l[3], l[4]], 6), ([l[0], -1, r, l[1], -1, l[2]], 6), ([l[0], r + 1, l[1], r, 13, l[2]], 6),
                              ([l[0], l[1], r, l[2], l[3], l[4]], 9), ([l[0], r, l[1], l[2], l[3], l[4]], -2), ([l[1], l[0], r, l[2], -1, l[3]], 3)][p]
                ids[b, h, x], counts[b, h, x] = torch.tensor(lst), n
    return ids, counts


def token_tile(T, k_len, new_len, t):
    """(pos, r, x) of slot t, or None when it holds no token."""
    n = clamp(k_len, 0, SMAX)
    pos = n - T + t
    if pos < 0 or t < T - (T if new_len is None else clamp(new_len, 0, T)):
        return None
    return pos, pos // KB, pos // KB - (n - T) // KB


def vis_of_lists(ids, counts, T, k_lens, new_lens=None, smax=SMAX):
    """Boolean CPU mask [B, Hkv, T, Smax] from the rule alone: the first clamp(count, 0, K) entries of the token's tile, inside
    the grid, not above r, keys ≤ pos."""
    B, Hkv, X, K = ids.shape
    vis = torch.zeros(B, Hkv, T, smax, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            where = token_tile(T, k_lens[b], None if new_lens is None else new_lens[b], t)
            if where is None:
                continue
            pos, r, x = where
            assert 0 <= x < X
            for h in range(Hkv):
                for J in ids[b, h, x, :clamp(counts[b, h, x], 0, K)].tolist():
                    if 0 <= J < SMAX // KB and J <= r:
                        vis[b, h, t, KB * J:min(KB * J + KB, pos + 1)] = True
    return vis


def layout_of_lists(ids, counts, T, k_lens, dev):
    """The equivalent (B, Hkv) layout: row r of item (b, h) holds the list of its tile in its order — a −1 as block 15, which
    like it is skipped (no row that holds a token reaches 15) —, row 15 pads every item to X · K entries."""
    B, Hkv, X, K = ids.shape
    crows, cols = [], []
    for b in range(B):
        for h in range(Hkv):
            per_row = {}
            for x in range(X):
                r = row_of(k_lens[b], T, x)
                if 0 <= r < BLOCKS - 1:
                    per_row[r] = [J if J >= 0 else BLOCKS - 1 for J in ids[b, h, x, :clamp(counts[b, h, x], 0, K)].tolist()]
            used = sum(len(v) for v in per_row.values())
            per_row[BLOCKS - 1] = list(range(X * K - used))
            crow, col = [0], []
            for r in range(BLOCKS):
                col += per_row.get(r, [])
                crow.append(len(col))
            crows.append(crow)
            cols.append(col)
    crow = torch.tensor(crows, device=dev).reshape(B, Hkv, BLOCKS + 1)
    col = torch.tensor(cols, device=dev).reshape(B, Hkv, X * K)
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape, device=dev), size=(B, Hkv, BLOCKS, BLOCKS))


def same(got, want, what):
    assert_same_bits(got[0], want[0], f"{what}: out")
    assert_same_bits(got[1], want[1], f"{what}: lse")


def news_tensor(new_lens, dev):
    return None if new_lens is None else torch.tensor(new_lens, device=dev, dtype=torch.int32)


# ---- 1. the bits of the layout call ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 5, 20])
@pytest.mark.parametrize("D", WIDTHS)
def test_1_hand_written_lists_have_the_bits_of_the_layout_call(mm, dev, D, G):
    B, Hkv = 2, 2
    dtype = torch.bfloat16 if (D // 32 + G) % 2 else torch.float16
    k_lens = [700, 131]  # T = 100: rows 9, 10 (both partial; the third tile holds no token) and rows 0, 1, 2 (first and last partial)
    for T, new_lens in ((1, None), (100, None), (100, [100, 40]), (100, [0, 3])):
        q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3300 + D + G + T, smax=SMAX)
        ids, counts = hand_lists(B, Hkv, T, k_lens, 3301 + T)
        lens, news = lens_tensor(k_lens, dev), news_tensor(new_lens, dev)
        out, lse = mm.block_sparse_attention_prefill_selected(q, k, v, ids.to(dev), counts.to(dev), lens, new_lens=news, return_lse=True)
        assert out.dtype == dtype and out.shape == q.shape and not out.requires_grad and lse.shape == q.shape[:3]
        want = mm.block_sparse_attention_prefill(q, k, v, layout_of_lists(ids, counts, T, k_lens, dev), lens, new_lens=news,
                                                 return_lse=True)
        same((out, lse), want, f"D={D} G={G} T={T} new_lens={new_lens}")
        vis = vis_of_lists(ids, counts, T, k_lens, new_lens)
        check_rule(f"prefill over lists D={D} G={G} T={T} new_lens={new_lens}", out, q, k, v, vis, G, lse)
        if T == 100 and new_lens is None:
            assert (counts < 0).any() and (counts > K_SLOTS).any() and not vis.any(-1).all() and vis.any(-1).any()


def test_1_a_block_listed_twice_counts_twice(mm, dev):
    """A CSR tensor cannot hold a block twice: the float64 reference runs on a cache of 17 blocks whose last block is a copy of
    the duplicated one, seen by the same tokens (the duplicate lies below r: every key of it is seen)."""
    B, Hkv, G, T, D, dtype, k_lens = 1, 2, 2, 100, 64, torch.bfloat16, [700]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3310, smax=SMAX)
    ids, counts = hand_lists(B, Hkv, T, k_lens, 3311, duplicate=True)
    out, lse = mm.block_sparse_attention_prefill_selected(q, k, v, ids.to(dev), counts.to(dev), lens_tensor(k_lens, dev), return_lse=True)
    vis = torch.cat([vis_of_lists(ids, counts, T, k_lens), torch.zeros(B, Hkv, T, KB, dtype=torch.bool)], -1)
    k2, v2 = (torch.cat([x, torch.zeros_like(x[:, :, :KB])], 2) for x in (k, v))
    for h in range(Hkv):
        for t in range(T):
            _, r, x = token_tile(T, k_lens[0], None, t)
            J = int(ids[0, h, x, 0])
            assert 0 <= J < r and int(ids[0, h, x, 3]) == J
            vis[0, h, t, SMAX:] = True
    # the chunk's two tiles duplicate a block of their own: the seventeenth block is filled, and the reference taken, tile by tile
    for x in range(2):
        rows = [t for t in range(T) if token_tile(T, k_lens[0], None, t)[2] == x]
        for h in range(Hkv):
            J = int(ids[0, h, x, 0])
            k2[0, h, SMAX:], v2[0, h, SMAX:] = k[0, h, KB * J:KB * J + KB], v[0, h, KB * J:KB * J + KB]
        sl = slice(rows[0], rows[-1] + 1)
        check_rule(f"a block listed twice, tile {x}", out[:, :, sl], q[:, :, sl], k2, v2, vis[:, :, sl], G, lse[:, :, sl])


# ---- 2. the cache forms ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [16, 128])
def test_2_the_paged_form_has_the_bits_of_the_contiguous_form(mm, dev, page):
    B, Hkv, G, T, D, dtype, k_lens, new_lens = 2, 2, 5, 100, 96, torch.float16, [700, 131], [100, 40]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3320 + page, smax=SMAX)
    ids, counts = (x.to(dev) for x in hand_lists(B, Hkv, T, k_lens, 3321))
    lens, news = lens_tensor(k_lens, dev), news_tensor(new_lens, dev)
    kp, vp, table = paged(k, v, page, 3322 + page)
    got = mm.block_sparse_attention_prefill_selected_paged(q, kp, vp, table, ids, counts, lens, new_lens=news, return_lse=True)
    want = mm.block_sparse_attention_prefill_selected(q, gathered(kp, table), gathered(vp, table), ids, counts, lens, new_lens=news,
                                                      return_lse=True)
    same(got, want, f"page {page}")
    assert torch.isfinite(got[0].float()).all()  # (the unreferenced pages of the pool are NaN)


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 64), (torch.float16, 128)])
def test_2_fp8_without_scales_has_the_bits_of_the_widened_cache(mm, dev, dtype, D):
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [700, 131]
    q = operands(dev, B, Hkv, G, T, D, dtype, 3330 + D, smax=KB)[0]
    kc, vc = codes(3331 + D, B, Hkv, SMAX, D), codes(3332 + D, B, Hkv, SMAX, D)
    ids, counts = (x.to(dev) for x in hand_lists(B, Hkv, T, k_lens, 3333))
    lens = lens_tensor(k_lens, dev)
    want = mm.block_sparse_attention_prefill_selected(q, wide(kc, dtype, dev), wide(vc, dtype, dev), ids, counts, lens, return_lse=True)
    same(mm.block_sparse_attention_prefill_selected_fp8(q, fp8(kc, dev), fp8(vc, dev), ids, counts, lens, return_lse=True), want,
         f"fp8 D={D} {dtype}")
    for page in (16, 64):
        kp, vp, table = pools(kc, vc, page, 3334 + D)
        same(mm.block_sparse_attention_prefill_selected_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), ids, counts, lens,
                                                                  return_lse=True), want, f"paged fp8 D={D} {dtype} page {page}")


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_2_fp8_with_per_head_scales_under_the_rule_on_the_scaled_cache(mm, dev, dtype, D):
    B, Hkv, G, T, k_lens = 2, 2, 2, 100, [700, 131]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3340 + D, smax=SMAX)
    ids, counts = hand_lists(B, Hkv, T, k_lens, 3341)
    lens = lens_tensor(k_lens, dev)
    k8, ks = mm.kv_to_fp8(k)
    v8, vs = mm.kv_to_fp8(v)
    real_k = k8.float() * ks.reshape(1, Hkv, 1, 1)
    real_v = v8.float() * vs.reshape(1, Hkv, 1, 1)
    got = mm.block_sparse_attention_prefill_selected_fp8(q, k8, v8, ids.to(dev), counts.to(dev), lens, k_scale=ks, v_scale=vs,
                                                         return_lse=True)
    check_rule(f"prefill over lists, fp8 per-head scales D={D} {dtype}", got[0], q, real_k, real_v, vis_of_lists(ids, counts, T, k_lens),
               G, got[1])
    same(got, mm.block_sparse_attention_prefill_fp8(q, k8, v8, layout_of_lists(ids, counts, T, k_lens, dev), lens, k_scale=ks, v_scale=vs,
                                                    return_lse=True), "fp8 with scales against the layout call")


# ---- 3. every candidate --------------------------------------------------------------------------------------------------

def causal_vis(B, Hkv, T, k_lens, new_lens=None):
    vis = torch.zeros(B, Hkv, T, SMAX, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            where = token_tile(T, k_lens[b], None if new_lens is None else new_lens[b], t)
            if where is not None:
                vis[b, :, t, :where[0] + 1] = True
    return vis


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)])
def test_3_every_candidate_is_the_dense_causal_call(mm, dev, D, dtype):
    """K = Smax / 64 ≥ the candidates of every tile: the list of tile r is 0 … r ascending, the row of the dense causal layout."""
    B, Hkv, G, T, k_lens, new_lens = 3, 2, 4, 100, [700, 131, 1024], [100, 40, 77]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3370 + D, smax=SMAX)
    lens, news = lens_tensor(k_lens, dev), news_tensor(new_lens, dev)
    bounds = mm.key_block_bounds(k, lens)
    ids, counts = mm.select_key_blocks_tiles(q, bounds, lens, BLOCKS, new_lens=news)
    got = mm.block_sparse_attention_prefill_selected(q, k, v, ids, counts, lens, new_lens=news, return_lse=True)
    causal = torch.tril(torch.ones(BLOCKS, BLOCKS, device=dev)).to_sparse_csr()
    same(got, mm.block_sparse_attention_prefill(q, k, v, causal, lens, new_lens=news, return_lse=True), f"every candidate D={D}")
    assert counts.cpu().tolist()[0][0] == [10, 11, 0] and counts.cpu().tolist()[1][1] == [0, 2, 3]
    check_rule(f"select + prefill, every candidate D={D}", got[0], q, k, v, causal_vis(B, Hkv, T, k_lens, new_lens), G, got[1])


# ---- 4. planted blocks ------------------------------------------------------------------------------------------------------------------------

def test_4_planted_blocks_are_listed_and_carry_the_attention(mm, dev):
    """Small keys everywhere but in blocks 3, 5 and 7, whose keys lie along the direction the chunk's queries share: on the
    CPU, in float64, the softmax mass outside sink + local + planted is below 2⁻²⁰ for every token (asserted first).  With
    K = forced + 3 every tile lists [0, 3, 5, 7, r − 1, r], and out is the dense causal attention under the accuracy rule."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 100, 64, torch.bfloat16, [700, 900]
    plantedJ = (3, 5, 7)
    g = torch.Generator(device=dev).manual_seed(3380)
    u = torch.nn.functional.normalize(torch.randn((B, Hkv, 1, 1, D), device=dev, generator=g), dim=-1)
    q = (16 * u + 0.5 * torch.randn((B, Hkv, G, T, D), device=dev, generator=g)).reshape(B, Hkv * G, T, D).to(dtype)
    k = (0.05 * torch.randn((B, Hkv, SMAX, D), device=dev, generator=g))
    for J in plantedJ:
        k[:, :, KB * J:KB * J + KB] = 16 * u[:, :, 0] + 0.05 * torch.randn((B, Hkv, KB, D), device=dev, generator=g)
    k, v = k.to(dtype), torch.randn((B, Hkv, SMAX, D), device=dev, generator=g).to(dtype)
    vis = causal_vis(B, Hkv, T, k_lens)
    kept = torch.zeros_like(vis)
    for b in range(B):
        for t in range(T):
            pos, r, _ = token_tile(T, k_lens[b], None, t)
            for J in (0, r - 1, r) + plantedJ:
                kept[b, :, t, KB * J:min(KB * J + KB, pos + 1)] = True
    logits = (q.cpu().double() @ k.cpu().double().repeat_interleave(G, 1).transpose(-1, -2)) / D ** 0.5
    p = torch.softmax(logits.masked_fill(~vis.repeat_interleave(G, 1), -float("inf")), -1)
    outside = p.masked_fill(kept.repeat_interleave(G, 1), 0.0).sum(-1).max()
    assert outside < 2.0 ** -20, f"precondition: float64 softmax mass {float(outside):.3e} outside the kept blocks"
    lens = lens_tensor(k_lens, dev)
    ids, counts = mm.select_key_blocks_tiles(q, mm.key_block_bounds(k, lens), lens, 6, sink=1, local=2)
    for b in range(B):
        for x in range(2):
            r = row_of(k_lens[b], T, x)
            assert ids[b, :, x].tolist() == [[0, 3, 5, 7, r - 1, r]] * Hkv and counts[b, :, x].tolist() == [6] * Hkv, (b, x, ids[b, :, x].tolist())
    out, lse = mm.block_sparse_attention_prefill_selected(q, k, v, ids, counts, lens, return_lse=True)
    check_rule("planted blocks against the dense causal attention", out, q, k, v, vis, G, lse)


# ---- 5. one graph --------------------------------------------------------------------------------------------------------------------------

def test_5_append_bounds_select_prefill_in_one_graph(mm, dev):
    """`lens += new; rope_kv_cache_append; key_block_bounds(last=T); select_key_blocks_tiles; prefill over the lists` captured
    once and replayed for three chunks while the cache grows in place (item 0 crosses a block boundary; item 1 takes 3 of the
    17 slots each time): every replay is bit for bit the eager sequence on a copy of the state — out, lse, the lists, the
    cache and the bounds."""
    B, Hkv, G, T, D, dtype, K = 2, 2, 2, 17, 64, torch.float16, 4
    Hq = Hkv * G
    g = torch.Generator(device=dev).manual_seed(3390)
    k, v = (torch.randn((B, Hkv, SMAX, D), device=dev, generator=g).to(dtype) for _ in range(2))
    lens = lens_tensor([370, 500], dev, torch.int64)
    news = lens_tensor([T, 3], dev, torch.int64)
    bounds = mm.key_block_bounds(k, lens, torch.zeros((B, Hkv, BLOCKS, 2, D), device=dev, dtype=dtype))
    ang = torch.arange(SMAX, device=dev, dtype=torch.float32)[:, None] * torch.exp(-torch.arange(D // 2, device=dev) * 0.2)[None]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    fused = torch.randn((B, T, Hq + 2 * Hkv, D), device=dev, generator=g).to(dtype)
    qv, knew, vnew = (fused[:, :, a:b].transpose(1, 2) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))

    def step(lens, k, v, bounds):
        lens += news
        qr = mm.rope_kv_cache_append(qv, knew, vnew, cos, sin, k, v, lens, new_lens=news)
        mm.key_block_bounds(k, lens, bounds, last=T)
        ids, counts = mm.select_key_blocks_tiles(qr, bounds, lens, K, sink=1, local=2, new_lens=news)
        out, lse = mm.block_sparse_attention_prefill_selected(qr, k, v, ids, counts, lens, new_lens=news, return_lse=True)
        return out, lse, ids, counts

    def copies():
        return lens.clone(), k.clone(), v.clone(), bounds.clone()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(*copies())  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    state = copies()  # the capture itself does not run: the state is as before
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        captured = step(lens, k, v, bounds)
    for x, y in zip((lens, k, v, bounds), state):
        x.copy_(y)
    previous = None
    for replay in range(3):
        fused.copy_(torch.randn(fused.shape, device=dev, generator=g).to(dtype))
        eager = copies()
        want = step(*eager)
        for x in captured[:2]:
            x.fill_(NAN)
        captured[2].fill_(-5), captured[3].fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        assert lens.tolist() == eager[0].tolist() == [370 + 17 * (replay + 1), 500 + 3 * (replay + 1)]
        same(captured[:2], want[:2], f"replay {replay}")
        assert torch.equal(captured[2], want[2]) and torch.equal(captured[3], want[3]), f"replay {replay}: the lists"
        assert_same_bits(k, eager[1], f"replay {replay}: the cache")
        assert_same_bits(bounds, eager[3], f"replay {replay}: the bounds")
        assert (captured[0][1, :, :T - 3] == 0).all() and torch.isfinite(captured[1][0]).all()
        assert previous is None or not torch.equal(previous, captured[0])
        previous = captured[0].clone()


# ---- 6. unseen memory --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["BSHD", "pool"])
def test_6_nothing_outside_is_read(mm, dev, form):
    """NaN in every key no token sees — unlisted blocks, blocks beyond a row's count, blocks above r, positions beyond pos, so
    everything at or beyond k_len —, between the rows of a strided cache, and in the unreferenced pages of a pool; q as the
    slice of a NaN buffer: out is finite and has the bits of the clean contiguous call."""
    B, Hkv, G, T, D, dtype, k_lens, new_lens = 2, 2, 4, 100, 64, torch.float16, [700, 131], [100, 40]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 3360, smax=SMAX)
    ids, counts = hand_lists(B, Hkv, T, k_lens, 3361)
    lens, news = lens_tensor(k_lens, dev), news_tensor(new_lens, dev)
    want = mm.block_sparse_attention_prefill_selected(q, k, v, ids.to(dev), counts.to(dev), lens, new_lens=news, return_lse=True)
    unseen = ~vis_of_lists(ids, counts, T, k_lens, new_lens).any(2).to(dev)
    assert unseen.any() and not unseen.all()
    kx, vx = k.clone(), v.clone()
    kx[unseen], vx[unseen] = NAN, NAN
    qbuf = torch.full((B, T, Hkv * G + 2, D), NAN, device=dev, dtype=dtype)  # a fused projection: q is a slice of it
    qs = qbuf[:, :, :Hkv * G].transpose(1, 2)
    qs.copy_(q)
    assert not qs.is_contiguous()
    if form == "BSHD":
        def strided(x):
            buf = torch.full((B, SMAX, Hkv, D + 8), NAN, device=dev, dtype=dtype)
            view = buf[..., :D].transpose(1, 2)
            view.copy_(x)
            return view
        got = mm.block_sparse_attention_prefill_selected(qs, strided(kx), strided(vx), ids.to(dev), counts.to(dev), lens, new_lens=news,
                                                         return_lse=True)
    else:
        kp, vp, table = paged(kx, vx, 32, 3362)
        got = mm.block_sparse_attention_prefill_selected_paged(qs, kp, vp, table, ids.to(dev), counts.to(dev), lens, new_lens=news,
                                                               return_lse=True)
    assert torch.isfinite(got[0].float()).all()
    same(got, want, form)


# ---- 7. a row's bits do not depend on T, B or the launch -------------------------------------------------------------------------------

def test_7_a_chunk_of_100_is_chunks_of_60_and_40_and_an_item_is_the_call_on_it_alone(mm, dev):
    """The lists are a function of the layout row here, so the chunks' shared rows agree: row r of every (b, h) lists
    [r, r − 2, 0, r − 1] cut to the grid."""
    B, Hkv, G, D, dtype, k_lens = 3, 2, 4, 128, torch.bfloat16, [700, 131, 420]
    q, k, v = operands(dev, B, Hkv, G, 100, D, dtype, 3350, smax=SMAX)

    def lists(T, lens_now):
        X = tiles_of(T)
        ids = torch.full((len(lens_now), Hkv, X, 4), -1, dtype=torch.int32)
        for b, n in enumerate(lens_now):
            for x in range(X):
                r = row_of(n, T, x)
                ids[b, :, x] = torch.tensor([r, r - 2, 0 if r > 2 else -1, r - 1])
        return ids.to(dev), torch.full((len(lens_now), Hkv, X), 4, dtype=torch.int32, device=dev)

    whole = mm.block_sparse_attention_prefill_selected(q, k, v, *lists(100, k_lens), lens_tensor(k_lens, dev), return_lse=True)
    first_lens = [n - 40 for n in k_lens]
    a = mm.block_sparse_attention_prefill_selected(q[:, :, :60], k, v, *lists(60, first_lens), lens_tensor(first_lens, dev), return_lse=True)
    b = mm.block_sparse_attention_prefill_selected(q[:, :, 60:], k, v, *lists(40, k_lens), lens_tensor(k_lens, dev), return_lse=True)
    same((torch.cat([a[0], b[0]], 2), torch.cat([a[1], b[1]], 2)), whole, "100 = 60 + 40")
    for i in range(B):
        ids, counts = lists(100, k_lens)
        alone = mm.block_sparse_attention_prefill_selected(q[i:i + 1], k[i:i + 1], v[i:i + 1], ids[i:i + 1].contiguous(),
                                                           counts[i:i + 1].contiguous(), lens_tensor(k_lens[i:i + 1], dev), return_lse=True)
        same(alone, (whole[0][i:i + 1], whole[1][i:i + 1]), f"item {i} alone")
    assert torch.isfinite(whole[0].float()).all() and torch.isfinite(whole[1]).all()
