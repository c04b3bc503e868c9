"""The two calls around a tree-masked decode step on the MI355X, and the step as one captured graph:
rope_kv_cache_append{,_paged}(positions=…) — a slot rotated by an explicit table row and still written to its own row —,
kv_cache_compact{,_paged} — the accepted path's rows moved to the front of the drafted window — and
`lens += T; rope(positions); decode(tree_mask); compact; lens −= T − n` replayed with new trees against the eager sequence.
Everything is bit for bit: the rope call against TODAY's call (positions = slot: the call without them; general positions:
per item, today's call with the cos / sin rows gathered into the slots' rows), the caches after a compaction against torch
indexing on a clone, byte for byte, sentinels and unreferenced pages included."""
import pytest
import torch

from gpu_helpers import assert_same_bits
from test_gpu_block_attention_decode import lens_tensor
from test_gpu_block_attention_decode_paged import fresh_table, gathered, scatter
from test_gpu_block_attention_decode_selected import causal_layout
from test_gpu_block_attention_decode_tree import mask_tensor, tree_parents, words_of
from test_gpu_rope_kv_cache_append import tables

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
FORMS = [(0, False), (0, True), (16, False), (64, True)]  # (page, fp8)


def raw(x):
    """A tensor's elements as integers: int16 bits, or e4m3fn bytes."""
    return x.view(torch.uint8 if x.element_size() == 1 else torch.int16).cpu()


def same_raw(got, want, what):
    got, want = raw(got), raw(want)
    bad = torch.nonzero(got != want)
    assert got.shape == want.shape and bad.numel() == 0, f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {bad[:4].tolist()}"


def random_cache(seed, dev, dtype, fp8, *shape):
    """Random finite values in the cache's own type."""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).clamp(-3, 3)
    return x.to(F8 if fp8 else dtype).to(dev)


def cache_of(seed, dev, dtype, page, fp8, B, Hkv, Smax, D):
    """(k, v, table or None): a flat cache, or a pool of shuffled pages with three unreferenced ones."""
    k, v = (random_cache(seed + i, dev, dtype, fp8, B, Hkv, Smax, D) for i in range(2))
    if not page:
        return k, v, None
    W = Smax // page
    table = fresh_table(B, W, B * W + 3, seed, dev)
    pools = []
    for i, x in enumerate((k, v)):
        pool = random_cache(seed + 10 + i, dev, dtype, fp8, B * W + 3, Hkv, page, D)
        scatter(pool.view(torch.uint8 if fp8 else torch.int16), table, x.view(torch.uint8 if fp8 else torch.int16))
        pools.append(pool)
    return pools[0], pools[1], table


def rows_of(x, table):
    """The logical cache [B, Hkv, Smax, D] as integers."""
    ints = x.view(torch.uint8 if x.element_size() == 1 else torch.int16)
    return (ints if table is None else gathered(ints, table)).cpu()


# ---- 4. rope with positions -----------------------------------------------------------------------------------------------------

def rope(mm, q, kn, vn, cos, sin, k, v, table, lens, **kw):
    if table is None:
        return mm.rope_kv_cache_append(q, kn, vn, cos, sin, k, v, lens, **kw)
    return mm.rope_kv_cache_append_paged(q, kn, vn, cos, sin, k, v, table, lens, **kw)


def rope_case(dev, dtype, seed, B=3, Hkv=2, Hq=4, T=5, D=64):
    g = torch.Generator().manual_seed(seed)
    q, kn, vn = (torch.randn((B, H, T, D), generator=g).to(dtype).to(dev) for H in (Hq, Hkv, Hkv))
    return q, kn, vn


@pytest.mark.parametrize("page,fp8", FORMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_4_positions_equal_to_the_slots_are_the_call_without_them(mm, dev, dtype, page, fp8):
    B, Hkv, T, D, Smax, k_lens = 3, 2, 5, 64, 256, [200, 65, 3]
    cos, sin = (x.to(dev) for x in tables(Smax, D))
    q, kn, vn = rope_case(dev, dtype, 3100)
    lens = lens_tensor(k_lens, dev)
    slots = (lens - T)[:, None] + torch.arange(T, device=dev, dtype=torch.int32)
    scales = dict(k_scale=torch.tensor([0.5, 2.0], device=dev), v_scale=0.25) if fp8 else {}
    for inter, new_lens, wide in ((False, None, False), (True, torch.tensor([5, 2, 4], device=dev), True)):
        k0, v0, table = cache_of(3110, dev, dtype, page, fp8, B, Hkv, Smax, D)
        k1, v1 = k0.clone(), v0.clone()
        want = rope(mm, q, kn, vn, cos, sin, k0, v0, table, lens, interleaved=inter, new_lens=new_lens, **scales)
        got = rope(mm, q, kn, vn, cos, sin, k1, v1, table, lens, interleaved=inter, new_lens=new_lens,
                   positions=slots.long() if wide else slots, **scales)
        assert_same_bits(got, want, f"page {page} fp8 {fp8} interleaved {inter}: q_out")
        same_raw(k1, k0, "k")
        same_raw(v1, v0, "v")


@pytest.mark.parametrize("page,fp8", FORMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_4_general_positions_are_todays_call_with_the_table_rows_gathered_into_the_slots(mm, dev, dtype, page, fp8):
    """Per item: the rows of the slots that hold a token — q_out's and the cache's — have the bits of TODAY's call on the item
    alone with cos / sin row positions[b, t] copied into row slot t.  A position outside [0, Pmax) holds no token: zero rows
    of q_out and k_out, the cache row keeps its bytes.  With new_lens too."""
    B, Hkv, Hq, T, D, Smax, k_lens = 3, 2, 4, 5, 64, 256, [200, 65, 130]
    cos, sin = (x.to(dev) for x in tables(Smax, D))
    q, kn, vn = rope_case(dev, dtype, 3200)
    lens = lens_tensor(k_lens, dev)
    positions = torch.tensor([[7, 7, 255, 0, 31], [64, -1, 256, 5, 2 ** 31 - 1], [9, 200, 3, 3, 129]], dtype=torch.int64, device=dev)
    scales = dict(k_scale=torch.tensor([0.5, 2.0], device=dev), v_scale=0.25) if fp8 else {}
    for new_lens in (None, [5, 4, 2]):
        news = None if new_lens is None else torch.tensor(new_lens, device=dev)
        k0, v0, table = cache_of(3210, dev, dtype, page, fp8, B, Hkv, Smax, D)
        k1, v1, k_out = k0.clone(), v0.clone(), torch.full_like(kn, 7.0)
        got = rope(mm, q, kn, vn, cos, sin, k1, v1, table, lens, new_lens=news, positions=positions, k_out=k_out, **scales)
        before_k, before_v, after_k, after_v = rows_of(k0, table), rows_of(v0, table), rows_of(k1, table), rows_of(v1, table)
        touched = torch.zeros(B, Smax, dtype=torch.bool)
        for b in range(B):
            n = T if new_lens is None else new_lens[b]
            held = [t for t in range(T) if t >= T - n and 0 <= int(positions[b, t]) < Smax]
            cos_b, sin_b = torch.zeros_like(cos), torch.zeros_like(sin)
            for t in held:
                cos_b[k_lens[b] - T + t], sin_b[k_lens[b] - T + t] = cos[positions[b, t]], sin[positions[b, t]]
            kb, vb = k0.clone(), v0.clone()
            tb = None if table is None else table[b:b + 1]
            kb_, vb_ = (kb, vb) if table is not None else (kb[b:b + 1], vb[b:b + 1])
            ko_b = torch.empty_like(kn[b:b + 1])
            want = rope(mm, q[b:b + 1], kn[b:b + 1], vn[b:b + 1], cos_b, sin_b, kb_, vb_, tb, lens[b:b + 1],
                        new_lens=None if news is None else news[b:b + 1], k_out=ko_b, **scales)
            want_k, want_v = rows_of(kb, table), rows_of(vb, table)
            for t in range(T):
                slot = k_lens[b] - T + t
                if t in held:
                    assert_same_bits(got[b, :, t], want[0, :, t], f"item {b} token {t}: q_out")
                    assert_same_bits(k_out[b, :, t], ko_b[0, :, t], f"item {b} token {t}: k_out")
                    assert torch.equal(after_k[b, :, slot], want_k[b, :, slot]) and torch.equal(after_v[b, :, slot], want_v[b, :, slot]), \
                        f"item {b} token {t}: the cache row {slot}"
                    touched[b, slot] = True
                else:
                    assert (got[b, :, t] == 0).all() and (k_out[b, :, t] == 0).all(), f"item {b} token {t}: no token, zero rows"
        assert torch.equal(after_k[~touched[:, None].expand(B, Hkv, Smax)], before_k[~touched[:, None].expand(B, Hkv, Smax)])
        assert torch.equal(after_v[~touched[:, None].expand(B, Hkv, Smax)], before_v[~touched[:, None].expand(B, Hkv, Smax)])
        if table is not None:  # the unreferenced pages
            free = torch.ones(k0.shape[0], dtype=torch.bool)
            free[table.cpu().long().flatten()] = False
            same_raw(k1[free.to(dev)], k0[free.to(dev)], "unreferenced pages")


# ---- 5. compaction --------------------------------------------------------------------------------------------------------------

def compacted(cache, table, k_lens, accept, counts, T, Smax):
    """torch indexing on a clone: the integers of the cache (or pool) after the compaction."""
    old, new = cache.clone(), cache.clone()
    B = len(k_lens)
    P = cache.shape[0]
    page = cache.shape[2]

    def row(b, j):  # (first index, row) of logical row j of item b, or None
        if not 0 <= j < Smax:
            return None
        if table is None:
            return b, j
        e = int(table[b, j // page])
        return (e, j % page) if 0 <= e < P else None

    for b in range(B):
        base = k_lens[b] - T
        for i in range(max(0, min(int(counts[b]), T))):
            off = int(accept[b, i])
            if not 0 <= off < T:
                continue
            src, dst = row(b, base + off), row(b, base + i)
            if src is not None and dst is not None:
                new[dst[0], :, dst[1]] = old[src[0], :, src[1]]
    return new


@pytest.mark.parametrize("page", [0, 16, 64])
@pytest.mark.parametrize("kind", ["bf16", "f16", "fp8"])
@pytest.mark.parametrize("D,T", [(64, 7), (128, 64), (32, 64)])
def test_5_every_byte_is_torch_indexing_on_a_clone(mm, dev, kind, page, D, T):
    """n ∈ {0, 1, T, 3}; the path [1, 2, 3] (a write before its read would show), a reversal and a rotation of the whole window
    (every row is another's source); offsets −1 and T; windows that leave the cache at both ends; a −1 table entry under a
    window.  The flat caches sit in padded buffers of sentinels, the pools keep three unreferenced pages."""
    B, Hkv, Smax = 7, 1, 512
    dtype, fp8 = {"bf16": (torch.bfloat16, False), "f16": (torch.float16, False), "fp8": (torch.bfloat16, True)}[kind]
    ints = torch.uint8 if fp8 else torch.int16
    k_lens = [130, 200, 300, 3, Smax + 2, 192, 449]
    g = torch.Generator().manual_seed(3300 + T)
    accept = torch.randint(0, T, (B, T), generator=g, dtype=torch.int32)
    accept[0, :3] = torch.tensor([1, 2, 3])
    accept[1] = torch.arange(T - 1, -1, -1)
    accept[2] = (torch.arange(T) + 1) % T
    accept[3, 0], accept[3, 1] = -1, T
    accept[5, :4] = torch.tensor([2, 2, 0, T - 1])
    counts = torch.tensor([3, T, T + 5, T, T, 1, 0], dtype=torch.int32)
    unit = 16 if fp8 else 8
    if page:
        k, v, table = cache_of(3310, dev, dtype, page, fp8, B, Hkv, Smax, D)
        table[1, (200 - 1) // page] = -1
        table[2, (300 - 1) // page] = -1
    else:
        bufs = [random_cache(3310 + i, dev, dtype, fp8, B, Hkv, Smax, D + unit) for i in range(2)]
        (k, v), table = (x[..., :D] for x in bufs), None
    whole = [x.view(ints) for x in ((k, v) if page else bufs)]
    want = [compacted(x.cpu()[..., :D] if not page else x.cpu(), None if table is None else table.cpu(), k_lens, accept, counts, T, Smax)
            for x in whole]
    before = [x.cpu().clone() for x in whole]
    lens = lens_tensor(k_lens, dev)
    if page:
        mm.kv_cache_compact_paged(k, v, table, lens, accept.to(dev), counts.to(dev), T)
    else:
        mm.kv_cache_compact(k, v, lens, accept.to(dev), counts.to(dev), T)
    for x, w, b0, name in zip(whole, want, before, "kv"):
        got = x.cpu()
        assert torch.equal(got[..., :D], w), f"{name}: {int((got[..., :D] != w).sum())} elements differ from torch indexing on a clone"
        assert torch.equal(got[..., D:], b0[..., D:]), f"{name}: the sentinels between the rows"
        assert not torch.equal(got, b0), f"{name}: the case moves something"
    assert torch.equal(lens.cpu(), torch.tensor(k_lens, dtype=torch.int32)), "k_lens is not written"


# ---- 6. the whole step in one captured graph ------------------------------------------------------------------------------------

def test_6_one_captured_graph_of_the_speculative_step(mm, dev):
    B, Hkv, G, T, D, Smax, dtype = 2, 2, 2, 5, 64, 512, torch.bfloat16
    cos, sin = (x.to(dev) for x in tables(Smax, D))
    layout = causal_layout(Smax // 64, dev)
    g = torch.Generator().manual_seed(3400)
    q, kn, vn = (torch.randn((B, H, T, D), generator=g).to(dtype).to(dev) for H in (Hkv * G, Hkv, Hkv))
    k0, v0, _ = cache_of(3410, dev, dtype, 0, False, B, Hkv, Smax, D)

    def tree(seed):
        parents = [tree_parents("random", T, seed + b) for b in range(B)]
        mask, depth = mm.tree_attention_mask(torch.tensor(parents, device=dev))
        assert torch.equal(mask.cpu(), mask_tensor([words_of(p) for p in parents], "cpu"))
        # the accepted path: the deepest node of item b and its ancestors, in order
        accept, counts = torch.zeros((B, T), dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        for b, p in enumerate(parents):
            node, path = max(range(T), key=lambda t: bin(words_of(p)[t]).count("1")), []
            while node >= 0:
                path.append(node)
                node = p[node]
            path.reverse()
            accept[b, :len(path)], counts[b] = torch.tensor(path, dtype=torch.int32), len(path)
        return mask, depth, accept.to(dev), counts.to(dev)

    mask, depth, accept, counts = tree(40)

    def step(lens, k, v):
        lens += T
        positions = (lens - T)[:, None] + depth
        qr = mm.rope_kv_cache_append(q, kn, vn, cos, sin, k, v, lens, positions=positions)
        out, lse = mm.block_sparse_attention_decode(qr, k, v, layout, lens, chunk=2, return_lse=True, tree_mask=mask)
        mm.kv_cache_compact(k, v, lens, accept, counts, T)
        lens -= T - counts
        return out, lse

    eager = (lens_tensor([100, 61], dev), k0.clone(), v0.clone())
    step(lens_tensor([100, 61], dev), k0.clone(), v0.clone())  # (the layout's record, the allocator's pools)
    held = (lens_tensor([100, 61], dev), k0.clone(), v0.clone())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    snapshot = [x.clone() for x in held]
    with torch.cuda.graph(graph):
        out, lse = step(*held)
    for x, s in zip(held, snapshot):  # (a capture runs nothing; the state is put back all the same)
        x.copy_(s)
    for turn, seed in enumerate((40, 50, 60)):
        for dst, src in zip((mask, depth, accept, counts), tree(seed)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        want = step(*eager)
        assert_same_bits(out, want[0], f"replay {turn}: out")
        assert_same_bits(lse, want[1], f"replay {turn}: lse")
        assert torch.equal(held[0], eager[0]), f"replay {turn}: lens"
        same_raw(held[1], eager[1], f"replay {turn}: k")
        same_raw(held[2], eager[2], f"replay {turn}: v")
