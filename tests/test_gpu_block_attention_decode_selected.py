"""matmuls.block_sparse_attention_decode_selected[_paged] on the GPU: the bits of the layout call on
hand-written lists, a long list, bounds → select → decode end to end against the dense causal layout, planted needles, one
captured graph of append → bounds → select → decode, and unseen memory."""
import pytest
import torch

from gpu_helpers import assert_same_bits
from test_gpu_block_attention_decode import SMAX, check_rule, lens_tensor, operands
from test_gpu_block_attention_decode_paged import gathered, paged

pytestmark = pytest.mark.gpu

NAN = float("nan")
WIDTHS = [32, 64, 96, 128]
K_SLOTS = 6
# (list, count): ascending; descending, with entries wholly beyond pos; with −1 (skipped inside its chunk); count 0 (the rest of
# the row is never looked at); a count beyond K is clamped
PATTERNS = [([0, 1, 2, 3, 4, 5], 6), ([7, 6, 5, 4, 3, 2], 6), ([2, -1, 0, 5, -1, 1], 6), ([3, 1, 4, 0, 2, 6], 0), ([1, 0, 3, 2, 6, 4], 9),
            ([4, 2, 0, -1, 1, 3], 3)]


def hand_lists(B, Hkv, T, dev, shift=0):
    ids = torch.empty((B, Hkv, T, K_SLOTS), dtype=torch.int32)
    counts = torch.empty((B, Hkv, T), dtype=torch.int32)
    for b in range(B):
        for h in range(Hkv):
            for t in range(T):
                lst, n = PATTERNS[(b * Hkv + h + t + shift) % len(PATTERNS)]
                ids[b, h, t], counts[b, h, t] = torch.tensor(lst), n
    return ids.to(dev), counts.to(dev)


def vis_of_lists(ids, counts, k_lens, T, smax=SMAX):
    """Boolean CPU mask [B, Hkv, T, Smax] from the rule alone: the first clamp(count, 0, K) entries inside the grid, keys ≤ pos."""
    ids, counts = ids.cpu(), counts.cpu()
    B, Hkv, _, K = ids.shape
    vis = torch.zeros(B, Hkv, T, smax, dtype=torch.bool)
    for b in range(B):
        for h in range(Hkv):
            for t in range(T):
                pos = min(max(k_lens[b], 0), smax) - T + t
                for J in ids[b, h, t, :max(0, min(int(counts[b, h, t]), K))].tolist():
                    if 0 <= J < smax // 64 and 64 * J <= pos:
                        vis[b, h, t, 64 * J:min(64 * J + 64, pos + 1)] = True
    return vis


def layout_of_token(ids, counts, k_lens, T, t, dev, smax=SMAX):
    """The equivalent (B, Hkv) layout of token t: row pos // 64 of item (b, h) holds its list in its order — a −1 as a block
    wholly beyond pos (both are skipped inside their chunk) —, the last row pads every item to one entry count."""
    ids, counts = ids.cpu(), counts.cpu()
    B, Hkv, _, K = ids.shape
    blocks = smax // 64
    crows, cols = [], []
    for b in range(B):
        for h in range(Hkv):
            pos = k_lens[b] - T + t
            assert 0 <= pos < 64 * (blocks - 1), "the last block is wholly beyond pos: it stands for −1"
            lst = [J if J >= 0 else blocks - 1 for J in ids[b, h, t, :max(0, min(int(counts[b, h, t]), K))].tolist()]
            row = [0] * (blocks + 1)
            for r in range(blocks):
                row[r + 1] = row[r] + (len(lst) if r == pos // 64 else K - len(lst) if r == blocks - 1 else 0)
            crows.append(row)
            cols.append(lst + list(range(K - len(lst))))
    crow = torch.tensor(crows, device=dev).reshape(B, Hkv, blocks + 1)
    col = torch.tensor(cols, device=dev).reshape(B, Hkv, K)
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.shape, device=dev), size=(B, Hkv, blocks, blocks))


def assert_bits_of_the_layout_calls(mm, what, out, lse, q, k, v, ids, counts, k_lens, chunk, dev):
    T = q.shape[2]
    for t in range(T):
        layout = layout_of_token(ids, counts, k_lens, T, t, dev)
        lens1 = lens_tensor([n - T + t + 1 for n in k_lens], dev)
        want = mm.block_sparse_attention_decode(q[:, :, t:t + 1].contiguous(), k, v, layout, lens1, chunk=chunk, return_lse=True)
        assert_same_bits(out[:, :, t:t + 1], want[0], f"{what}, token {t}, chunk {chunk}: out")
        assert_same_bits(lse[:, :, t:t + 1], want[1], f"{what}, token {t}, chunk {chunk}: lse")


# ---- 1. the bits of the layout call ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 5, 16])
@pytest.mark.parametrize("D", WIDTHS)
def test_1_hand_written_lists_have_the_bits_of_the_layout_call(mm, dev, D, G):
    B, Hkv = 2, 2
    dtype = torch.bfloat16 if (D // 32 + G) % 2 else torch.float16
    k_lens = [300, 131]
    for T in (1, 3):
        q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 9000 + D + G + T)
        ids, counts = hand_lists(B, Hkv, T, dev, shift=T)
        lens = lens_tensor(k_lens, dev)
        for chunk in (1, 2, 64):
            out, lse = mm.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, chunk=chunk, return_lse=True)
            assert out.dtype == dtype and not out.requires_grad
            assert_bits_of_the_layout_calls(mm, f"D={D} G={G} T={T}", out, lse, q, k, v, ids, counts, k_lens, chunk, dev)
        check_rule(f"lists D={D} G={G} T={T}", out, q, k, v, vis_of_lists(ids, counts, k_lens, T), G, lse)
        empty = (counts == 0).cpu()
        assert empty.any() and (out.cpu().reshape(B, Hkv, G, T, D).permute(0, 1, 3, 2, 4)[empty] == 0).all()


@pytest.mark.parametrize("page", [16, 128])
def test_1_the_paged_form_has_the_bits_of_the_contiguous_form(mm, dev, page):
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 5, 3, 96, torch.float16, [300, 131]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 9100 + page)
    ids, counts = hand_lists(B, Hkv, T, dev)
    lens = lens_tensor(k_lens, dev)
    kp, vp, table = paged(k, v, page, 11 + page)
    for chunk in (1, 2, 64):
        got = mm.block_sparse_attention_decode_selected_paged(q, kp, vp, table, ids, counts, lens, chunk=chunk, return_lse=True)
        want = mm.block_sparse_attention_decode_selected(q, gathered(kp, table), gathered(vp, table), ids, counts, lens, chunk=chunk,
                                                         return_lse=True)
        assert_same_bits(got[0], want[0], f"page {page}, chunk {chunk}: out")
        assert_same_bits(got[1], want[1], f"page {page}, chunk {chunk}: lse")
    assert_bits_of_the_layout_calls(mm, f"page {page}", got[0], got[1], q, k, v, ids, counts, k_lens, 64, dev)


# ---- 2. a long list ------------------------------------------------------------------------------------------------------------

def test_2_a_list_of_64_entries_in_chunks_of_four(mm, dev):
    B, Hkv, G, T, D, dtype, smax = 1, 2, 4, 1, 128, torch.bfloat16, 4096
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 9201, smax=smax)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(9202))
    ids = torch.stack([perm, perm.flip(0)]).reshape(B, Hkv, T, 64).to(torch.int32).to(dev)
    counts = torch.full((B, Hkv, T), 64, dtype=torch.int32, device=dev)
    lens = lens_tensor([smax], dev)
    out, lse = mm.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, chunk=4, return_lse=True)
    crow = torch.zeros((B, Hkv, 65), dtype=torch.int64)
    crow[..., 64] = 64                                              # row 63 holds the list, in its order
    layout = torch.sparse_csr_tensor(crow.to(dev), ids.reshape(B, Hkv, 64).long(), torch.ones((B, Hkv, 64), device=dev),
                                     size=(B, Hkv, 64, 64))
    want = mm.block_sparse_attention_decode(q, k, v, layout, lens, chunk=4, return_lse=True)
    assert_same_bits(out, want[0], "64 entries, chunk 4: out")
    assert_same_bits(lse, want[1], "64 entries, chunk 4: lse")
    assert torch.isfinite(out.float()).all()


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------

def causal_layout(blocks, dev):
    return torch.tril(torch.ones(blocks, blocks, device=dev)).to_sparse_csr()


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)])
def test_3_bounds_select_decode_with_every_candidate_is_the_dense_causal_call(mm, dev, D, dtype):
    B, Hkv, G, T, k_lens = 4, 2, 4, 3, [512, 200, 66, 2]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 9300 + D)
    lens = lens_tensor(k_lens, dev)
    bounds = mm.key_block_bounds(k, lens)
    ids, counts = mm.select_key_blocks(q, bounds, lens, 8)          # K ≥ candidates: every candidate, ascending
    out, lse = mm.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, chunk=2, return_lse=True)
    want = mm.block_sparse_attention_decode(q, k, v, causal_layout(8, dev), lens, chunk=2, return_lse=True)
    assert_same_bits(out, want[0], "every candidate: out")
    assert_same_bits(lse, want[1], "every candidate: lse")
    vis = torch.zeros(B, Hkv, T, SMAX, dtype=torch.bool)
    for b, n in enumerate(k_lens):
        for t in range(T):
            vis[b, :, t, :max(n - T + t + 1, 0)] = True
    check_rule(f"end to end D={D}", out, q, k, v, vis, G, lse)     # e_dev ≤ 8·e_ref against dense masked attention in float64


# ---- 4. planted needles ----------------------------------------------------------------------------------------------------------

def test_4_a_planted_key_brings_its_block_into_the_list(mm, dev):
    B, Hkv, G, T, D, dtype = 2, 2, 2, 1, 64, torch.bfloat16
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 9401)
    k = (k.float() * 0.05).to(dtype)                                # small-norm keys …
    needle = {(0, 0): 4 * 64 + 17, (0, 1): 2 * 64 + 63, (1, 0): 5 * 64, (1, 1): 3 * 64 + 40}
    for (b, h), j in needle.items():
        k[b, h, j] = q[b, h * G, 0]                                 # … and one key with q·k = |q|² ≈ D in a middle block
    lens = lens_tensor([512, 512], dev)
    bounds = mm.key_block_bounds(k, lens)
    ids, counts = mm.select_key_blocks(q, bounds, lens, 3, sink=1, local=1)
    assert (counts == 3).all()
    for (b, h), j in needle.items():
        assert ids[b, h, 0].tolist() == [0, j // 64, 7], (b, h, ids[b, h, 0].tolist())
    out, lse = mm.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, return_lse=True)
    check_rule("needles", out, q, k, v, vis_of_lists(ids, counts, [512, 512], T), G, lse)   # float64 attention over the three blocks


# ---- 5. one graph ------------------------------------------------------------------------------------------------------------------

def test_5_append_bounds_select_decode_in_one_graph(mm, dev):
    """One capture on one stream: kv_cache_append → key_block_bounds(last=1) → select_key_blocks →
    block_sparse_attention_decode_selected.  Before every replay k_lens, k_new, v_new and q are updated in place (item 0
    crosses from block 0 into block 1); the appended row and its block's bounds are spoilt after the eager run, so the
    replay has to redo them: out, lse, the lists and the bounds have the bits of the eager sequence."""
    B, Hkv, G, T, D, dtype = 2, 2, 4, 1, 64, torch.float16
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 9501)
    g = torch.Generator(device=dev).manual_seed(9502)
    k_new, v_new = (torch.randn((B, Hkv, T, D), device=dev, generator=g).to(dtype) for _ in range(2))
    lens = lens_tensor([62, 190], dev)
    bounds = mm.key_block_bounds(k, lens)

    def step():
        mm.kv_cache_append(k_new, v_new, k, v, lens)
        mm.key_block_bounds(k, lens, bounds, last=1)
        ids, counts = mm.select_key_blocks(q, bounds, lens, 3, sink=1, local=1)
        out, lse = mm.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, chunk=2, return_lse=True)
        return out, lse, ids, counts

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        captured = step()
    for i, host_lens in enumerate(([63, 191], [64, 192], [65, 193])):
        with torch.no_grad():
            lens += 1
            for x in (k_new, v_new, q):
                x.copy_(torch.randn(x.shape, device=dev, generator=g).to(dtype))
        assert lens.tolist() == host_lens
        want = [x.clone() for x in step()]
        want_bounds, want_k = bounds.clone(), k.clone()
        for b, n in enumerate(host_lens):                           # spoil what the graph has to redo
            k[b, :, n - 1], v[b, :, n - 1] = 0, 0
            bounds[b, :, (n - 1) // 64] = NAN
        for x in captured[:2]:
            x.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(captured[0], want[0], f"replay {i}: out")
        assert_same_bits(captured[1], want[1], f"replay {i}: lse")
        assert torch.equal(captured[2], want[2]) and torch.equal(captured[3], want[3]), f"replay {i}: the lists"
        assert_same_bits(k, want_k, f"replay {i}: the cache")
        for b, n in enumerate(host_lens):
            nb = (n + 63) // 64
            assert_same_bits(bounds[b, :, :nb], want_bounds[b, :, :nb], f"replay {i}: the bounds")
        assert torch.isfinite(captured[0].float()).all()


# ---- 6. unseen memory ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["BSHD", "pool"])
def test_6_nothing_outside_is_read(mm, dev, form):
    """NaN in every key no token sees — unlisted blocks, blocks beyond a row's count, positions beyond pos —, between the rows
    of a strided cache, and in the unreferenced pages of a pool: out is finite and has the bits of the clean contiguous call."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 2, 64, torch.float16, [300, 131]
    q, k, v = operands(dev, B, Hkv, G, T, D, dtype, 9601)
    ids, counts = hand_lists(B, Hkv, T, dev, shift=1)
    lens = lens_tensor(k_lens, dev)
    want = mm.block_sparse_attention_decode_selected(q, k, v, ids, counts, lens, chunk=2, return_lse=True)
    unseen = ~vis_of_lists(ids, counts, k_lens, T).any(2).to(dev)
    kx, vx = k.clone(), v.clone()
    kx[unseen], vx[unseen] = NAN, NAN
    if form == "BSHD":
        def strided(x):
            buf = torch.full((B, SMAX, Hkv, D + 8), NAN, device=dev, dtype=dtype)
            view = buf[..., :D].transpose(1, 2)
            view.copy_(x)
            return view
        ks, vs = strided(kx), strided(vx)
        assert not ks.is_contiguous()
        got = mm.block_sparse_attention_decode_selected(q, ks, vs, ids, counts, lens, chunk=2, return_lse=True)
    else:
        kp, vp, table = paged(kx, vx, 32, 97)
        got = mm.block_sparse_attention_decode_selected_paged(q, kp, vp, table, ids, counts, lens, chunk=2, return_lse=True)
    assert torch.isfinite(got[0].float()).all()
    assert_same_bits(got[0], want[0], f"{form}: out")
    assert_same_bits(got[1], want[1], f"{form}: lse")
