"""matmuls.block_sparse_attention_decode_selected[_paged]_fp8 on the GPU: the bits of the fp8 layout call on
hand-written lists, of the 2-byte selected call on the widened cache, the paged form, a long list, kv_to_fp8 → bounds → select
→ decode end to end against the dense causal layout, planted needles, one captured graph of append → bounds → select → decode,
and unseen memory."""
import pytest
import torch

from gpu_helpers import assert_same_bits
from test_gpu_block_attention_decode import SMAX, check_rule, lens_tensor
from test_gpu_block_attention_decode_fp8 import F8, NANB, codes, fp8, pools, queries, same, wide
from test_gpu_block_attention_decode_paged import gathered
from test_gpu_block_attention_decode_selected import causal_layout, hand_lists, layout_of_token, vis_of_lists

pytestmark = pytest.mark.gpu

NAN = float("nan")
WIDTHS = [32, 64, 96, 128]


def head_scales(dev, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    ks, vs = (0.25 + 2.0 * torch.rand(Hkv, generator=g) for _ in range(2))   # per head, no powers of two
    return ks.to(dev), vs.to(dev)


def assert_bits_of_the_fp8_layout_calls(mm, what, got, q, k8, v8, ids, counts, k_lens, chunk, dev, **scales):
    T = q.shape[2]
    for t in range(T):
        layout = layout_of_token(ids, counts, k_lens, T, t, dev)
        lens1 = lens_tensor([n - T + t + 1 for n in k_lens], dev)
        want = mm.block_sparse_attention_decode_fp8(q[:, :, t:t + 1].contiguous(), k8, v8, layout, lens1, chunk=chunk, return_lse=True,
                                                    **scales)
        same((got[0][:, :, t:t + 1], got[1][:, :, t:t + 1]), want, f"{what}, token {t}, chunk {chunk}")


def dequantised(c, s):
    """CPU codes times the per-head scales in float64: the cache the call stands for."""
    return c.view(F8).to(torch.float32).double() * s.cpu().double().reshape(1, -1, 1, 1)


# ---- 1. the bits of the fp8 layout call ------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 5, 16])
@pytest.mark.parametrize("D", WIDTHS)
def test_1_hand_written_lists_have_the_bits_of_the_fp8_layout_call(mm, dev, D, G):
    B, Hkv = 2, 2
    dtype = torch.bfloat16 if (D // 32 + G) % 2 else torch.float16
    k_lens = [300, 131]
    kc, vc = codes(3301 + D + G, B, Hkv, SMAX, D), codes(3302 + D + G, B, Hkv, SMAX, D)
    k8, v8 = fp8(kc, dev), fp8(vc, dev)
    ks, vs = head_scales(dev, Hkv, 3303 + D + G)
    lens = lens_tensor(k_lens, dev)
    for T in (1, 3):
        q = queries(3304 + D + G + T, dev, B, Hkv * G, T, D, dtype)
        ids, counts = hand_lists(B, Hkv, T, dev, shift=T)
        for chunk in (1, 2, 64):
            got = mm.block_sparse_attention_decode_selected_fp8(q, k8, v8, ids, counts, lens, k_scale=ks, v_scale=vs, chunk=chunk,
                                                                return_lse=True)
            assert got[0].dtype == dtype and not got[0].requires_grad and got[1].dtype == torch.float32
            assert_bits_of_the_fp8_layout_calls(mm, f"D={D} G={G} T={T}", got, q, k8, v8, ids, counts, k_lens, chunk, dev,
                                                k_scale=ks, v_scale=vs)
        check_rule(f"fp8 lists D={D} G={G} T={T}", got[0], q, dequantised(kc, ks), dequantised(vc, vs),
                   vis_of_lists(ids, counts, k_lens, T), G, got[1])
        empty = (counts == 0).cpu()
        assert empty.any() and (got[0].cpu().reshape(B, Hkv, G, T, D).permute(0, 1, 3, 2, 4)[empty] == 0).all()


# ---- 2. without scales: the 2-byte selected call on the widened cache ------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_2_without_scales_the_bits_of_the_selected_call_on_the_widened_cache(mm, dev, dtype):
    B, Hkv, G, T, D, k_lens = 2, 2, 4, 3, 64, [300, 131]
    q = queries(3310, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(3311, B, Hkv, SMAX, D), codes(3312, B, Hkv, SMAX, D)
    ids, counts = hand_lists(B, Hkv, T, dev)
    lens = lens_tensor(k_lens, dev)
    for chunk in (1, 2, 64):
        got = mm.block_sparse_attention_decode_selected_fp8(q, fp8(kc, dev), fp8(vc, dev), ids, counts, lens, chunk=chunk, return_lse=True)
        want = mm.block_sparse_attention_decode_selected(q, wide(kc, dtype, dev), wide(vc, dtype, dev), ids, counts, lens, chunk=chunk,
                                                         return_lse=True)
        same(got, want, f"{dtype}, chunk {chunk}")
    default = mm.block_sparse_attention_decode_selected_fp8(q, fp8(kc, dev), fp8(vc, dev), ids, counts, lens)
    assert_same_bits(default, got[0], "chunk=None: one chunk over six slots")


# ---- 3. paged ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [16, 128])
def test_3_the_paged_form_has_the_bits_of_the_contiguous_form(mm, dev, page):
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 5, 3, 96, torch.float16, [300, 131]
    q = queries(3320 + page, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(3321 + page, B, Hkv, SMAX, D), codes(3322 + page, B, Hkv, SMAX, D)
    kp, vp, table = pools(kc, vc, page, 3323 + page)
    ks, vs = head_scales(dev, Hkv, 3324)
    ids, counts = hand_lists(B, Hkv, T, dev)
    lens = lens_tensor(k_lens, dev)
    for chunk in (1, 2, 64):
        got = mm.block_sparse_attention_decode_selected_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), ids, counts, lens,
                                                                  k_scale=ks, v_scale=vs, chunk=chunk, return_lse=True)
        want = mm.block_sparse_attention_decode_selected_fp8(q, fp8(gathered(kp, table), dev), fp8(gathered(vp, table), dev), ids, counts,
                                                             lens, k_scale=ks, v_scale=vs, chunk=chunk, return_lse=True)
        same(got, want, f"page {page}, chunk {chunk}")
    assert_bits_of_the_fp8_layout_calls(mm, f"page {page}", got, q, fp8(kc, dev), fp8(vc, dev), ids, counts, k_lens, 64, dev,
                                        k_scale=ks, v_scale=vs)


# ---- 4. a long list --------------------------------------------------------------------------------------------------------------

def test_4_a_list_of_64_entries_in_chunks_of_four(mm, dev):
    B, Hkv, G, T, D, dtype, smax = 1, 2, 4, 1, 128, torch.bfloat16, 4096
    q = queries(3330, dev, B, Hkv * G, T, D, dtype)
    k8, v8 = fp8(codes(3331, B, Hkv, smax, D), dev), fp8(codes(3332, B, Hkv, smax, D), dev)
    ks, vs = head_scales(dev, Hkv, 3333)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(3334))
    ids = torch.stack([perm, perm.flip(0)]).reshape(B, Hkv, T, 64).to(torch.int32).to(dev)
    counts = torch.full((B, Hkv, T), 64, dtype=torch.int32, device=dev)
    lens = lens_tensor([smax], dev)
    got = mm.block_sparse_attention_decode_selected_fp8(q, k8, v8, ids, counts, lens, k_scale=ks, v_scale=vs, chunk=4, return_lse=True)
    crow = torch.zeros((B, Hkv, 65), dtype=torch.int64)
    crow[..., 64] = 64                                              # row 63 holds the list, in its order
    layout = torch.sparse_csr_tensor(crow.to(dev), ids.reshape(B, Hkv, 64).long(), torch.ones((B, Hkv, 64), device=dev),
                                     size=(B, Hkv, 64, 64))
    want = mm.block_sparse_attention_decode_fp8(q, k8, v8, layout, lens, k_scale=ks, v_scale=vs, chunk=4, return_lse=True)
    same(got, want, "64 entries, chunk 4")
    assert torch.isfinite(got[0].float()).all()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------

def real_cache(seed, B, Hkv, D, smax=SMAX):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, Hkv, smax, D), generator=g) for _ in range(2))


@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)])
def test_5_quantise_bounds_select_decode_with_every_candidate_is_the_dense_causal_fp8_call(mm, dev, D, dtype):
    B, Hkv, G, T, k_lens = 4, 2, 4, 3, [512, 200, 66, 2]
    q = queries(3340 + D, dev, B, Hkv * G, T, D, dtype)
    k, v = real_cache(3341 + D, B, Hkv, D)
    (k8, ks), (v8, vs) = mm.kv_to_fp8(k.to(dev)), mm.kv_to_fp8(v.to(dev))
    lens = lens_tensor(k_lens, dev)
    bounds = mm.key_block_bounds_fp8(k8, lens, dtype=dtype)
    ids, counts = mm.select_key_blocks(q, bounds, lens, 8)          # K ≥ candidates: every candidate, ascending
    got = mm.block_sparse_attention_decode_selected_fp8(q, k8, v8, ids, counts, lens, k_scale=ks, v_scale=vs, chunk=2, return_lse=True)
    want = mm.block_sparse_attention_decode_fp8(q, k8, v8, causal_layout(8, dev), lens, k_scale=ks, v_scale=vs, chunk=2, return_lse=True)
    same(got, want, "every candidate")
    vis = torch.zeros(B, Hkv, T, SMAX, dtype=torch.bool)
    for b, n in enumerate(k_lens):
        for t in range(T):
            vis[b, :, t, :max(n - T + t + 1, 0)] = True
    kd, vd = dequantised(k8.cpu().view(torch.uint8), ks), dequantised(v8.cpu().view(torch.uint8), vs)
    check_rule(f"fp8 end to end D={D}", got[0], q, kd, vd, vis, G, got[1])   # e_dev ≤ 8·e_ref against float64 on the scaled cache


# ---- 6. planted needles ------------------------------------------------------------------------------------------------------------

def test_6_a_planted_key_brings_its_block_into_the_list(mm, dev):
    B, Hkv, G, T, D, dtype = 2, 2, 2, 1, 64, torch.bfloat16
    q = queries(3350, torch.device("cpu"), B, Hkv * G, T, D, dtype)
    k, v = real_cache(3351, B, Hkv, D)
    k = k * 0.05                                                    # small-norm keys …
    needle = {(0, 0): 4 * 64 + 17, (0, 1): 2 * 64 + 63, (1, 0): 5 * 64, (1, 1): 3 * 64 + 40}
    for (b, h), j in needle.items():
        k[b, h, j] = q[b, h * G, 0].float()                         # … and one key with q·k = |q|² ≈ D in a middle block
    (k8, ks), (v8, vs) = mm.kv_to_fp8(k), mm.kv_to_fp8(v)           # torch ops: on the CPU here
    # on the CPU, from the widened bounds: the needle block's score exceeds every other unforced candidate's (by a factor ≥ 2
    # with these seeds; the forced blocks are 0 — sink — and 7 — local)
    wide_k = k8.to(dtype).double().reshape(B, Hkv, 8, 64, D)
    lo, hi = wide_k.amin(3), wide_k.amax(3)
    for (b, h), j in needle.items():
        qg = q[b, h * G:(h + 1) * G, 0].double()                    # [G, D]
        score = torch.maximum(qg[:, None] * lo[b, h][None], qg[:, None] * hi[b, h][None]).sum(-1).amax(0)   # [8]
        others = [float(score[J]) for J in range(1, 7) if J != j // 64]
        assert float(score[j // 64]) > 2 * max(others) > 0, (b, h, float(score[j // 64]), others)
    q, k8, v8, ks, vs = (x.to(dev) for x in (q, k8, v8, ks, vs))
    lens = lens_tensor([512, 512], dev)
    bounds = mm.key_block_bounds_fp8(k8, lens, dtype=dtype)
    ids, counts = mm.select_key_blocks(q, bounds, lens, 3, sink=1, local=1)
    assert (counts == 3).all()
    for (b, h), j in needle.items():
        assert ids[b, h, 0].tolist() == [0, j // 64, 7], (b, h, ids[b, h, 0].tolist())
    got = mm.block_sparse_attention_decode_selected_fp8(q, k8, v8, ids, counts, lens, k_scale=ks, v_scale=vs, return_lse=True)
    kd, vd = dequantised(k8.cpu().view(torch.uint8), ks), dequantised(v8.cpu().view(torch.uint8), vs)
    check_rule("fp8 needles", got[0], q, kd, vd, vis_of_lists(ids, counts, [512, 512], T), G, got[1])


# ---- 7. one graph --------------------------------------------------------------------------------------------------------------------

def test_7_append_bounds_select_decode_in_one_graph(mm, dev):
    """One capture on one stream: kv_cache_append into the fp8 cache → key_block_bounds_fp8(last=1) → select_key_blocks →
    block_sparse_attention_decode_selected_fp8.  Before every replay k_lens, k_new, v_new, q and the two scale tensors are
    updated in place (item 0 crosses from block 0 into block 1); the appended row and its block's bounds are spoilt after the
    eager run, so the replay has to redo them: out, lse, the lists, the bounds and the cache bytes are the eager sequence's."""
    B, Hkv, G, T, D, dtype = 2, 2, 4, 1, 64, torch.float16
    q = queries(3360, dev, B, Hkv * G, T, D, dtype)
    k8, v8 = fp8(codes(3361, B, Hkv, SMAX, D), dev), fp8(codes(3362, B, Hkv, SMAX, D), dev)
    g = torch.Generator(device=dev).manual_seed(3363)
    k_new, v_new = (torch.randn((B, Hkv, T, D), device=dev, generator=g).to(dtype) for _ in range(2))
    ks, vs = torch.tensor([0.011, 0.013], device=dev), torch.tensor([0.012, 0.009], device=dev)
    lens = lens_tensor([62, 190], dev)
    bounds = mm.key_block_bounds_fp8(k8, lens, dtype=dtype)

    def step():
        mm.kv_cache_append(k_new, v_new, k8, v8, lens, k_scale=ks, v_scale=vs)
        mm.key_block_bounds_fp8(k8, lens, bounds, last=1)
        ids, counts = mm.select_key_blocks(q, bounds, lens, 3, sink=1, local=1)
        out, lse = mm.block_sparse_attention_decode_selected_fp8(q, k8, v8, ids, counts, lens, k_scale=ks, v_scale=vs, chunk=2,
                                                                 return_lse=True)
        return out, lse, ids, counts

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        captured = step()
    kb, vb = k8.view(torch.uint8), v8.view(torch.uint8)
    for i, host_lens in enumerate(([63, 191], [64, 192], [65, 193])):
        with torch.no_grad():
            lens += 1
            for x in (k_new, v_new, q):
                x.copy_(torch.randn(x.shape, device=dev, generator=g).to(dtype))
            ks.mul_(1.25)
            vs.mul_(0.75)
        assert lens.tolist() == host_lens
        want = [x.clone() for x in step()]
        want_bounds, want_k, want_v = bounds.clone(), kb.clone(), vb.clone()
        for b, n in enumerate(host_lens):                           # spoil what the graph has to redo
            kb[b, :, n - 1], vb[b, :, n - 1] = NANB, NANB
            bounds[b, :, (n - 1) // 64] = NAN
        for x in captured[:2]:
            x.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        same(captured[:2], want[:2], f"replay {i}")
        assert torch.equal(captured[2], want[2]) and torch.equal(captured[3], want[3]), f"replay {i}: the lists"
        assert torch.equal(kb, want_k) and torch.equal(vb, want_v), f"replay {i}: the cache bytes"
        for b, n in enumerate(host_lens):
            nb = (n + 63) // 64
            assert_same_bits(bounds[b, :, :nb], want_bounds[b, :, :nb], f"replay {i}: the bounds")
        assert torch.isfinite(captured[0].float()).all()


# ---- 8. unseen memory ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["BSHD", "pool"])
def test_8_nothing_outside_is_read(mm, dev, form):
    """The NaN code in every key no token sees — unlisted blocks, blocks beyond a row's count, positions beyond pos —, between
    the rows of a strided cache, and in the unreferenced pages of a pool: out is finite and has the bits of the clean call."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 2, 64, torch.float16, [300, 131]
    q = queries(3370, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(3371, B, Hkv, SMAX, D), codes(3372, B, Hkv, SMAX, D)
    ks, vs = head_scales(dev, Hkv, 3373)
    ids, counts = hand_lists(B, Hkv, T, dev, shift=1)
    lens = lens_tensor(k_lens, dev)
    want = mm.block_sparse_attention_decode_selected_fp8(q, fp8(kc, dev), fp8(vc, dev), ids, counts, lens, k_scale=ks, v_scale=vs, chunk=2,
                                                         return_lse=True)
    unseen = ~vis_of_lists(ids, counts, k_lens, T).any(2)
    kx, vx = kc.clone(), vc.clone()
    kx[unseen], vx[unseen] = NANB, NANB
    if form == "BSHD":
        def strided(x):
            buf = torch.full((B, SMAX, Hkv, D + 16), NANB, device=dev, dtype=torch.uint8)
            view = buf[..., :D].transpose(1, 2)
            view.copy_(x.to(dev))
            return view.view(F8)
        k8, v8 = strided(kx), strided(vx)
        assert not k8.is_contiguous()
        got = mm.block_sparse_attention_decode_selected_fp8(q, k8, v8, ids, counts, lens, k_scale=ks, v_scale=vs, chunk=2, return_lse=True)
    else:
        kp, vp, table = pools(kx, vx, 32, 3374)
        got = mm.block_sparse_attention_decode_selected_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), ids, counts, lens,
                                                                  k_scale=ks, v_scale=vs, chunk=2, return_lse=True)
    assert torch.isfinite(got[0].float()).all()
    same(got, want, form)
