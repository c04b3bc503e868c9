"""matmuls.block_sparse_attention_decode_fp8 and block_sparse_attention_decode_paged_fp8 on the MI355X:
the decode calls over an OCP e4m3fn cache with per-head scales.  The contract is on bits: without scales the call is the
2-byte call on the cache widened to q's type (widened HERE on the CPU, where the cast is known to be exact); with a uniform
k_scale s and v_scale 2^n it is that call at scale' = fl32(scale · s), times 2^n; the paged call is the contiguous one on
the gathered cache.  Accuracy where scales are no powers of two is the project's rule e_dev ≤ 8 · e_ref on the dequantised
operands.  fp8 data is made from bytes on the CPU and written through uint8 views: no fp8 operator of torch runs on the
device.  The NaN code 0x7F stands wherever nothing may be read.

Smax = 512, B · Hkv ≤ 8, chunk=2 unless stated.  Long lists (64 entries, up to 16 turns per wave) live in
tests/test_gpu_block_attention_decode_long.py."""
import ctypes

import pytest
import torch

from gpu_helpers import SENTINEL, assert_outside_untouched, assert_same_bits, padded
from test_gpu_block_attention_decode import ROWS, SMAX, check_rule, layout_from_rows, lens_tensor, visible
from test_gpu_block_attention_decode_paged import gathered, scatter

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
NANB = 0x7F
NAN = float("nan")
WIDTHS = [32, 64, 96, 128]
FINITE = torch.tensor([c for c in range(256) if c & 0x7F != NANB], dtype=torch.uint8)  # the 254 finite codes


def codes(seed, *shape):
    """Random finite e4m3fn codes with |x| < 4 (subnormals, ±0 included), uint8 on the CPU."""
    small = FINITE[(FINITE & 0x7F) < 0x48]
    return small[torch.randint(len(small), shape, generator=torch.Generator().manual_seed(seed))]


def queries(seed, dev, B, Hq, T, D, dtype):
    return torch.randn((B, Hq, T, D), generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


def wide(c, dtype, dev):
    """CPU codes widened to `dtype` on the CPU — exact — and moved to the device: the operand of the 2-byte call."""
    return c.view(F8).to(dtype).to(dev)


def fp8(c, dev):
    return c.to(dev).view(F8)


def poisoned(c, vis):
    """A copy of the codes [B, Hkv, Smax, D] with the NaN code in every key no token of its item sees."""
    c = c.clone()
    c[~vis.any(2)] = NANB
    return c


def pools(kc, vc, page, seed, extra=3):
    """(k pool, v pool, table), uint8 / int32 on the CPU: the caches' pages shuffled into P = B · W + extra pages, the
    unreferenced ones full of the NaN code."""
    B, Hkv, smax, D = kc.shape
    W = smax // page
    P = B * W + extra
    table = torch.randperm(P, generator=torch.Generator().manual_seed(seed))[:B * W].reshape(B, W).to(torch.int32)
    out = []
    for x in (kc, vc):
        pool = torch.full((P, Hkv, page, D), NANB, dtype=torch.uint8)
        scatter(pool, table, x)
        out.append(pool)
    return out[0], out[1], table


def same(got, want, what):
    assert_same_bits(got[0], want[0], f"{what}: out")
    assert_same_bits(got[1], want[1], f"{what}: lse")


# ---- 1. the bits of the widened call, contiguous ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", WIDTHS)
def test_1_the_bits_of_the_call_on_the_widened_cache(mm, dev, dtype, D):
    B, Hkv, G, T, k_lens = 2, 2, 4, 1, [512, 200]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2210 + D, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(2211 + D, B, Hkv, SMAX, D), codes(2212 + D, B, Hkv, SMAX, D)
    got = mm.block_sparse_attention_decode_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, chunk=2, return_lse=True)
    assert got[0].dtype == dtype and not got[0].requires_grad and got[1].dtype == torch.float32
    kw, vw = wide(kc, dtype, dev), wide(vc, dtype, dev)
    same(got, mm.block_sparse_attention_decode(q, kw, vw, layout, lens, chunk=2, return_lse=True), f"{dtype} D={D}")
    check_rule(f"fp8 {dtype} D={D}", got[0], q, kw, vw, visible([ROWS], B, Hkv, T, k_lens), G, got[1])
    one_chunk = mm.block_sparse_attention_decode_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, chunk=8, return_lse=True)
    same(one_chunk, mm.block_sparse_attention_decode(q, kw, vw, layout, lens, chunk=8, return_lse=True), "one chunk: no combine launch")


# ---- 2. … paged -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page,D,dtype", [(page, D, (torch.bfloat16, torch.float16)[(i + j) % 2])
                                          for i, page in enumerate([16, 64, 256]) for j, D in enumerate(WIDTHS)])
def test_2_the_paged_call_has_the_bits_of_the_widened_and_of_the_contiguous_call(mm, dev, page, D, dtype):
    B, Hkv, G, T, k_lens = 2, 2, 4, 1, [512, 200]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2220 + D + page, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(2221 + D + page, B, Hkv, SMAX, D), codes(2222 + D + page, B, Hkv, SMAX, D)
    kp, vp, table = pools(kc, vc, page, 2223 + page)
    assert torch.equal(gathered(kp, table), kc)
    tab = table.to(dev)
    got = mm.block_sparse_attention_decode_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), tab, layout, lens, chunk=2, return_lse=True)
    widened = mm.block_sparse_attention_decode_paged(q, wide(kp, dtype, dev), wide(vp, dtype, dev), tab, layout, lens, chunk=2,
                                                     return_lse=True)
    same(got, widened, f"page {page} D={D} {dtype}: the 2-byte paged call on the widened pool")
    flat = mm.block_sparse_attention_decode_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, chunk=2, return_lse=True)
    same(got, flat, f"page {page} D={D} {dtype}: the contiguous fp8 call on the gathered cache")
    assert torch.isfinite(got[0].float()).all()


# ---- 3. every code ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("which", ["v", "k"])
def test_3_every_finite_code_in_k_and_in_v(mm, dev, which, D, dtype):
    """One operand cycles through the 254 finite codes (±0, the subnormals, ±448; neighbours in a row differ), the other is
    random; k_scale is a power of two, so the call must have the bits of the 2-byte call at scale · k_scale.  The softmax
    is far from one-hot (asserted on the float64 probabilities): a wrong value anywhere moves the result."""
    B, Hkv, G, T, k_lens = 2, 2, 4, 1, [512, 200]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2230 + D, dev, B, Hkv * G, T, D, dtype)
    cycle = FINITE[(torch.arange(B * Hkv * SMAX * D) + 3) % 254].reshape(B, Hkv, SMAX, D)
    assert len(set(cycle[0, 0, :8].flatten().tolist())) == 254
    rand = codes(2231 + D, B, Hkv, SMAX, D)
    kc, vc, ks = (rand, cycle, 0.5) if which == "v" else (cycle, rand, 2.0 ** -9)
    scale = float(torch.tensor(1.0 / D ** 0.5, dtype=torch.float32) * torch.tensor(ks, dtype=torch.float32))
    vis = visible([ROWS], B, Hkv, T, k_lens)
    s = scale * (q.cpu().double() @ kc.view(F8).to(torch.float32).double().repeat_interleave(G, 1).transpose(-1, -2))
    p = torch.softmax(s.masked_fill(~vis.repeat_interleave(G, 1), -float("inf")), -1)
    print(f"every code in {which}, D={D}: largest probability {float(p.max()):.3f}")
    assert float(p.max()) <= 0.5
    got = mm.block_sparse_attention_decode_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, k_scale=torch.tensor(ks, device=dev),
                                               chunk=2, return_lse=True)
    want = mm.block_sparse_attention_decode(q, wide(kc, dtype, dev), wide(vc, dtype, dev), layout, lens, scale=scale, chunk=2,
                                            return_lse=True)
    same(got, want, f"every code in {which}, {dtype} D={D}")
    assert torch.isfinite(got[0].float()).all()


# ---- 4. scales -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float16, 64)])
def test_4_scales(mm, dev, dtype, D):
    B, Hkv, G, T, k_lens = 2, 2, 4, 2, [512, 200]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2240 + D, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(2241 + D, B, Hkv, SMAX, D), codes(2242 + D, B, Hkv, SMAX, D)
    k8, v8, kw, vw = fp8(kc, dev), fp8(vc, dev), wide(kc, dtype, dev), wide(vc, dtype, dev)
    # one k_scale for all heads and v_scale a power of two: the 2-byte call at fl32(scale · 0.37), times 0.5 — bit for bit.
    # The values here are positive codes of at least 0.125, so every output (a weighted mean of them) and its half are
    # normal numbers of both types: halving the rounded result is exact and commutes with the rounding at the store.
    vp = (vc & 0x7F).clamp(min=0x20)
    v8p, vwp = fp8(vp, dev), wide(vp, dtype, dev)
    got = mm.block_sparse_attention_decode_fp8(q, k8, v8p, layout, lens, k_scale=torch.tensor(0.37, device=dev),
                                               v_scale=torch.tensor(0.5, device=dev), chunk=2, return_lse=True)
    scale = float(torch.tensor(1.0 / D ** 0.5, dtype=torch.float32) * torch.tensor(0.37, dtype=torch.float32))
    want = mm.block_sparse_attention_decode(q, kw, vwp, layout, lens, scale=scale, chunk=2, return_lse=True)
    assert float(want[0].float().abs().min()) >= 0.125
    assert_same_bits(got[0], (want[0].float() * 0.5).to(dtype), "k_scale 0.37, v_scale 0.5: out")
    assert_same_bits(got[1], want[1], "k_scale 0.37, v_scale 0.5: lse")
    # a float and the equal 0-d tensor; a (1,) tensor
    as_float = mm.block_sparse_attention_decode_fp8(q, k8, v8p, layout, lens, k_scale=0.37, v_scale=0.5, chunk=2, return_lse=True)
    same(as_float, got, "scales given as floats")
    one = mm.block_sparse_attention_decode_fp8(q, k8, v8p, layout, lens, k_scale=torch.tensor([0.37], device=dev), v_scale=0.5,
                                               chunk=2, return_lse=True)
    same(one, got, "k_scale of shape (1,)")
    # per head, no power of two: the rule against float64 on the dequantised operands, lse to 1e-5
    ks, vs = torch.tensor([0.37, 1.9]), torch.tensor([0.11, 3.3])
    per_head = mm.block_sparse_attention_decode_fp8(q, k8, v8, layout, lens, k_scale=ks.to(dev), v_scale=vs.to(dev), chunk=2,
                                                    return_lse=True)
    kd, vd = (c.view(F8).to(torch.float32).double() * s.double().reshape(1, Hkv, 1, 1) for c, s in ((kc, ks), (vc, vs)))
    check_rule(f"per-head scales {dtype} D={D}", per_head[0], q, kd, vd, visible([ROWS], B, Hkv, T, k_lens), G, per_head[1])
    # each head follows its own scale: head 0 alone with its scales as 0-d tensors
    alone = mm.block_sparse_attention_decode_fp8(q[:, :G], k8[:, :1], v8[:, :1], layout, lens, k_scale=0.37, v_scale=0.11, chunk=2,
                                                 return_lse=True)
    same((per_head[0][:, :G], per_head[1][:, :G]), alone, "k / v head 0 under its own scales")
    # … and the paged form takes the same scales
    kp, vp, table = pools(kc, vc, 32, 2243)
    paged = mm.block_sparse_attention_decode_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, k_scale=ks.to(dev),
                                                       v_scale=vs.to(dev), chunk=2, return_lse=True)
    same(paged, per_head, "the paged call with per-head scales")


# ---- 5. nothing outside is read ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["BHSD", "BSHD"])
def test_5_nothing_outside_the_cache_is_read(mm, dev, form):
    """The NaN code in every key no token sees and between the rows (row stride D + 16 in a buffer of 0x7F)."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 2, 64, torch.float16, [130, 449]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2250, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(2251, B, Hkv, SMAX, D), codes(2252, B, Hkv, SMAX, D)
    vis = visible([ROWS], B, Hkv, T, k_lens)

    def strided(c):
        shape = (B, Hkv, SMAX, D + 16) if form == "BHSD" else (B, SMAX, Hkv, D + 16)
        buf = torch.full(shape, NANB, device=dev, dtype=torch.uint8)
        view = buf[..., :D] if form == "BHSD" else buf[..., :D].transpose(1, 2)
        view.copy_(poisoned(c, vis).to(dev))
        return view.view(F8)

    ks, vs = strided(kc), strided(vc)
    assert not ks.is_contiguous() and ks.stride(2) >= D + 16 and ks.shape == (B, Hkv, SMAX, D)
    ptrs = (ks.data_ptr(), vs.data_ptr())
    got = mm.block_sparse_attention_decode_fp8(q, ks, vs, layout, lens, k_scale=0.5, chunk=2, return_lse=True)
    assert (ks.data_ptr(), vs.data_ptr()) == ptrs
    check_rule(f"poisoned {form} fp8 cache", got[0], q, wide(kc, dtype, dev) * 0.5, wide(vc, dtype, dev), vis, G, got[1])
    clone = mm.block_sparse_attention_decode_fp8(q, fp8(poisoned(kc, vis), dev), fp8(poisoned(vc, vis), dev), layout, lens, k_scale=0.5,
                                                 chunk=2, return_lse=True)
    same(got, clone, f"{form}: the strided cache against a contiguous clone")


@pytest.mark.parametrize("page", [16, 128])
@pytest.mark.parametrize("form", ["PHSD", "PSHD"])
def test_5_nothing_outside_the_pool_is_read(mm, dev, form, page):
    """… and in every unreferenced page; the table entries of logical pages wholly beyond pos are −1 and P + 5."""
    B, Hkv, G, T, D, dtype, k_lens = 2, 2, 4, 2, 64, torch.bfloat16, [130, 449]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2253 + page, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(2254 + page, B, Hkv, SMAX, D), codes(2255 + page, B, Hkv, SMAX, D)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    kp, vp, table = pools(poisoned(kc, vis), poisoned(vc, vis), page, 2256 + page)
    W, P = table.shape[1], kp.shape[0]

    def strided(pool):
        shape = (P, Hkv, page, D + 16) if form == "PHSD" else (P, page, Hkv, D + 16)
        buf = torch.full(shape, NANB, device=dev, dtype=torch.uint8)
        view = buf[..., :D] if form == "PHSD" else buf[..., :D].transpose(1, 2)
        view.copy_(pool.to(dev))
        return view.view(F8)

    ks, vs = strided(kp), strided(vp)
    assert not ks.is_contiguous() and ks.shape == (P, Hkv, page, D)
    beyond = [(b, lp) for b in range(B) for lp in range(W) if lp * page > k_lens[b] - 1]
    assert len(beyond) >= 2
    for i, (b, lp) in enumerate(beyond):
        table[b, lp] = (-1, P + 5)[i % 2]
    tab = table.to(dev)
    ptrs = (ks.data_ptr(), vs.data_ptr(), tab.data_ptr())
    got = mm.block_sparse_attention_decode_paged_fp8(q, ks, vs, tab, layout, lens, v_scale=2.0, chunk=2, return_lse=True)
    assert (ks.data_ptr(), vs.data_ptr(), tab.data_ptr()) == ptrs
    check_rule(f"poisoned {form} fp8 pool, page {page}", got[0], q, wide(kc, dtype, dev), wide(vc, dtype, dev) * 2, vis, G, got[1])
    clone = mm.block_sparse_attention_decode_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), tab, layout, lens, v_scale=2.0, chunk=2,
                                                       return_lse=True)
    same(got, clone, f"{form}: the strided pool against a contiguous clone")


@pytest.mark.parametrize("page", [16, 128])
def test_5_invalid_entries_hide_their_keys(mm, dev, page):
    """Seen logical pages carry −1 or P; the pool pages they named before are full of the NaN code.  The rule holds with
    those keys removed from the mask; the item whose entries are all invalid gives zero rows and lse −inf."""
    B, Hkv, G, T, D, dtype, k_lens = 3, 2, 4, 2, 64, torch.bfloat16, [512, 200, 300]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2257 + page, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(2258 + page, B, Hkv, SMAX, D), codes(2259 + page, B, Hkv, SMAX, D)
    kp, vp, table = pools(kc, vc, page, 2260 + page)
    P = kp.shape[0]
    vis = visible([ROWS], B, Hkv, T, k_lens)
    for b, lp, entry in [(0, 100 // page, -1), (0, 400 // page, P), (1, 70 // page, P), (1, 195 // page, -1)]:
        assert vis[b, :, :, lp * page:(lp + 1) * page].any(), "a page with seen keys"
        kp[int(table[b, lp])] = NANB
        vp[int(table[b, lp])] = NANB
        table[b, lp] = entry
        vis[b, :, :, lp * page:(lp + 1) * page] = False
    table[2] = torch.tensor([-1, P, P + 7, -2 ** 31] * (table.shape[1] // 4), dtype=torch.int32)
    vis[2] = False
    got = mm.block_sparse_attention_decode_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, chunk=2, return_lse=True)
    check_rule(f"hidden fp8 pages, page {page}", got[0], q, wide(kc, dtype, dev), wide(vc, dtype, dev), vis, G, got[1])
    assert (got[0][2] == 0).all() and (got[1][2] == -float("inf")).all() and torch.isfinite(got[1][0]).all()
    assert torch.equal(torch.isfinite(got[1]).cpu(), vis.any(-1).repeat_interleave(G, 1))  # (page 128 hides all of item 1)
    empty = mm.block_sparse_attention_decode_paged_fp8(q, fp8(kp[:0], dev), fp8(vp[:0], dev), table.to(dev), layout, lens, chunk=2,
                                                       return_lse=True)
    assert (empty[0] == 0).all() and (empty[1] == -float("inf")).all()


# ---- 6. groups, tokens, the batch ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 5, 16])
def test_6_group_sizes_and_three_tokens_across_a_block_boundary(mm, dev, G):
    B, Hkv, T, D, dtype, k_lens = 6, 1, 3, 64, torch.bfloat16, [1, 64, 65, 130, 512, 0]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev, torch.int64)
    q = queries(2261 + G, dev, B, Hkv * G, T, D, dtype)
    kc, vc = codes(2262 + G, B, Hkv, SMAX, D), codes(2263 + G, B, Hkv, SMAX, D)
    kw, vw = wide(kc, dtype, dev), wide(vc, dtype, dev)
    got = mm.block_sparse_attention_decode_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, chunk=2, return_lse=True)
    same(got, mm.block_sparse_attention_decode(q, kw, vw, layout, lens, chunk=2, return_lse=True), f"G={G} T=3")
    check_rule(f"fp8 G={G} T=3", got[0], q, kw, vw, visible([ROWS], B, Hkv, T, k_lens), G, got[1])
    assert (got[0][5] == 0).all() and (got[1][5] == -float("inf")).all()
    # (1 · v summed from +0 on the MFMA: a −0 code comes out as +0, as in the 2-byte call)
    assert_same_bits(got[0][0, :, 2], (vw[0, 0, 0] + 0.0).expand(G, D), "one visible key: its value row, widened")
    kp, vp, table = pools(kc, vc, 16, 2264 + G)
    paged = mm.block_sparse_attention_decode_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, chunk=2, return_lse=True)
    same(paged, got, f"G={G} T=3 over pages of 16 keys")


def test_6_an_item_of_a_batch_is_the_call_on_it_alone(mm, dev):
    B, Hkv, G, T, D, dtype, k_lens = 6, 1, 4, 2, 128, torch.float16, [512, 65, 300, 1, 129, 448]
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2265, dev, B, Hkv * G, T, D, dtype)
    k8, v8 = fp8(codes(2266, B, Hkv, SMAX, D), dev), fp8(codes(2267, B, Hkv, SMAX, D), dev)
    ks = torch.tensor([0.7], device=dev)
    got = mm.block_sparse_attention_decode_fp8(q, k8, v8, layout, lens, k_scale=ks, v_scale=1.3, chunk=2, return_lse=True)
    for b in range(B):
        one = mm.block_sparse_attention_decode_fp8(q[b:b + 1], k8[b:b + 1], v8[b:b + 1], layout, lens[b:b + 1], k_scale=ks, v_scale=1.3,
                                                   chunk=2, return_lse=True)
        same((got[0][b:b + 1], got[1][b:b + 1]), one, f"item {b} alone")


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------------------

def test_7_one_graph_replayed_while_the_pool_the_table_and_the_scales_change(mm, dev):
    """One capture of the paged fp8 call over pages of 16 keys.  Before every replay k_lens is advanced in place, the new
    fp8 rows are written through the uint8 view, a table slot is filled when a length opens a logical page, and k_scale and
    v_scale are CHANGED in place: the replay has the bits of the eager call on the new state."""
    B, Hkv, G, T, D, dtype, page = 2, 2, 4, 1, 64, torch.float16, 16
    W, P = SMAX // page, 12
    layout = layout_from_rows(ROWS, dev)
    q = queries(2270, dev, B, Hkv * G, T, D, dtype)
    kp, vp = (torch.full((P, Hkv, page, D), NANB, dtype=torch.uint8, device=dev) for _ in range(2))
    table = torch.full((B, W), -1, dtype=torch.int32, device=dev)
    free = [7, 2, 9, 0, 11, 4, 5, 1, 10, 3, 8, 6]
    host_lens, seed = [15, 63], 2271
    for b, n in enumerate(host_lens):
        for lp in range((n + page - 1) // page):
            table[b, lp] = free.pop(0)
        rows_k, rows_v = codes(seed + b, n, Hkv, D).to(dev), codes(seed + 10 + b, n, Hkv, D).to(dev)
        for j in range(n):
            kp[int(table[b, j // page]), :, j % page] = rows_k[j]
            vp[int(table[b, j // page]), :, j % page] = rows_v[j]
    lens = lens_tensor(host_lens, dev, torch.int64)
    ks, vs = torch.tensor([0.37, 1.9], device=dev), torch.tensor(0.8, device=dev)
    k8, v8 = kp.view(F8), vp.view(F8)
    run = lambda: mm.block_sparse_attention_decode_paged_fp8(q, k8, v8, table, layout, lens, k_scale=ks, v_scale=vs, chunk=2,  # noqa: E731
                                                             return_lse=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up on the side stream: the layout's lists are built here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a host synchronisation in here would fail the capture
        out, lse = run()
    ptrs = (kp.data_ptr(), vp.data_ptr(), table.data_ptr(), ks.data_ptr(), vs.data_ptr())
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
                kp[int(table[b, lp]), :, (n - 1) % page] = codes(seed + 100 + 10 * step + b, Hkv, D).to(dev)
                vp[int(table[b, lp]), :, (n - 1) % page] = codes(seed + 200 + 10 * step + b, Hkv, D).to(dev)
            ks.mul_(1.25 + step)
            vs.fill_(0.3 * (step + 1))
        assert lens.tolist() == host_lens and (kp.data_ptr(), vp.data_ptr(), table.data_ptr(), ks.data_ptr(), vs.data_ptr()) == ptrs
        want = run()
        flat = mm.block_sparse_attention_decode_fp8(q, gathered(kp, table).view(F8), gathered(vp, table).view(F8), layout, lens,
                                                    k_scale=ks, v_scale=vs, chunk=2, return_lse=True)
        out.fill_(NAN)
        lse.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        same((out, lse), want, f"replay {step}, k_lens {host_lens}: the eager paged fp8 call")
        same((out, lse), flat, f"replay {step}: the contiguous fp8 call on the gathered state")
        assert torch.isfinite(out.float()).all()
        assert previous is None or not torch.equal(previous, out)
        previous = out.clone()
    assert host_lens == [18, 66] and allocated == 2
    frozen = out.clone()   # the scales alone move the result
    ks.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(frozen, out)
    same((out, lse), run(), "a replay after k_scale alone changed")


# ---- 8. the C ABI --------------------------------------------------------------------------------------------------------------------------

def _fp8_entry(capi, dtype, paged_form):
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    suffix = {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]
    fn = getattr(capi, f"mi_block_attention_decode_{'paged_' if paged_form else ''}fp8_{suffix}")
    table = [vp, i64, i32, i32] if paged_form else []
    fn.argtypes = [vp, vp, i64] + 5 * [i32] + table + [i32] + [vp, i64, i64] + 2 * [vp, i64, i64, i64] + \
        [vp, i32, i32, i32, f32, vp, i32, vp, i32] + [vp, i64, i64, vp, vp, sz, vp]
    fn.restype = ctypes.c_int
    capi.mi_block_attention_decode_workspace_bytes.argtypes = 6 * [i32]
    capi.mi_block_attention_decode_workspace_bytes.restype = sz
    return fn


@pytest.mark.parametrize("dtype,D,page", [(torch.bfloat16, 96, 0), (torch.float16, 32, 0), (torch.bfloat16, 128, 16), (torch.float16, 64, 128)])
def test_8_c_abi_refusals_and_one_padded_call(mm, capi, dev, dtype, D, page):
    """MI_EINVAL / MI_ENOMEM without a launch (the outputs keep their sentinel), then one call on operands with leading
    dimensions and strides of their own — NaN around q, the NaN code around the cache (page = 0) or the pool, SENTINEL
    around out, lse and the workspace —: the bits of the call through matmuls, nothing outside touched."""
    B, Hkv, G, T, k_lens, chunk = 2, 2, 5, 2, [130, 512], 2
    items, Hq = B * Hkv, Hkv * G
    layout, lens = layout_from_rows(ROWS, dev), lens_tensor(k_lens, dev)
    q = queries(2280 + D, dev, B, Hq, T, D, dtype)
    vis = visible([ROWS], B, Hkv, T, k_lens)
    kc, vc = poisoned(codes(2281 + D, B, Hkv, SMAX, D), vis), poisoned(codes(2282 + D, B, Hkv, SMAX, D), vis)
    ks, vs = torch.tensor([0.37, 1.9], device=dev), torch.tensor([0.6], device=dev)
    if page:
        kp, vp, table = pools(kc, vc, page, 2283 + D)
        P, W, rows = kp.shape[0], SMAX // page, page
        outer = P
        want = mm.block_sparse_attention_decode_paged_fp8(q, fp8(kp, dev), fp8(vp, dev), table.to(dev), layout, lens, k_scale=ks, v_scale=vs,
                                                          chunk=chunk, return_lse=True)
        ptable = torch.full((B, W + 3), 2 ** 31 - 1, dtype=torch.int32, device=dev)
        ptable[:, :W] = table.to(dev)
    else:
        kp, vp, outer, rows = kc, vc, B, SMAX
        want = mm.block_sparse_attention_decode_fp8(q, fp8(kc, dev), fp8(vc, dev), layout, lens, k_scale=ks, v_scale=vs, chunk=chunk,
                                                    return_lse=True)
    assert torch.isfinite(want[0].float()).all()
    offsets, columns, nnz, L = mm._block_layout(layout, dev, 1, mm._csr_state(layout))["fwd"]
    fn = _fp8_entry(capi, dtype, bool(page))
    pq = padded(q.reshape(items * G, T, D), 0, NAN)
    pk, pv = (padded(x.to(dev).reshape(outer * Hkv, rows, D), i, NANB, step=16) for i, x in ((1, kp), (2, vp)))
    pout = padded(torch.full((items * G, T, D), SENTINEL, device=dev, dtype=dtype), 3, SENTINEL)
    lse_buf = torch.full((B * Hq * T + 16,), SENTINEL, device=dev)
    lse = lse_buf[8:8 + B * Hq * T]
    ws_bytes = capi.mi_block_attention_decode_workspace_bytes(items, T, G, D, SMAX, chunk)
    ws_buf = torch.full((ws_bytes + 32,), 0xAB, device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / D ** 0.5

    def call(group=G, chunk=chunk, D=D, q_ptr=pq.buf.data_ptr(), ldk=pk.ld, headK=pk.stride, ws_bytes=ws_bytes, k_count=Hkv, v_count=1,
             k_scale=ks.data_ptr(), page=page):
        tab = (ptable.data_ptr(), W + 3, P, page) if page else ()
        return fn(offsets.data_ptr(), columns.data_ptr(), nnz, L, items, Hkv, T, SMAX, *tab, D, q_ptr, pq.ld, pq.stride,
                  pk.buf.data_ptr(), ldk, headK, Hkv * pk.stride, pv.buf.data_ptr(), pv.ld, pv.stride, Hkv * pv.stride,
                  lens.data_ptr(), B, group, chunk, scale, k_scale, k_count, vs.data_ptr(), v_count, pout.buf.data_ptr(), pout.ld,
                  pout.stride, lse.data_ptr(), ws_buf.data_ptr() + 16, ws_bytes, stream)

    assert pk.ld % 16 == 0 and pk.stride % 16 == 0 and pv.stride % 16 == 0
    for kw in ({"group": 0}, {"group": 17}, {"D": 48}, {"chunk": 0}, {"q_ptr": pq.buf.data_ptr() + 2}, {"ldk": pk.ld + 8},
               {"headK": pk.stride + 8}, {"k_count": 3}, {"k_count": 0}, {"v_count": 4}, {"k_scale": ks.data_ptr() + 2}):
        assert call(**kw) == -1, kw   # MI_EINVAL
    if page:
        assert call(page=24) == -1 and call(page=8) == -1
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
