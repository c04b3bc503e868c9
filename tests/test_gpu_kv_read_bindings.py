"""The 14 custom_mm bindings that read the KV cache — 4 decode, 2 decode over lists, 8 prefill (unsplit and split) — called
DIRECTLY, beneath matmuls' own checks: (a) one table of single malformed operands, each with the fragment
of the message the binding raises — no kernel is launched by these rows —, and (b) one valid call per binding at the
smallest shape, bit for bit (out and lse) the call through matmuls on the same operands: the argument lists as the bindings
hand them to the C entries.  The messages are those of the three *_impl functions before their shared lines were moved into
custom_mm_kv_cache.inc.

B = 2, Hkv = 1, Hq = 2, T = 1 (prefill: T = 3 with new_lens = [3, 1]), D = 32, Smax = 128, pages of 16 keys, chunk = 1 /
split = 1 (two chunks / two parts), lists of K = 2 entries, a dense causal layout."""
import pytest
import torch

from gpu_helpers import assert_same_bits

pytestmark = pytest.mark.gpu

D, SMAX, PAGE, K = 32, 128, 16, 2
W = SMAX // PAGE
NAN = float("nan")

BINDINGS = ([f"block_attention_decode{p}{f}" for p in ("", "_paged") for f in ("", "_fp8")] +
            [f"block_attention_decode_lists{p}" for p in ("", "_paged")] +
            [f"block_attention_prefill{s}{p}{f}" for s in ("", "_split") for p in ("", "_paged") for f in ("", "_fp8")])


def kind(name):
    return dict(paged="paged" in name, fp8="fp8" in name, lists="lists" in name, prefill="prefill" in name, split="split" in name)


def operands(mm, dev, name, B=2, Hkv=1, Hq=2):
    """The operands of a valid call of binding `name`, by the binding's parameter names."""
    kd = kind(name)
    T = 3 if kd["prefill"] else 1
    g = torch.Generator().manual_seed(35 + B + 7 * Hkv)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev, torch.bfloat16)  # noqa: E731
    c = dict(q=rnd(B, Hq, T, D), scale=0.25)
    shape = (B * W, Hkv, PAGE, D) if kd["paged"] else (B, Hkv, SMAX, D)
    c["k"], c["v"] = rnd(*shape), rnd(*shape)
    if kd["fp8"]:
        c["k"], c["v"] = c["k"].to(torch.float8_e4m3fn), c["v"].to(torch.float8_e4m3fn)
        c["k_scale"] = torch.linspace(0.5, 1.5, Hkv, device=dev)
        c["v_scale"] = torch.linspace(2.0, 1.0, Hkv, device=dev)
    if kd["paged"]:
        c["block_table"] = torch.arange(B * W, device=dev, dtype=torch.int32).flip(0).reshape(B, W)
    c["k_lens"] = torch.tensor(([128, 70, 33] * B)[:B], device=dev, dtype=torch.int32)
    if kd["lists"]:
        c["block_ids"] = torch.tensor([0, 1], device=dev, dtype=torch.int32).repeat(B, Hkv, T, 1)
        c["block_counts"] = torch.full((B, Hkv, T), K, device=dev, dtype=torch.int32)
    else:
        c["layout"] = torch.tril(torch.ones(SMAX // 64, SMAX // 64, device=dev)).to_sparse_csr()
        c["offsets"], c["columns"], c["nnz"], _ = mm._block_layout(c["layout"], dev, 1, mm._csr_state(c["layout"]))["fwd"]
    if kd["prefill"]:
        c["new_lens"] = torch.tensor(([3, 1, 2] * B)[:B], device=dev, dtype=torch.int32)
    if kd["split"]:
        c["split"] = 1
    if not kd["prefill"]:
        c["chunk"] = 1
    c["out"] = torch.full((B, Hq, T, D), NAN, device=dev, dtype=torch.bfloat16)
    c["lse"] = torch.full((B, Hq, T), NAN, device=dev)
    return c


def call(cmm, name, c):
    kd = kind(name)
    table = [c["block_table"]] if kd["paged"] else []
    scales = [c["k_scale"], c["v_scale"]] if kd["fp8"] else []
    if kd["lists"]:
        args = [c["block_ids"], c["block_counts"], c["q"], c["k"], c["v"], *table, c["k_lens"], c["scale"], c["chunk"], c["out"], c["lse"]]
    elif kd["prefill"]:
        args = [c["offsets"], c["columns"], c["nnz"], c["q"], c["k"], c["v"], *table, c["k_lens"], c["new_lens"], c["scale"], *scales,
                c["out"], c["lse"], *([c["split"]] if kd["split"] else [])]
    else:
        args = [c["offsets"], c["columns"], c["nnz"], c["q"], c["k"], c["v"], *table, c["k_lens"], c["scale"], *scales, c["chunk"],
                c["out"], c["lse"]]
    return getattr(cmm, name)(*args)


def through_matmuls(mm, name, c):
    kd = kind(name)
    table = [c["block_table"]] if kd["paged"] else []
    kw = dict(scale=c["scale"], return_lse=True)
    if kd["fp8"]:
        kw.update(k_scale=c["k_scale"], v_scale=c["v_scale"])
    if kd["lists"]:
        fn = mm.block_sparse_attention_decode_selected_paged if kd["paged"] else mm.block_sparse_attention_decode_selected
        return fn(c["q"], c["k"], c["v"], *table, c["block_ids"], c["block_counts"], c["k_lens"], chunk=c["chunk"], **kw)
    stem = "block_sparse_attention_prefill" if kd["prefill"] else "block_sparse_attention_decode"
    fn = getattr(mm, stem + ("_paged" if kd["paged"] else "") + ("_fp8" if kd["fp8"] else ""))
    if kd["prefill"]:
        kw.update(new_lens=c["new_lens"], split=c.get("split"))
    else:
        kw.update(chunk=c["chunk"])
    return fn(c["q"], c["k"], c["v"], *table, c["layout"], c["k_lens"], **kw)


def head_stride_4(c):
    """k over two heads that stand 4 elements apart (a view: nothing reads it)"""
    k = c["k"]
    c["k"] = torch.as_strided(k, k.shape, (k.stride(0), 4, k.stride(2), 1))


def set_(key, fn):
    def change(c):
        c[key] = fn(c[key])
    return change


ANY = lambda kd: True  # noqa: E731
# (title, the bindings it goes to, the operands' (B, Hkv, Hq), what it changes, the message's fragment or fragments by form)
MALFORMED = [
    ("cache dtype", lambda kd: not kd["fp8"], (2, 1, 2), set_("k", lambda k: k.float()), "all operands must share one dtype"),
    ("cache dtype", lambda kd: kd["fp8"], (2, 1, 2), set_("k", lambda k: k.to(torch.bfloat16)),
     "must be float8_e4m3fn (the OCP e4m3fn encoding is what is read), got BFloat16 and Float8_e4m3fn"),
    ("3-d k", lambda kd: not kd["paged"], (2, 1, 2), set_("k", lambda k: k[0]), ": q must be [B, Hq, T, D], k and v [B, Hkv, Smax, D]"),
    ("3-d k", lambda kd: kd["paged"], (2, 1, 2), set_("k", lambda k: k[0]),
     ": q must be [B, Hq, T, D], k_pages and v_pages [P, Hkv, page, D]"),
    ("k batch != B", lambda kd: not kd["paged"], (2, 1, 2), set_("k", lambda k: k[:1]),
     ": k and v must be [B, Hkv, Smax, D] = [2, Hkv, Smax, 32]"),
    ("v shape != k shape", lambda kd: not kd["paged"], (2, 1, 2), set_("v", lambda v: v[:, :, :64]),
     ": k and v must be [B, Hkv, Smax, D] = [2, Hkv, Smax, 32]"),
    ("v shape != k shape", lambda kd: kd["paged"], (2, 1, 2), set_("v", lambda v: v[:4]),
     ": k_pages and v_pages must be [P, Hkv, page, D] = [P, Hkv, page, 32]"),
    ("page 24", lambda kd: kd["paged"], (2, 1, 2),
     lambda c: c.update(k=c["k"][:, :, :1].expand(-1, -1, 24, -1), v=c["v"][:, :, :1].expand(-1, -1, 24, -1)),
     ": a page must hold a power of two >= 16 keys, got 24"),
    ("Hq % Hkv", ANY, (2, 2, 3), lambda c: None, ": 3 query heads are not a multiple of 2 k / v heads"),
    ("chunk 0", lambda kd: not kd["prefill"], (2, 1, 2), lambda c: c.update(chunk=0), ": chunk must be a positive int32, got 0"),
    ("split 0", lambda kd: kd["split"], (2, 1, 2), lambda c: c.update(split=0), ": split must be a positive int32, got 0"),
    ("table on another dtype", lambda kd: kd["paged"], (2, 1, 2), set_("block_table", lambda t: t.long()), "block_table must be int32, got Long"),
    ("non-contiguous out", lambda kd: not kd["prefill"], (2, 1, 2), set_("out", lambda o: o.repeat(1, 1, 1, 2)[..., ::2]),
     ": q and out must be contiguous [B, Hq, T, D] tensors of one shape"),
    ("non-contiguous out", lambda kd: kd["prefill"], (2, 1, 2), set_("out", lambda o: o.repeat(1, 1, 1, 2)[..., ::2]),
     ": out must be a contiguous [B, Hq, T, D] tensor of q's shape"),
    ("non-contiguous q", lambda kd: not kd["prefill"], (2, 1, 2), set_("q", lambda q: q.repeat(1, 1, 1, 2)[..., ::2]),
     ": q and out must be contiguous [B, Hq, T, D] tensors of one shape"),
    ("lse of the wrong numel", ANY, (2, 1, 2), set_("lse", lambda l: l[:1]), ": lse must be a contiguous [B, Hq, T] tensor"),
    ("k_lens of 2 entries for B = 3", ANY, (3, 1, 2), set_("k_lens", lambda l: l[:2]),
     ": k_lens must be a contiguous int32 tensor of B = 3 entries or of one, got 2"),
    ("a cache head stride of 4", lambda kd: not kd["fp8"], (2, 2, 2), head_stride_4, "'s head stride must be a multiple of 8 elements, got 4"),
    ("a cache head stride of 4", lambda kd: kd["fp8"], (2, 2, 2), head_stride_4, "'s head stride must be a multiple of 16 elements, got 4"),
    ("k_scale of 2 entries for 3 heads", lambda kd: kd["fp8"], (2, 3, 3), set_("k_scale", lambda s: s[:2]),
     ": k_scale must be None or a contiguous float32 tensor on q's device of 1 or Hkv = 3 entries"),
    ("new_lens of 2 entries for B = 3", lambda kd: kd["prefill"], (3, 1, 2), set_("new_lens", lambda l: l[:2]),
     ": new_lens must be None or a contiguous int32 tensor of B = 3 entries or of one, got 2"),
    ("block_ids of a wrong leading shape", lambda kd: kd["lists"], (2, 1, 2), set_("block_ids", lambda t: t[:1]),
     ": block_ids must be a contiguous [B, Hkv, T, K] = [2, 1, 1, K >= 1] tensor"),
    ("block_counts non-contiguous", lambda kd: kd["lists"], (2, 2, 2), set_("block_counts", lambda t: t.repeat(1, 2, 1)[:, ::2]),
     ": block_counts must be a contiguous [B, Hkv, T] = [2, 2, 1] tensor"),
]


def test_the_table_names_every_reading_binding(cmm):
    have = {n for n in dir(cmm) if n.startswith(("block_attention_decode", "block_attention_prefill"))}
    assert have == set(BINDINGS) and len(BINDINGS) == 14


@pytest.mark.parametrize("name", BINDINGS)
def test_a_malformed_operand_is_refused_with_its_message(cmm, mm, dev, name):
    kd, sent = kind(name), 0
    base = {}
    for title, where, shape, change, fragment in MALFORMED:
        if not where(kd):
            continue
        if shape not in base:
            base[shape] = operands(mm, dev, name, *shape)
        c = dict(base[shape])
        change(c)
        with pytest.raises((RuntimeError, ValueError, IndexError)) as err:
            call(cmm, name, c)
        assert (name + fragment if fragment.startswith(":") else fragment) in str(err.value), f"{name}, {title}: {err.value}"
        sent += 1
    assert sent >= 10
    torch.cuda.synchronize()
    for c in base.values():  # no kernel was launched
        assert torch.isnan(c["out"]).all() and torch.isnan(c["lse"]).all(), name


@pytest.mark.parametrize("name", BINDINGS)
def test_a_valid_call_has_the_bits_of_the_call_through_matmuls(cmm, mm, dev, name):
    c = operands(mm, dev, name)
    want_out, want_lse = through_matmuls(mm, name, c)
    assert call(cmm, name, c) is not None
    torch.cuda.synchronize()
    assert_same_bits(c["out"], want_out, f"{name}: out")
    assert_same_bits(c["lse"], want_lse, f"{name}: lse")
    assert torch.isfinite(want_lse[:, :, -1]).all() and not torch.isnan(c["out"]).any()
