"""The split key walks of matmuls.block_sparse_attention_prefill and its paged / fp8 forms without a GPU:
`split` refused with its exception type in all four calls, before the device, through the decode calls' one shared check;
split=None on the old binding with the old argument list, an int on the split binding with that int, q, the cache and the
table handed over with their own data_ptr and strides; the rule including new_lens at split ∈ {1, 3} against a dense mask,
through the float64 stand-in tests/fake_custom_mm_block_attention_prefill_split.py; the nine new entries of the C ABI —
declared, exported, mi_block_attention_prefill_split_workspace_bytes against its formula, MI_EINVAL / MI_ENOMEM / MI_OK before
any HIP call —; and block_attention_prefill_split, the suggested split of a shape."""
import ctypes
import importlib
import inspect
import re
import sys

import pytest
import torch

from test_block_attention_prefill_host import (DEFAULTS, EINVAL, FAKE, FORMS, HEADER, OK, SUFFIXES, _check, _dense_reference, _full,
                                               _poison_unseen, _random_layout, _visible)

ENOMEM, ERANGE = -4, -2
CALLS = ("block_sparse_attention_prefill", "block_sparse_attention_prefill_paged", "block_sparse_attention_prefill_fp8",
         "block_sparse_attention_prefill_paged_fp8")


# ---- the C ABI -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    for form in FORMS:
        for s in SUFFIXES:
            fn = getattr(lib, f"mi_block_attention_prefill_split_{form}{s}")
            fn.argtypes = [vp, vp, i64] + 5 * [i32] + ([vp, i64, i32, i32] if "paged" in form else []) + [i32] + \
                3 * [vp, i64, i64, i64] + [vp, i32, vp, i32, i32, f32] + ([vp, i32, vp, i32] if "fp8" in form else []) + \
                [vp, i64, i64, vp, i32, vp, ctypes.c_size_t, vp]
            fn.restype = ctypes.c_int
    lib.mi_block_attention_prefill_split_workspace_bytes.argtypes = 6 * [i32]
    lib.mi_block_attention_prefill_split_workspace_bytes.restype = i64
    lib.mi_status_string.restype = ctypes.c_char_p
    return lib


def test_header_declares_and_library_exports_the_nine_split_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = [f"mi_block_attention_prefill_split_{form}{s}" for form in FORMS for s in SUFFIXES]
    names.append("mi_block_attention_prefill_split_workspace_bytes")
    assert len(names) == 9
    for name in names:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
    assert lib.mi_status_string(ENOMEM) != lib.mi_status_string(EINVAL)


def formula(items, group, T, D, Smax, split):
    parts = -(-(Smax // 64) // split)
    return 0 if parts <= 1 else items * group * (-(-T // 64) + 1) * parts * 64 * (D + 2) * 4


def test_workspace_bytes_against_the_formula(lib):
    f = lib.mi_block_attention_prefill_split_workspace_bytes
    for items, group, T, D, Smax, split in ((8, 4, 100, 64, 512, 1), (8, 4, 100, 64, 512, 3), (1, 1, 1, 32, 128, 1), (3, 17, 64, 96, 2048, 5),
                                            (8, 4, 512, 128, 131072, 256), (65536, 8, 65, 128, 1 << 20, 7), (2, 2, 200, 128, 2048, 31)):
        assert f(items, group, T, D, Smax, split) == formula(items, group, T, D, Smax, split) > 0, (items, group, T, D, Smax, split)
    # one part: the unsplit launch, no workspace
    for Smax, split in ((512, 8), (512, 9), (512, 2 ** 31 - 1), (64, 1), (0, 1)):
        assert f(8, 4, 100, 64, Smax, split) == 0, (Smax, split)
    assert f(0, 4, 100, 64, 512, 1) == 0 and f(8, 4, 0, 64, 512, 1) == 0  # an empty call
    for bad in ((-1, 4, 100, 64, 512, 1), (8, 0, 100, 64, 512, 1), (8, 4, -1, 64, 512, 1), (8, 4, 100, 48, 512, 1), (8, 4, 100, 64, 500, 1),
                (8, 4, 100, 64, -64, 1), (8, 4, 100, 64, 512, 0), (8, 4, 100, 64, 512, -2)):
        assert f(*bad) == EINVAL, bad
    assert f(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 128, 2 ** 31 - 64, 1) == ERANGE  # beyond int64


def split_prefill(lib, form, s, split=2, workspace=FAKE, workspace_bytes=1 << 40, **kw):
    a = {**DEFAULTS, **kw}
    D, T = a["D"], a["T"]
    rows = a["page"] if "paged" in form else 512
    ldq, ldk, ldo = (D if a[n] is None else a[n] for n in ("ldq", "ldk", "ldo"))
    headQ = T * D if a["headQ"] is None else a["headQ"]
    batchQ = 8 * T * D if a["batchQ"] is None else a["batchQ"]
    headK = rows * D if a["headK"] is None else a["headK"]
    outerK = 2 * rows * D if a["outerK"] is None else a["outerK"]
    args = [FAKE, FAKE, a["nnz"], a["layouts"], a["items"], a["heads"], T, a["Smax"]]
    if "paged" in form:
        args += [a["table"], a["table_ld"], a["pages"], a["page"]]
    args += [D, a["q"], ldq, headQ, batchQ, a["k"], ldk, headK, outerK, FAKE, D, rows * D, 2 * rows * D, a["k_lens"], a["lens_count"],
             a["new_lens"], a["new_lens_count"], a["group"], 1.0]
    if "fp8" in form:
        args += [a["k_scale"], a["k_scale_count"], a["v_scale"], a["v_scale_count"]]
    args += [a["out"], ldo, T * ldo, a["lse"], split, workspace, workspace_bytes, None]
    return getattr(lib, f"mi_block_attention_prefill_split_{form}{s}")(*args)


@pytest.mark.parametrize("s", SUFFIXES)
@pytest.mark.parametrize("form", FORMS)
def test_split_entries_validate_before_any_hip_call(lib, form, s):
    """Pointers that are never dereferenced: every call here returns before the device."""
    unit = 16 if "fp8" in form else 8
    # what the prefill entries refuse
    refused = [{"group": 0}, {"D": 48}, {"Smax": 500}, {"nnz": -1}, {"layouts": 0}, {"heads": 3}, {"T": -1}, {"items": -8},
               {"lens_count": 3}, {"k_lens": None}, {"new_lens": FAKE + 2, "new_lens_count": 4}, {"new_lens": FAKE, "new_lens_count": 3},
               {"q": None}, {"q": FAKE + 8}, {"ldq": 60}, {"out": None}, {"ldo": 60}, {"lse": None}, {"lse": FAKE + 1},
               {"k": None}, {"ldk": 48}, {"headK": unit // 2}, {"outerK": unit + unit // 2}]
    if "paged" in form:
        refused += [{"page": 0}, {"page": 8}, {"page": 24}, {"pages": -1}, {"table": None}, {"table_ld": 31}]
    if "fp8" in form:
        refused += [{"k_scale_count": 3}, {"v_scale": FAKE + 2}]
    for kw in refused:
        assert split_prefill(lib, form, s, **kw) == EINVAL, kw
    # split itself, and the workspace: needed only when a full list has more than one part
    for bad in (0, -1, -2 ** 31):
        assert split_prefill(lib, form, s, split=bad) == EINVAL, bad
        assert split_prefill(lib, form, s, split=bad, items=0) == EINVAL, bad  # (a bad form is refused even for an empty call)
    need = formula(8, 4, 100, 64, 512, 2)
    assert need == lib.mi_block_attention_prefill_split_workspace_bytes(8, 4, 100, 64, 512, 2)
    assert split_prefill(lib, form, s, workspace=None) == EINVAL
    assert split_prefill(lib, form, s, workspace=FAKE + 8) == EINVAL          # misaligned
    assert split_prefill(lib, form, s, workspace_bytes=need - 1) == ENOMEM
    assert split_prefill(lib, form, s, workspace_bytes=0) == ENOMEM
    assert split_prefill(lib, form, s, workspace_bytes=need - 1, q=None) == EINVAL  # the operands come first
    # an empty call is MI_OK, with nothing looked at that it does not need
    assert split_prefill(lib, form, s, items=0, q=None, out=None, workspace=None, workspace_bytes=0) == OK
    assert split_prefill(lib, form, s, T=0, k_lens=None, lse=None, workspace=None, workspace_bytes=0) == OK


# ---- matmuls on the real extension: refusals before the device ---------------------------------------------------

@pytest.fixture()
def real(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)


def _cpu_operands():
    q = torch.rand(2, 4, 70, 64).bfloat16()
    k = torch.rand(2, 2, 256, 64).bfloat16()
    pool = torch.rand(9, 2, 32, 64).bfloat16()
    table = torch.arange(16).reshape(2, 8) % 9
    k8, pool8 = k.to(torch.float8_e4m3fn), pool.to(torch.float8_e4m3fn)
    lay, lens = _full(4), torch.tensor([100, 256])
    return {"block_sparse_attention_prefill": (q, k, k, lay, lens), "block_sparse_attention_prefill_paged": (q, pool, pool, table, lay, lens),
            "block_sparse_attention_prefill_fp8": (q, k8, k8, lay, lens),
            "block_sparse_attention_prefill_paged_fp8": (q, pool8, pool8, table, lay, lens)}


@pytest.mark.parametrize("name", CALLS)
def test_split_is_refused_before_the_device_with_its_type(real, name):
    f, args = getattr(real, name), _cpu_operands()[name]
    assert inspect.signature(f).parameters["split"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(f).parameters["split"].default is None
    for bad in (True, False, 2.0, 0, -3, 2 ** 31, "4", (2,)):
        with pytest.raises(ValueError, match=name + ": split must be None or a positive int, got " + re.escape(repr(bad))):
            f(*args, split=bad)
    # a good split (and None) passes every ValueError and reaches the last check: the operands are host tensors
    for good in (None, 1, 3, 2 ** 31 - 1):
        with pytest.raises(RuntimeError, match=name + r": layout, q, .* must be device \(HIP\) tensors"):
            f(*args, split=good)
    # the one shared check: the refusal comes with the decode calls' refusals, before a shape is looked at
    with pytest.raises(ValueError, match=name + ": split must be None or a positive int"):
        f(args[0][0], *args[1:], split=0)  # (q 3-d is refused later)
    with pytest.raises(TypeError):  # there is still no chunk
        f(*args, chunk=2)


def test_the_split_bindings_exist_and_refuse_host_tensors(built):
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    import custom_mm
    offs, col = torch.tensor([[0, 1]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    q, kv = torch.rand(1, 2, 3, 32).bfloat16(), torch.rand(1, 1, 64, 32).bfloat16()
    lens, lse = torch.tensor([5], dtype=torch.int32), torch.empty(1, 2, 3)
    with pytest.raises(RuntimeError, match="device"):
        custom_mm.block_attention_prefill_split(offs, col, 1, q, kv, kv, lens, None, 1.0, torch.empty_like(q), lse, 2)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(RuntimeError, match="block_attention_prefill_split: split must be a positive int32"):
            custom_mm.block_attention_prefill_split(offs, col, 1, q, kv, kv, lens, None, 1.0, torch.empty_like(q), lse, bad)
    with pytest.raises(TypeError):  # split is required
        custom_mm.block_attention_prefill_split(offs, col, 1, q, kv, kv, lens, None, 1.0, torch.empty_like(q), lse)
    for name in ("block_attention_prefill_split_paged", "block_attention_prefill_split_fp8", "block_attention_prefill_split_paged_fp8"):
        assert callable(getattr(custom_mm, name))


def test_the_suggested_split_is_none_or_a_positive_int_of_its_five_arguments(real):
    f = real.block_attention_prefill_split
    assert list(inspect.signature(f).parameters) == ["B", "Hq", "T", "Smax", "D"]
    shapes = [(B, 32, T, S, D) for B in (1, 4) for T in (1, 64, 512, 2048, 131072) for S in (64, 8192, 32768, 131072) for D in (32, 128)]
    first = [f(*s) for s in shapes]
    for s, got in zip(shapes, first):
        assert got is None or (isinstance(got, int) and not isinstance(got, bool) and 1 <= got < 2 ** 31), (s, got)
    torch.manual_seed(5)  # nothing else moves it: not the generator, not an earlier call, not the order
    assert [f(*s) for s in reversed(shapes)] == first[::-1]
    assert f(B=1, Hq=32, T=512, Smax=131072, D=128) == f(1, 32, 512, 131072, 128)
    assert "profiles/r30_block_attention_prefill_split.log" in f.__doc__


def test_the_suggested_split_against_the_rows_it_was_fitted_on(real):
    """Every row of profiles/r30_block_attention_prefill_split.log: where the helper names a split, that split was measured on
    the row and its median is no slower than the unsplit call by more than the unsplit call's own [min … max] of that row;
    where every block is kept it wins outright; where it names none, no measured split beat the unsplit minimum by 10 %."""
    log = (HEADER.parent.parent / "profiles" / "r30_block_attention_prefill_split.log").read_text()
    rows, cur = [], None
    for line in log.splitlines():
        m = re.match(r"chunk:(\d+):(\d+):(\d+), .*k_len = \d+, ([^:]+):", line)
        if m:
            cur = {"shape": (int(m[1]), 32, int(m[2]), int(m[3]), 128), "layout": m[4], "ms": {}}
            rows.append(cur)
        m = re.match(r"\s+(unsplit|split \d+)\s+([\d.]+)\s+\[([\d.]+) … ([\d.]+)\]", line)
        if m and cur is not None:
            cur["ms"][m[1]] = tuple(float(x) for x in m.groups()[1:])
    assert len(rows) == 2 * 3 * 3 * 3
    named = 0
    for row in rows:
        s = real.block_attention_prefill_split(*row["shape"])
        unsplit = row["ms"]["unsplit"]
        if s is None:
            assert all(v[0] > 0.9 * unsplit[1] for n, v in row["ms"].items() if n != "unsplit"), row
            continue
        named += 1
        assert f"split {s}" in row["ms"], (row["shape"], s)
        assert row["ms"][f"split {s}"][0] <= unsplit[2], row
        if row["layout"] == "fully kept":
            assert row["ms"][f"split {s}"][0] < 0.75 * unsplit[1], row
    assert named == 3 * 3 * 3


# ---- wiring on CPU tensors, float64 stand-in arithmetic on float16 storage -----------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in)."""
    import fake_custom_mm_block_attention_prefill_split as fake
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


def _spy(monkeypatch, fake, name):
    """The positional arguments `name` of the stand-in receives, call by call."""
    seen, inner = [], getattr(fake, name)

    def binding(*args, **kw):
        assert not kw
        seen.append(args)
        return inner(*args)

    monkeypatch.setattr(fake, name, binding)
    return seen


def test_none_reaches_the_old_binding_and_an_int_the_split_binding(mm, monkeypatch):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(131)
    B, Hkv, G, T, Smax, D, page = 2, 2, 2, 10, 128, 32, 16
    Hq = Hkv * G
    layout, lens, news = _random_layout(g, (), 2, keep=2), torch.tensor([100, 128]), torch.tensor([10, 4])
    fused = torch.randn(B, T, Hq + 2 * Hkv, D, generator=g).half()
    q = fused[:, :, :Hq].transpose(1, 2)  # strided: handed over as it is
    k, v = (torch.randn(B, Smax, Hkv, D, generator=g).half().transpose(1, 2) for _ in range(2))
    W = Smax // page
    table = torch.zeros(B, W + 3, dtype=torch.int32)
    table[:, :W] = torch.randperm(B * W, generator=g).reshape(B, W).to(torch.int32)
    pool_k, pool_v = (torch.randn(B * W, Hkv, page, D, generator=g).half() for _ in range(2))
    k8, v8 = (torch.randn(B, Hkv, Smax, D, generator=g).to(torch.float8_e4m3fn) for _ in range(2))
    p8k, p8v = (x.to(torch.float8_e4m3fn) for x in (pool_k, pool_v))
    ks = torch.tensor([0.5, 2.0])
    forms = {"": (matmuls.block_sparse_attention_prefill, (q, k, v), {}, 11),
             "_paged": (matmuls.block_sparse_attention_prefill_paged, (q, pool_k, pool_v, table[:, :W]), {}, 12),
             "_fp8": (matmuls.block_sparse_attention_prefill_fp8, (q, k8, v8), {"k_scale": ks}, 13),
             "_paged_fp8": (matmuls.block_sparse_attention_prefill_paged_fp8, (q, p8k, p8v, table[:, :W]), {"k_scale": ks}, 14)}
    for suffix, (call, operands, kw, old_count) in forms.items():
        old = _spy(monkeypatch, fake, "block_attention_prefill" + suffix)
        new = _spy(monkeypatch, fake, "block_attention_prefill_split" + suffix)
        fake.calls.clear()
        want = call(*operands, layout, lens, new_lens=news, **kw)
        same = call(*operands, layout, lens, new_lens=news, split=None, **kw)
        assert len(old) == 2 and not new and all(len(a) == old_count for a in old)  # the old binding, its own argument list
        assert [c[0] for c in fake.calls] == 2 * ["block_attention_prefill" + suffix] and "split" not in fake.calls[0][1]
        assert torch.equal(want, same)
        for split in (1, 7, 2 ** 31 - 1):
            fake.calls.clear()
            got = call(*operands, layout, lens, new_lens=news, split=split, **kw)
            assert len(old) == 2 and len(new[-1]) == old_count + 1 and new[-1][-1] == split and type(new[-1][-1]) is int
            for x, y in zip(new[-1][:old_count - 2], old[-1][:old_count - 2]):  # the old argument list in front of split
                assert (x.data_ptr() == y.data_ptr() or torch.equal(x, y)) if isinstance(x, torch.Tensor) else x == y
            (name, rec), = fake.calls
            assert name == "block_attention_prefill_split" + suffix and rec["split"] == split
            kk, vv = operands[1], operands[2]
            assert rec["q_ptr"] == q.data_ptr() and rec["q_stride"] == tuple(q.stride())  # no .contiguous() on q
            assert rec["k_ptr"] == kk.data_ptr() and rec["k_stride"] == tuple(kk.stride())
            assert rec["v_ptr"] == vv.data_ptr() and rec["v_stride"] == tuple(vv.stride())
            if "paged" in suffix:
                assert rec["table_ptr"] == table.data_ptr() and rec["table_stride"] == (W + 3, 1)
            assert rec["new_lens"].tolist() == [10, 4] and torch.equal(got, want)
            out, lse = call(*operands, layout, lens, new_lens=news, split=split, return_lse=True, **kw)
            assert torch.equal(out, want) and lse.shape == (B, Hq, T) and lse.dtype == torch.float32


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("G,T,block,l_lead,k_lens,new_lens", [
    (4, 70, 64, (), [130, 256], [70, 33]),
    (2, 5, 128, (), [130, 257], [0, 5]),
    (3, 9, 64, (2, 2), [200, 64], [4, 9]),
    (2, 40, 64, (2,), [0, 12], [40, -3]),
])
def test_the_rule_with_new_lens_through_the_split_binding(mm, split, G, T, block, l_lead, k_lens, new_lens):
    matmuls, fake = mm
    g = torch.Generator().manual_seed(137 + G + T)
    B, Hkv, Smax, D = 2, 2, 256, 32
    layout = _random_layout(g, l_lead, Smax // block, keep=max(1, Smax // block - 1))
    lens, news = torch.tensor(k_lens, dtype=torch.int64), torch.tensor(new_lens, dtype=torch.int64)
    vis = _visible(layout, B, Hkv, T, Smax, block, k_lens, new_lens)
    q = torch.randn(B, Hkv * G, T, D, generator=g).half()
    k, v = (torch.randn(B, Hkv, Smax, D, generator=g).half() for _ in range(2))
    want, want_lse = _dense_reference(q, k.double(), v.double(), vis, 1.0 / D ** 0.5, G)
    out, lse = matmuls.block_sparse_attention_prefill(q, _poison_unseen(k, vis), _poison_unseen(v, vis), layout, lens, block=block,
                                                      new_lens=news, return_lse=True, split=split)
    _check(out, lse, q, want, want_lse, vis, G)
    (name, rec), = fake.calls
    assert name == "block_attention_prefill_split" and rec["split"] == split
    assert rec["new_lens"].dtype == torch.int32 and rec["new_lens"].tolist() == new_lens  # as given: the kernel clamps
