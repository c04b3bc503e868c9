"""The block-sparse linear layer without a GPU: block_linear_takes is a rule of (dtype, block) alone, every refusal of
matmuls.block_sparse_linear is raised with its exception type before any device call, the C-ABI declares and exports the
entries and they validate their arguments before any HIP call, the split rule is a function of (kept blocks, tokens),
custom_mm refuses host tensors, and the autograd wiring of block_sparse_linear and fc_layers.blockSparseLinear is checked on
CPU tensors against torch autograd of x @ W_dense.T + bias in float64, with a float64 stand-in for the kernels
(tests/fake_custom_mm_block_linear.py)."""
import ctypes
import importlib
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "mi_spmm.h"
SUFFIXES = ("bf16", "f16")
ENTRIES = tuple(f"mi_bsr_linear_{s}" for s in SUFFIXES) + tuple(f"mi_bsr_wgrad_{s}" for s in SUFFIXES) + \
    ("mi_bsr_wgrad_split_count", "mi_bsr_wgrad_workspace_bytes")
OK, EINVAL, ERANGE, ENOMEM = 0, -1, -2, -4
FAKE = 0x1000  # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before the device


@pytest.fixture(scope="module")
def lib(built):
    import torch  # noqa: F401  (torch's HIP runtime first, as in the product)
    lib = ctypes.CDLL(str(built / "libmi_spmm.so"))
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_size_t
    for s in SUFFIXES:
        getattr(lib, f"mi_bsr_linear_{s}").argtypes = [vp, vp, vp, i64] + 4 * [i32] + [vp, i64, vp, i64, vp, vp, i64, vp]
        getattr(lib, f"mi_bsr_wgrad_{s}").argtypes = [vp, vp, vp, i64] + 3 * [i32] + [vp, i64, vp, i64, vp, i64, i32, vp, sz, vp]
    lib.mi_bsr_wgrad_split_count.argtypes = [i64, i64]
    lib.mi_bsr_wgrad_workspace_bytes.argtypes = [i64, i32]
    lib.mi_bsr_wgrad_workspace_bytes.restype = sz
    return lib


def test_header_declares_the_entries():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", text), name


def test_library_exports_the_entries(lib):
    for name in ENTRIES:
        assert hasattr(lib, name), name


LIN = dict(rowptr=FAKE, col=FAKE, ids=FAKE, nnz=4, trans_w=0, tokens=40, inner=192, outer=128, values=FAKE, nvalues=4, X=FAKE, ldx=None,
           bias=FAKE, Y=FAKE, ldy=None)
WG = dict(row=FAKE, col=FAKE, ids=FAKE, nnz=4, tokens=4096, out=128, inn=192, dY=FAKE, lddy=None, X=FAKE, ldx=None, dvalues=FAKE,
          nvalues=4, splits=1, ws=FAKE, ws_bytes=1 << 30)


def lin_call(lib, s, **kw):
    a = {**LIN, **kw}
    ldx = a["inner"] if a["ldx"] is None else a["ldx"]
    ldy = a["outer"] if a["ldy"] is None else a["ldy"]
    return getattr(lib, f"mi_bsr_linear_{s}")(a["rowptr"], a["col"], a["ids"], a["nnz"], a["trans_w"], a["tokens"], a["inner"],
                                              a["outer"], a["values"], a["nvalues"], a["X"], ldx, a["bias"], a["Y"], ldy, None)


def wg_call(lib, s, **kw):
    a = {**WG, **kw}
    lddy = a["out"] if a["lddy"] is None else a["lddy"]
    ldx = a["inn"] if a["ldx"] is None else a["ldx"]
    return getattr(lib, f"mi_bsr_wgrad_{s}")(a["row"], a["col"], a["ids"], a["nnz"], a["tokens"], a["out"], a["inn"], a["dY"], lddy,
                                             a["X"], ldx, a["dvalues"], a["nvalues"], a["splits"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("s", SUFFIXES)
def test_product_entry_validates_before_any_hip_call(lib, s):
    for kw in ({"nnz": -1}, {"nvalues": -1}, {"tokens": -1}, {"inner": -64}, {"outer": -64}):
        assert lin_call(lib, s, **kw) == EINVAL, kw
    for kw in ({"inner": 200}, {"outer": 100}, {"outer": 32}, {"ldx": 191}, {"ldy": 127}):
        assert lin_call(lib, s, **kw) == EINVAL, kw
    assert lin_call(lib, s, nnz=2 ** 31, nvalues=2 ** 31) == ERANGE
    assert lin_call(lib, s, nvalues=2 ** 31) == ERANGE
    assert lin_call(lib, s, ldx=2 ** 31) == ERANGE and lin_call(lib, s, ldy=2 ** 31) == ERANGE
    assert lin_call(lib, s, ids=None, nvalues=3) == EINVAL  # fewer blocks than entries, and no ids to say which
    for trans_w in (0, 1):
        for p in ("rowptr", "col", "values", "X", "Y"):
            assert lin_call(lib, s, trans_w=trans_w, **{p: None}) == EINVAL, p
        for p in ("X", "Y", "bias"):
            assert lin_call(lib, s, trans_w=trans_w, **{p: FAKE + 1}) == EINVAL, p  # not even 2-byte aligned
        assert lin_call(lib, s, trans_w=trans_w, values=FAKE + 8) == EINVAL  # blocks start on 16 bytes
        assert lin_call(lib, s, trans_w=trans_w, inner=0) == EINVAL  # entries, and nothing they could meet
    # an empty problem: nothing is touched, no pointer is looked at
    nulls = {p: None for p in ("rowptr", "col", "ids", "values", "X", "bias", "Y")}
    for kw in ({"tokens": 0}, {"outer": 0}):
        assert lin_call(lib, s, **kw) == OK, kw
        assert lin_call(lib, s, **kw, **nulls) == OK, kw


@pytest.mark.parametrize("s", SUFFIXES)
def test_weight_gradient_entry_validates_before_any_hip_call(lib, s):
    for kw in ({"nnz": -1}, {"nvalues": -1}, {"tokens": -1}, {"out": -64}, {"inn": -64}, {"splits": -1}):
        assert wg_call(lib, s, **kw) == EINVAL, kw
    for kw in ({"out": 100}, {"inn": 200}, {"inn": 32}, {"lddy": 127}, {"ldx": 191}, {"out": 0}, {"inn": 0}):
        assert wg_call(lib, s, **kw) == EINVAL, kw
    assert wg_call(lib, s, nnz=2 ** 31, nvalues=2 ** 31) == ERANGE
    assert wg_call(lib, s, lddy=2 ** 31) == ERANGE
    assert wg_call(lib, s, ids=None, nvalues=3) == EINVAL
    for p in ("row", "col", "dY", "X", "dvalues"):
        assert wg_call(lib, s, **{p: None}) == EINVAL, p
    for p in ("dY", "X"):
        assert wg_call(lib, s, **{p: FAKE + 1}) == EINVAL, p
    assert wg_call(lib, s, dvalues=FAKE + 8) == EINVAL
    # the ranges are whole 32-steps: 4096 = 32 · 128 takes 2, 4, …, 128 but not 3 or 256; 4000 = 32 · 125 takes 5, not 2
    for splits in (3, 256, 48):
        assert wg_call(lib, s, splits=splits) == EINVAL, splits
    assert wg_call(lib, s, tokens=4000, splits=2) == EINVAL
    # a split needs its workspace: never a silent unsplit product
    need = lib.mi_bsr_wgrad_workspace_bytes(4, 8)
    assert wg_call(lib, s, splits=8, ws=None) == EINVAL
    assert wg_call(lib, s, splits=8, ws=FAKE + 8) == EINVAL
    assert wg_call(lib, s, splits=8, ws_bytes=need - 1) == ENOMEM
    assert wg_call(lib, s, splits=0, ws_bytes=0) == ENOMEM  # the rule splits 4 blocks × 4096 tokens
    nulls = {p: None for p in ("row", "col", "ids", "dY", "X", "dvalues", "ws")}
    assert wg_call(lib, s, nnz=0, nvalues=0) == OK and wg_call(lib, s, nnz=0, nvalues=0, **nulls) == OK


def split_rule(nnz, tokens):
    """The rule of include/mi_spmm.h, restated."""
    if nnz <= 0 or tokens < 2048:
        return 1
    cap = min(1024 // nnz, tokens // 512, 32)
    s = 1
    while 2 * s <= cap:
        s *= 2
    while s > 1 and tokens % (32 * s) != 0:
        s //= 2
    return s


def test_split_rule_is_a_function_of_blocks_and_tokens(lib, built):
    import custom_mm
    for nnz in (0, 1, 2, 3, 8, 63, 64, 65, 144, 512, 1024, 2047, 2048, 2049, 10 ** 6):
        for tokens in (0, 1, 31, 2047, 2048, 2049, 2080, 4000, 4096, 6144, 8192, 10000, 16384, 16416, 65536, 2 ** 20, 2 ** 31 - 1):
            s = lib.mi_bsr_wgrad_split_count(nnz, tokens)
            assert s == split_rule(nnz, tokens) == custom_mm.bsr_wgrad_split_count(nnz, tokens), (nnz, tokens)
            assert 1 <= s <= 32 and (s == 1 or tokens % (32 * s) == 0), (nnz, tokens, s)
            if tokens < 2048:
                assert s == 1
    assert lib.mi_bsr_wgrad_split_count(8, 4096) == 8 and lib.mi_bsr_wgrad_split_count(144, 16384) == 4
    for nnz in (0, 1, 8, 144):
        for splits in (-1, 0, 1, 2, 8, 32):
            want = splits * nnz * 64 * 64 * 4 if splits > 1 else 0
            assert lib.mi_bsr_wgrad_workspace_bytes(nnz, splits) == want, (nnz, splits)


def test_custom_mm_refuses_host_tensors(built):
    import custom_mm
    offs, col = torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    for dtype in (torch.bfloat16, torch.float16):
        v, x = torch.rand(1, 64, 64).to(dtype), torch.rand(8, 64).to(dtype)
        for trans_w in (False, True):
            with pytest.raises(RuntimeError, match="device"):
                custom_mm.bsr_linear(offs, col, None, 1, v, x, None, torch.empty_like(x), trans_w)
            with pytest.raises(RuntimeError, match="device"):
                custom_mm.bsr_linear(offs, col, None, 1, v, x, x[0].clone(), torch.empty_like(x), trans_w)
        with pytest.raises(RuntimeError, match="device"):
            custom_mm.bsr_wgrad(col, col, col, 1, x, x, torch.empty_like(v))
    v, x = torch.rand(1, 64, 64).bfloat16(), torch.rand(8, 64).bfloat16()
    both = r"(?s)(?=.*\bBFloat16\b)(?=.*\bHalf\b)"  # checked before the device, so host tensors show it
    with pytest.raises(RuntimeError, match=both):
        custom_mm.bsr_linear(offs, col, None, 1, v, x.half(), None, torch.empty_like(x), False)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.bsr_linear(offs, col, None, 1, v, x, x[0].half(), torch.empty_like(x), False)
    with pytest.raises(RuntimeError, match=both):
        custom_mm.bsr_wgrad(col, col, None, 1, x, x, torch.empty_like(v).half())


@pytest.fixture()
def real(built):
    """matmuls on the real extension, imported afresh."""
    for k in ("custom_mm", "matmuls", "fc_layers"):
        sys.modules.pop(k, None)
    import matmuls
    yield matmuls
    for k in ("custom_mm", "matmuls", "fc_layers"):
        sys.modules.pop(k, None)


def test_block_linear_takes_is_a_rule_of_dtype_and_block(real):
    for block in (0, 1, 16, 32, 63, 64, 65, 128, 256, -64):
        for dt in (torch.bfloat16, torch.float16):
            assert real.block_linear_takes(dt, block) == (block == 64), (dt, block)
        for dt in (torch.float32, torch.float64, torch.int32):
            assert not real.block_linear_takes(dt, block)
    assert not real.block_linear_takes(torch.bfloat16, 64.0) and not real.block_linear_takes(torch.bfloat16, True)


def _layout(rows, cols, lead=()):
    return torch.ones(lead + (rows, cols)).to_sparse_csr()


def test_every_refusal_comes_before_the_device(real):
    f = real.block_sparse_linear
    lay = _layout(2, 3)  # out = 128, in = 192
    v = torch.rand(6, 64, 64).bfloat16()
    x = torch.rand(2, 5, 192).bfloat16()
    bias = torch.rand(128).bfloat16()
    with pytest.raises(ValueError, match="block_sparse_linear.*CSR"):
        f(x, v, lay.to_dense())
    with pytest.raises(ValueError, match="block_sparse_linear.*batched layout"):
        f(x, v, _layout(2, 3, lead=(2,)))  # a 3-d layout
    with pytest.raises(ValueError, match="block_sparse_linear: x must be a dense tensor"):
        f(lay, v, lay)
    with pytest.raises(ValueError, match=r"block_sparse_linear: x must be bfloat16 or float16, got torch.float32.*block = 64"):
        f(x.float(), v.float(), lay, bias.float())
    with pytest.raises(ValueError, match="block_sparse_linear: values must be bfloat16 or float16, got torch.float64"):
        f(x, v.double(), lay)
    with pytest.raises(RuntimeError, match=r"block_sparse_linear: x is torch.bfloat16 but values is torch.float16.*one dtype"):
        f(x, v.half(), lay)
    with pytest.raises(RuntimeError, match=r"block_sparse_linear: x is torch.bfloat16 but bias is torch.float16.*one dtype"):
        f(x, v, lay, bias.half())
    with pytest.raises(ValueError, match="block_sparse_linear: bias must be bfloat16 or float16, got torch.float32"):
        f(x, v, lay, bias.float())
    for block in (32, 128, 0, -64, 64.0, True):
        with pytest.raises(ValueError, match="block_sparse_linear: block must be 64"):
            f(x, v, lay, bias, block=block)
    with pytest.raises(ValueError, match=r"block_sparse_linear: values must be \[n, 64, 64\]"):
        f(x, torch.rand(6, 32, 32).bfloat16(), lay)
    with pytest.raises(ValueError, match="block_sparse_linear: values holds 5 blocks but the layout stores 6"):
        f(x, v[:5], lay)
    with pytest.raises(ValueError, match="block_sparse_linear: values must be contiguous"):
        f(x, v.transpose(1, 2), lay)
    for fin in (128, 100, 200, 256):  # in not the layout's, a multiple of 64 or not
        with pytest.raises(ValueError, match=rf"block_sparse_linear: x of shape .* has in = {fin} features.*multiples of block"):
            f(torch.rand(4, fin).bfloat16(), v, lay)
    for bad in (torch.rand(127).bfloat16(), torch.rand(192).bfloat16(), torch.rand(1, 128).bfloat16()):
        with pytest.raises(ValueError, match=r"block_sparse_linear: bias must be \[out\] = \[128\]"):
            f(x, v, lay, bad)
    # host tensors: the last check, and still before any device call
    for args in ((x, v, lay), (x, v, lay, bias), (x.half(), v.half(), lay, bias.half()), (x[0, 0], v, lay)):
        with pytest.raises(RuntimeError, match="block_sparse_linear.*device"):
            f(*args)


# ---- the autograd wiring on CPU tensors, float64 stand-in arithmetic -------------------------------------------------

@pytest.fixture()
def mm(oracle_mod):
    """(matmuls bound to the float64 stand-in, the stand-in, fc_layers on both)."""
    import fake_custom_mm_block_linear as fake
    names = ("custom_mm", "matmuls", "fc_layers")
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules["custom_mm"] = fake
    sys.modules.pop("matmuls", None)
    sys.modules.pop("fc_layers", None)
    matmuls = importlib.import_module("matmuls")
    fc_layers = importlib.import_module("fc_layers")
    fake.calls.clear()
    yield matmuls, fake, fc_layers
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def _random_layout(g, rows, cols, keep, index_dtype=torch.int64):
    """A CSR block layout with `keep[r]` blocks in block row r, columns in a shuffled order."""
    col = torch.cat([torch.randperm(cols, generator=g)[:k] for k in keep]).to(index_dtype)
    crow = torch.tensor([0] + list(torch.tensor(keep).cumsum(0))).to(index_dtype)
    return torch.sparse_csr_tensor(crow, col, torch.ones(col.numel()), size=(rows, cols))


def _dense_weight(values, layout):
    """W_dense [out, in] from float64 blocks in stored-entry order, differentiable in `values`."""
    rows, cols = layout.shape
    crow, col = layout.crow_indices(), layout.col_indices()
    row = torch.repeat_interleave(torch.arange(rows), crow[1:] - crow[:-1])
    blocks = values.new_zeros((rows, cols, 64, 64)).index_put((row, col.to(torch.int64)), values)
    return blocks.permute(0, 2, 1, 3).reshape(rows * 64, cols * 64)


def _close(name, got, want, dtype):
    tol = 4e-3 if dtype == torch.float16 else 3e-2  # the stand-in computes in float64 and narrows once
    assert got.dtype == dtype and got.shape == want.shape, name
    err = float((got.double() - want).abs().max()) if got.numel() else 0.0
    assert err <= tol * (float(want.abs().max() if want.numel() else 0.0) + 1.0), (name, err)


@pytest.mark.parametrize("lead,rows,cols,keep,with_bias,dtype", [
    ((40,), 2, 3, (2, 3), True, torch.float16),
    ((2, 3, 5), 3, 2, (1, 0, 2), True, torch.bfloat16),
    ((7,), 4, 4, (4, 1, 0, 2), False, torch.float16),
    ((), 2, 2, (1, 2), True, torch.bfloat16),
])
def test_block_sparse_linear_matches_dense_autograd(mm, lead, rows, cols, keep, with_bias, dtype):
    matmuls, fake, _ = mm
    g = torch.Generator().manual_seed(31)
    layout = _random_layout(g, rows, cols, keep)
    values = (torch.randn(sum(keep), 64, 64, generator=g) / 8).to(dtype).requires_grad_(True)
    x = torch.randn(lead + (cols * 64,), generator=g).to(dtype).requires_grad_(True)
    bias = torch.randn(rows * 64, generator=g).to(dtype).requires_grad_(True) if with_bias else None
    y = matmuls.block_sparse_linear(x, values, layout, bias)
    assert tuple(y.shape) == lead + (rows * 64,)
    w = torch.randn(y.shape, generator=g).to(dtype)
    y.backward(w)
    rv, rx = values.detach().double().requires_grad_(True), x.detach().double().requires_grad_(True)
    rb = bias.detach().double().requires_grad_(True) if with_bias else None
    ref = rx @ _dense_weight(rv, layout).T + (rb if with_bias else 0.0)
    grads = torch.autograd.grad(ref, (rx, rv) + ((rb,) if with_bias else ()), grad_outputs=w.double())
    _close("y", y.detach(), ref.detach(), dtype)
    _close("d x", x.grad, grads[0], dtype)
    _close("d values", values.grad, grads[1], dtype)
    if with_bias:
        _close("d bias", bias.grad, grads[2], dtype)
    names = [c[0] for c in fake.calls]
    assert names.count("bsr_linear") == 2 and names.count("bsr_wgrad") == 1 and names.count("csr_transpose") == 1
    assert names.count("column_sums") == (1 if with_bias else 0)
    lin = [c[1] for c in fake.calls if c[0] == "bsr_linear"]
    assert [(c[3], c[4]) for c in lin] == [(with_bias, False), (False, True)]  # the bias in the forward only
    tokens = 1
    for d in lead:
        tokens *= d
    assert lin[0][0] == (tokens, cols * 64) and lin[0][1] == (tokens, rows * 64)  # the leading dimensions flattened to tokens
    # a second step on the same layout tensor sorts and transposes nothing again
    y2 = matmuls.block_sparse_linear(x, values, layout, bias)
    y2.backward(w)
    assert [c[0] for c in fake.calls].count("csr_transpose") == 1
    assert torch.equal(y2.detach(), y.detach())


def test_nothing_is_computed_for_a_gradient_nobody_asked_for(mm):
    matmuls, fake, _ = mm
    g = torch.Generator().manual_seed(7)
    layout = _random_layout(g, 2, 3, (2, 1))
    mk = lambda *s: torch.randn(*s, generator=g).half()  # noqa: E731
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        x, values, bias = (t.requires_grad_(n) for t, n in zip((mk(9, 192), mk(3, 64, 64), mk(128)), need))
        fake.calls.clear()
        matmuls.block_sparse_linear(x, values, layout, bias).sum().backward()
        names = [c[0] for c in fake.calls]
        assert names.count("bsr_linear") == 1 + need[0] and names.count("bsr_wgrad") == int(need[1])
        assert names.count("column_sums") == int(need[2])
        assert [t.grad is not None for t in (x, values, bias)] == list(need)
    # without d x the transposed lists are never built
    fresh = _random_layout(g, 2, 3, (1, 1))
    values = mk(2, 64, 64).requires_grad_(True)
    fake.calls.clear()
    matmuls.block_sparse_linear(mk(4, 192), values, fresh).sum().backward()
    assert "csr_transpose" not in [c[0] for c in fake.calls]


def test_layout_record_is_shared_with_block_sparse_mm(mm, monkeypatch):
    matmuls, fake, _ = mm
    g = torch.Generator().manual_seed(11)
    layout = _random_layout(g, 2, 3, (3, 2))
    sorts = []
    plain = matmuls._sorted_lists
    monkeypatch.setattr(matmuls, "_sorted_lists", lambda *a: (sorts.append(1), plain(*a))[1])
    values = torch.randn(5, 64, 64, generator=g).half().requires_grad_(True)
    b = torch.randn(192, 8, generator=g).half().requires_grad_(True)
    matmuls.block_sparse_mm(values, layout, b).sum().backward()
    assert len(sorts) == 2  # the lists and their transpose, once
    x = torch.randn(6, 192, generator=g).half().requires_grad_(True)
    matmuls.block_sparse_linear(x, values, layout).sum().backward()
    assert len(sorts) == 2 and [c[0] for c in fake.calls].count("csr_transpose") == 1  # one sort, one transpose for both


def test_empty_cases_launch_nothing(mm):
    matmuls, fake, _ = mm
    none = torch.sparse_csr_tensor(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0), size=(3, 2))
    values = torch.zeros(0, 64, 64).half().requires_grad_(True)
    x = torch.randn(2, 5, 128).half().requires_grad_(True)
    bias = torch.randn(192).half().requires_grad_(True)
    y = matmuls.block_sparse_linear(x, values, none, bias)
    assert tuple(y.shape) == (2, 5, 192) and torch.equal(y.detach(), bias.detach().expand(2, 5, 192))  # the bias broadcast
    y.backward(torch.ones_like(y))
    assert tuple(values.grad.shape) == (0, 64, 64) and not x.grad.any() and torch.equal(bias.grad, torch.full((192,), 10.0).half())
    y = matmuls.block_sparse_linear(x, values, none)
    assert not y.any() and not torch.signbit(y).any()  # +0
    g = torch.Generator().manual_seed(3)
    layout = _random_layout(g, 3, 2, (1, 1, 2))
    v2 = torch.randn(4, 64, 64, generator=g).half().requires_grad_(True)
    e = torch.zeros(4, 0, 128).half().requires_grad_(True)  # zero tokens
    y = matmuls.block_sparse_linear(e, v2, layout, bias)
    assert tuple(y.shape) == (4, 0, 192)
    y.backward(torch.ones_like(y))
    assert tuple(v2.grad.shape) == (4, 64, 64) and not v2.grad.any() and tuple(e.grad.shape) == (4, 0, 128)
    assert not [c for c in fake.calls if c[0].startswith("bsr_")]


def test_saved_for_backward_is_the_operands_alone(mm):
    matmuls, fake, _ = mm
    g = torch.Generator().manual_seed(29)
    layout = _random_layout(g, 2, 3, (2, 1))
    values = torch.randn(3, 64, 64, generator=g).half().requires_grad_(True)
    x = torch.randn(2, 16, 192, generator=g).half().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        matmuls.block_sparse_linear(x, values, layout, torch.randn(128, generator=g).half())
    dense = [t for t in saved if t.layout == torch.strided]
    assert {t.data_ptr() for t in dense} == {values.data_ptr(), x.data_ptr()}


# ---- fc_layers.blockSparseLinear ------------------------------------------------------------------------------------------

def test_layer_state_dict_from_dense_and_contracts(mm, capsys):
    matmuls, fake, fc_layers = mm
    g = torch.Generator().manual_seed(5)
    layout = _random_layout(g, 2, 3, (2, 1))
    layer = fc_layers.blockSparseLinear(192, 128, layout).half()
    assert set(layer.state_dict()) == {"values", "bias", "crow_indices", "col_indices"}
    assert set(dict(layer.named_parameters())) == {"values", "bias"} and tuple(layer.values.shape) == (3, 64, 64)
    assert torch.equal(layer.crow_indices, layout.crow_indices()) and torch.equal(layer.col_indices, layout.col_indices())
    # a full layout starts with cublasLinear's parameters (the same seed, the same draws)
    full = fc_layers.blockSparseLinear(192, 128, _layout(2, 3))
    ref = fc_layers.cublasLinear(192, 128)
    assert torch.equal(full.dense_weight().detach(), ref.weight.detach()) and torch.equal(full.bias.detach(), ref.bias.detach())
    assert torch.equal(layer.dense_weight().detach().float()[:64, :],
                       (ref.weight.detach().half().float() * _dense_weight(torch.ones(3, 64, 64), layout))[:64, :])
    assert fc_layers.blockSparseLinear(192, 128, layout, bias=False).bias is None
    # from_dense / dense_weight round trip: what lies outside the layout is dropped
    weight, bias = torch.randn(128, 192, generator=g).half(), torch.randn(128, generator=g).half()
    made = fc_layers.blockSparseLinear.from_dense(weight, layout, bias)
    mask = _dense_weight(torch.ones(3, 64, 64), layout).half()
    assert made.values.dtype == torch.float16 and torch.equal(made.dense_weight().detach(), weight * mask)
    assert torch.equal(made.bias.detach(), bias)
    again = fc_layers.blockSparseLinear.from_dense(made.dense_weight().detach(), layout)
    assert again.bias is None and torch.equal(again.values.detach(), made.values.detach())
    # state_dict round trip into a layer built on another layout of the same size
    other = fc_layers.blockSparseLinear(192, 128, _random_layout(g, 2, 3, (1, 2))).half()
    first = other.layout()
    assert other.layout() is first  # kept while the buffers stay where they are
    other.load_state_dict(made.state_dict())
    assert torch.equal(other.col_indices, made.col_indices) and torch.equal(other.values.detach(), made.values.detach())
    rebuilt = other.layout()
    assert rebuilt is not first and torch.equal(rebuilt.col_indices(), layout.col_indices())  # rebuilt once the buffers changed
    assert other.layout() is rebuilt
    moved = other._apply(lambda t: t.clone())  # what .to(device) does to parameters and buffers
    assert moved.layout() is not rebuilt and moved.layout().col_indices().data_ptr() == moved.col_indices.data_ptr()
    # forward + backward against the dense expression
    x = torch.randn(2, 9, 192, generator=g).half().requires_grad_(True)
    y = made(x)
    y.sum().backward()
    ref_y = x.detach().double() @ made.dense_weight().detach().double().T + bias.double()
    _close("y", y.detach(), ref_y, torch.float16)
    assert made.values.grad is not None and made.bias.grad is not None and tuple(x.grad.shape) == (2, 9, 192)
    assert torch.equal(other(x.detach()), y.detach())  # the loaded layer computes the same
    # the reference's `Invalid dimensions` contract, and the dtype rule
    capsys.readouterr()
    assert made(torch.rand(4, 128).half()) == 0
    assert "Invalid dimensions" in capsys.readouterr().out
    with pytest.raises(RuntimeError, match=r"(?s)fc_layers: the input is torch.float32 but the layer's weight is torch.float16"):
        made(torch.rand(4, 192))
    with pytest.raises(ValueError, match="multiples of 64"):
        fc_layers.blockSparseLinear(100, 128, layout)
    with pytest.raises(ValueError, match="2-d CSR tensor"):
        fc_layers.blockSparseLinear(192, 128, _layout(3, 2))
