"""The corpus of the recorded-behaviour test of the sixteen KV-cache reading calls' Python front — a plain
module, imported by tools/record_kv_read_front.py (which writes tests/golden/kv_read_front.json) and by
tests/test_kv_read_front_host.py (which replays the corpus and compares with ==).

Two halves, all on host tensors of the smallest shapes at which the front can still go wrong:
  accepted calls, through the stand-in tests/fake_custom_mm_window.py: the binding reached and every positional argument as it
    arrives — a tensor's dtype, shape, strides and WHICH of the caller's operands it is (by data pointer), anything else by
    type name and value —, and what the call returns;
  refusals, on the real extension, whose device check refuses host tensors and names them in order: single defects that reach
    every refusal of the front, and pairs of defects across the places where the calls order their checks differently.  The
    exception's type name and its message are the record."""
import contextlib
import importlib
import sys
from collections import namedtuple

import torch

F8 = torch.float8_e4m3fn
BF16 = torch.bfloat16
B, HKV, HQ, T, D, SMAX, BLOCK, PAGE, K = 1, 1, 2, 3, 32, 128, 64, 16, 2
POOL = SMAX // PAGE  # the pages of the pool: W = 8 logical pages per item

Call = namedtuple("Call", "name decode listed paged fp8")
CALLS = [Call("block_sparse_attention_" + stem + ("_selected" if listed else "") + ("_paged" if paged else "") + ("_fp8" if fp8 else ""),
              stem == "decode", listed, paged, fp8)
         for stem in ("decode", "prefill") for listed in (False, True) for paged, fp8 in ((False, False), (True, False), (False, True),
                                                                                          (True, True))]


def kind(call):
    return ("decode" if call.decode else "prefill") + ("-lists" if call.listed else "-layout")


def modifiers(call):
    """The forms a call is accepted in: plain, and each optional piece it takes."""
    return ("plain", "tree", "window") if call.decode else ("plain", "window") if call.listed else ("plain", "split", "window")


def tiles(t):
    return -(-t // 64) + 1


def names(call):
    return ("k_pages", "v_pages") if call.paged else ("k", "v")


def expanded(shape, dtype, dim):
    """A tensor of `shape` whose dimension `dim` is one row seen again and again: a size without its memory."""
    one = list(shape)
    one[dim] = 1
    return torch.zeros(one).to(dtype).expand(shape)


def valid(call, b=B, t=T):
    """The keyword arguments of a call that every check accepts.  q is a strided view, so that a copy shows."""
    kn, vn = names(call)
    cache = F8 if call.fp8 else BF16
    q = torch.zeros(b, HQ, t, 2 * D, dtype=BF16)[..., :D] if t <= SMAX else expanded((b, HQ, t, D), BF16, 2)
    shape = (POOL, HKV, PAGE, D) if call.paged else (b, HKV, SMAX, D)
    kw = {"q": q, kn: torch.zeros(shape).to(cache), vn: torch.zeros(shape).to(cache)}
    if call.paged:
        kw["block_table"] = (torch.arange(b * POOL, dtype=torch.int32) % POOL).reshape(b, POOL)
    if call.listed:
        rows = t if call.decode else tiles(t)
        kw["block_ids"] = torch.zeros(b, HKV, rows, K, dtype=torch.int32)
        kw["block_counts"] = torch.ones(b, HKV, rows, dtype=torch.int32)
    else:
        kw["layout"] = torch.ones(SMAX // BLOCK, SMAX // BLOCK).tril().to_sparse_csr()
    kw["k_lens"] = torch.full((b,), 100, dtype=torch.int64)
    if call.fp8:
        kw.update(k_scale=0.5, v_scale=torch.ones(HKV))
    if not call.decode:
        kw["new_lens"] = torch.full((b,), 2, dtype=torch.int64)
    return kw


def with_modifier(call, kw, modifier):
    if modifier == "tree":
        kw["tree_mask"] = torch.tensor([[1, 3, 5]] * kw["q"].shape[0], dtype=torch.int64).reshape(-1, 3)
    elif modifier == "window":
        kw.update(window=5, sink=1)
    elif modifier == "split":
        kw["split"] = 1
    return kw


def accepted_cases():
    """(call, form, keyword arguments): the 44 forms with return_lse both ways, and every call on an empty batch."""
    cases = []
    for call in CALLS:
        for modifier in modifiers(call):
            for lse in (False, True):
                cases.append((call, f"{modifier}, return_lse={lse}", dict(with_modifier(call, valid(call), modifier), return_lse=lse)))
        cases.append((call, "empty batch", valid(call, b=0)))
    return cases


# ---- what a binding receives ------------------------------------------------------------------------------------------------------

def _owners(kw):
    owners = {}
    for name, t in kw.items():
        if not isinstance(t, torch.Tensor):
            continue
        if t.layout == torch.sparse_csr:
            owners[t.values().data_ptr()] = name + ".values"
            owners[t.crow_indices().data_ptr()] = name + ".crow_indices"
            owners[t.col_indices().data_ptr()] = name + ".col_indices"
        elif t.numel() > 0:
            owners[t.data_ptr()] = name
    return owners


def _describe(x, owners):
    """One line per value: a tensor's dtype, shape, strides and whose memory it is; anything else by type name and value."""
    if isinstance(x, torch.Tensor):
        whose = owners.get(x.data_ptr(), "new") if x.numel() > 0 else "new"
        return f"{x.dtype} {list(x.shape)} strides {list(x.stride())} is {whose}" + (" requires_grad" if x.requires_grad else "")
    return f"{type(x).__name__} {x!r}"


def replay_accepted(matmuls, fake, call, kw):
    """One accepted call with every block_attention_* attribute of the stand-in wrapped: the bindings reached from matmuls, in
    order, and the call's result."""
    seen, depth = [], [0]
    bindings = {n: getattr(fake, n) for n in dir(fake) if n.startswith("block_attention_") and callable(getattr(fake, n))}

    def wrap(name, fn):
        def binding(*args, **kwargs):
            if depth[0] == 0:
                seen.append((name, args, kwargs))
            depth[0] += 1
            try:
                return fn(*args, **kwargs)
            finally:
                depth[0] -= 1
        return binding

    for name, fn in bindings.items():
        setattr(fake, name, wrap(name, fn))
    try:
        result = getattr(matmuls, call.name)(**kw)
    finally:
        for name, fn in bindings.items():
            setattr(fake, name, fn)
    owners = _owners(kw)
    record = {"bindings": [[name] + [_describe(a, owners) for a in args] + [f"{k}=" + _describe(a, owners) for k, a in kwargs.items()]
                           for name, args, kwargs in seen]}
    handed = {a.data_ptr(): f"args[{i}]" for _, args, _ in seen for i, a in enumerate(args)
              if isinstance(a, torch.Tensor) and a.numel() > 0}
    parts = result if isinstance(result, tuple) else (result,)
    record["returns"] = [type(result).__name__] + [_describe(p, handed) for p in parts]
    return record


# ---- the defects ------------------------------------------------------------------------------------------------------------------

def _cache(call, kw, shape=None, dtype=None):
    """Both cache operands again, of another shape or dtype."""
    for n in names(call):
        t = kw[n]
        kw[n] = torch.zeros(shape or tuple(t.shape)).to(dtype or t.dtype)


def _set(**values):
    return lambda call, kw: kw.update(values)


def _restart(t, then=None):
    def apply(call, kw):
        kw.clear()
        kw.update(valid(call, t=t))
        if then:
            then(call, kw)
    return apply


def _mask(kw):
    return torch.ones(kw["q"].shape[0], kw["q"].shape[2], dtype=torch.int64)


def _strided_last(t):
    return torch.zeros(*t.shape[:-1], 2 * t.shape[-1]).to(t.dtype)[..., ::2]


def _padded_rows(t):
    return torch.zeros(*t.shape[:-1], t.shape[-1] + 4).to(t.dtype)[..., :t.shape[-1]]


def _unaligned(t):
    flat = torch.zeros(t.numel() + 8).to(t.dtype)
    return flat[4:4 + t.numel()].view(t.shape)


def _on(name, f):
    return lambda call, kw: kw.__setitem__(name, f(kw[name]))


def _on_cache(which, f):
    return lambda call, kw: kw.__setitem__(names(call)[which], f(kw[names(call)[which]]))


def _cache_dtype(call, kw):
    if call.fp8:
        for n in names(call):
            kw[n] = kw[n].view(torch.uint8)
    else:
        kw[names(call)[0]] = kw[names(call)[0]].float()


def _v_dtype(call, kw):
    vn = names(call)[1]
    kw[vn] = kw[vn].to(torch.float8_e5m2 if call.fp8 else torch.float16)


def _smax(smax):
    """Another Smax, as a size without its memory where it is large."""
    def apply(call, kw):
        for n in names(call):
            if call.paged:
                kw[n] = expanded((1, HKV, smax, D), kw[n].dtype, 2) if smax > SMAX else kw[n]
            else:
                kw[n] = expanded((kw["q"].shape[0], HKV, smax, D), kw[n].dtype, 2)
        if call.paged:
            kw["block_table"] = torch.zeros(kw["q"].shape[0], 1 if smax > SMAX else smax // PAGE, dtype=torch.int32)
    return apply


def _layout_beyond_int32(call, kw):
    _smax(2 ** 22)(call, kw)
    kw.update(layout=torch.ones(1, 1).to_sparse_csr(), block=2 ** 22)


def _lists(ids=None, counts=None):
    def apply(call, kw):
        b, h, r = (B, HKV, (T if call.decode else tiles(T))) if kw["q"].dim() != 4 else \
            (kw["q"].shape[0], HKV, kw["q"].shape[2] if call.decode else tiles(max(kw["q"].shape[2], 1)))
        if ids:
            kw["block_ids"] = ids(b, h, r)
        if counts:
            kw["block_counts"] = counts(b, h, r)
    return apply


def _i32(*shape, device=None):
    return torch.zeros(shape, dtype=torch.int32, device=device)


ALL = lambda c: True  # noqa: E731
DECODE = lambda c: c.decode  # noqa: E731
PREFILL = lambda c: not c.decode  # noqa: E731
LAYOUT = lambda c: not c.listed  # noqa: E731
LISTS = lambda c: c.listed  # noqa: E731
PAGED = lambda c: c.paged  # noqa: E731
FP8 = lambda c: c.fp8  # noqa: E731
SPLIT = lambda c: not c.decode and not c.listed  # noqa: E731

# name → (the calls it applies to, what it does to the keyword arguments)
DEFECTS = {
    "valid": (ALL, lambda call, kw: None),  # the device check itself: host tensors
    # _check_window
    "window=0": (ALL, _set(window=0)),
    "window=True": (ALL, _set(window=True)),
    "window=2^31": (ALL, _set(window=2 ** 31)),
    "sink=-1": (ALL, _set(window=4, sink=-1)),
    "sink=None": (ALL, _set(sink=None)),
    "sink alone": (ALL, _set(sink=1)),
    "window+tree": (DECODE, lambda call, kw: kw.update(window=4, tree_mask=_mask(kw))),
    "window+split": (SPLIT, _set(window=4, split=2)),
    # _check_tree_mask
    "tree list": (DECODE, _set(tree_mask=[1, 3, 7])),
    "tree int32": (DECODE, lambda call, kw: kw.update(tree_mask=_mask(kw).int())),
    "tree shape": (DECODE, lambda call, kw: kw.update(tree_mask=torch.ones(kw["q"].shape[0], kw["q"].shape[2] + 1, dtype=torch.int64))),
    "tree T=65": (DECODE, _restart(65, lambda call, kw: kw.update(tree_mask=_mask(kw)))),
    "tree strided": (DECODE, lambda call, kw: kw.update(tree_mask=_strided_last(_mask(kw)))),
    "tree meta": (DECODE, lambda call, kw: kw.update(tree_mask=_mask(kw).to("meta"))),
    # kinds and dtypes
    "q float32": (ALL, _on("q", lambda q: q.float())),
    "q None": (ALL, _set(q=None)),
    "cache dtype": (ALL, _cache_dtype),
    "v dtype": (ALL, _v_dtype),
    "k None": (ALL, lambda call, kw: kw.__setitem__(names(call)[0], None)),
    "layout dense": (LAYOUT, _set(layout=torch.ones(2, 2))),
    "block=96": (LAYOUT, _set(block=96)),
    "block=True": (LAYOUT, _set(block=True)),
    "chunk=0": (DECODE, _set(chunk=0)),
    "chunk=True": (DECODE, _set(chunk=True)),
    "split=0": (SPLIT, _set(split=0)),
    "split=2.0": (SPLIT, _set(split=2.0)),
    "ids int64": (LISTS, _on("block_ids", lambda t: t.long())),
    "counts None": (LISTS, _set(block_counts=None)),
    # the cache's shape
    "q 3-d": (ALL, _on("q", lambda q: q[0])),
    "D=16": (ALL, _on("q", lambda q: torch.zeros(*q.shape[:3], 16, dtype=BF16))),
    "k wide": (ALL, lambda call, kw: _cache(call, kw, tuple(kw[names(call)[0]].shape[:3]) + (2 * D,))),
    "group 17": (DECODE, _on("q", lambda q: torch.zeros(q.shape[0], 17, q.shape[2], D, dtype=BF16))),
    "Hq=0": (PREFILL, _on("q", lambda q: torch.zeros(q.shape[0], 0, q.shape[2], D, dtype=BF16))),
    "v shape": (ALL, _on_cache(1, lambda v: torch.zeros(v.shape[0] + 1, *v.shape[1:]).to(v.dtype))),
    "page 8": (PAGED, lambda call, kw: _cache(call, kw, (POOL, HKV, 8, D))),
    "table None": (PAGED, _set(block_table=None)),
    "table float": (PAGED, _on("block_table", lambda t: t.float())),
    "table 1-d": (PAGED, _on("block_table", lambda t: t[0])),
    "table strided": (PAGED, _on("block_table", _strided_last)),
    "T=0": (ALL, _on("q", lambda q: torch.zeros(q.shape[0], q.shape[1], 0, D, dtype=BF16))),
    # the layout's half
    "Smax % block": (LAYOUT, _set(block=192)),
    "layout shape": (LAYOUT, _set(layout=torch.ones(3, 3).tril().to_sparse_csr())),
    "layout lead": (LAYOUT, _set(layout=torch.ones(3, 2, 2).tril().to_sparse_csr())),
    "layout beyond int32": (LAYOUT, _layout_beyond_int32),
    # the lists' half
    "Smax % 64": (LISTS, _smax(96)),
    "ids shape": (LISTS, _lists(ids=lambda b, h, r: _i32(b, h, r + 1, K))),
    "ids 3-d": (LISTS, _lists(ids=lambda b, h, r: _i32(b, h, r))),
    "ids K=0": (LISTS, _lists(ids=lambda b, h, r: _i32(b, h, r, 0))),
    "ids strided": (LISTS, _lists(ids=lambda b, h, r: _i32(b, h, r, 2 * K)[..., ::2])),
    "counts shape": (LISTS, _lists(counts=lambda b, h, r: _i32(b, h, r + 1))),
    "counts strided": (LISTS, _lists(counts=lambda b, h, r: _i32(b, h, 2 * r)[..., ::2])),
    "ids beyond int32": (LISTS, _lists(ids=lambda b, h, r: _i32(b, h, r, 2 ** 30, device="meta"))),
    # the grid
    "T=65536": (DECODE, _restart(65536)),
    "T=2^31": (lambda c: not c.decode and not c.listed, _on("q", lambda q: expanded((q.shape[0], q.shape[1], 2 ** 31, D), BF16, 2))),
    "Smax=2^31": (lambda c: not c.decode and c.listed, _smax(2 ** 31)),
    # the lengths
    "k_lens None": (ALL, _set(k_lens=None)),
    "k_lens float": (ALL, _on("k_lens", lambda t: t.float())),
    "k_lens shape": (ALL, _on("k_lens", lambda t: torch.zeros(t.shape[0] + 1, dtype=torch.int64))),
    "new_lens list": (PREFILL, _set(new_lens=[2])),
    "new_lens float": (PREFILL, _on("new_lens", lambda t: t.float())),
    "new_lens 0-d": (PREFILL, _set(new_lens=torch.tensor(2))),
    # the strides
    "q last stride": (PREFILL, _on("q", _strided_last)),
    "q token stride": (PREFILL, _on("q", _padded_rows)),
    "q unaligned": (PREFILL, _on("q", _unaligned)),
    "k last stride": (ALL, _on_cache(0, _strided_last)),
    "v row stride": (ALL, _on_cache(1, _padded_rows)),
    "k unaligned": (ALL, _on_cache(0, _unaligned)),
    # the scales
    "k_scale str": (FP8, _set(k_scale="0.5")),
    "v_scale float64": (FP8, _set(v_scale=torch.ones(HKV, dtype=torch.float64))),
    "k_scale shape": (FP8, _set(k_scale=torch.ones(3))),
    "v_scale meta": (FP8, _set(v_scale=torch.ones(HKV, device="meta"))),
}

# pairs of defects across the places where the four bodies order their checks differently, by kind; each is applied to every
# call of the kind that both defects apply to, in the order written
PAIRS = {
    "decode-layout": [("window=0", "q float32"), ("sink alone", "layout dense"), ("chunk=0", "D=16"), ("layout dense", "block=96"),
                      ("block=96", "chunk=0"), ("cache dtype", "block=True"), ("layout shape", "k_lens float"),
                      ("T=65536", "k_lens None"), ("T=65536", "layout shape"), ("k_lens shape", "k last stride"),
                      ("tree shape", "k unaligned"), ("tree meta", "k_lens None"), ("v shape", "layout shape"),
                      ("Smax % block", "T=0"), ("k_scale str", "tree shape"), ("k_scale str", "v row stride"),
                      ("page 8", "layout shape"), ("table float", "Smax % block")],
    "decode-lists": [("window=0", "q float32"), ("chunk=0", "D=16"), ("ids int64", "ids shape"), ("ids int64", "chunk=0"),
                     ("cache dtype", "counts None"), ("Smax % 64", "ids shape"), ("ids shape", "counts shape"),
                     ("T=65536", "counts strided"), ("T=65536", "ids beyond int32"), ("T=65536", "k_lens None"),
                     ("ids beyond int32", "k_lens None"), ("k_lens float", "v row stride"), ("tree strided", "k unaligned"),
                     ("v shape", "Smax % 64"), ("group 17", "ids shape"), ("k_scale str", "tree shape"), ("page 8", "ids 3-d"),
                     ("sink alone", "ids int64")],
    "prefill-layout": [("window=0", "q float32"), ("split=0", "D=16"), ("split=0", "block=96"), ("sink alone", "split=0"),
                       ("layout dense", "cache dtype"), ("layout shape", "k_lens float"), ("k_lens None", "T=2^31"),
                       ("T=2^31", "new_lens float"), ("T=2^31", "layout shape"), ("new_lens 0-d", "q token stride"),
                       ("q last stride", "k last stride"), ("new_lens float", "k last stride"), ("Hq=0", "v shape"),
                       ("Smax % block", "T=0"), ("k_scale str", "v row stride"), ("q unaligned", "k_scale shape"),
                       ("page 8", "layout shape"), ("window+split", "block=True")],
    "prefill-lists": [("window=0", "q float32"), ("ids int64", "D=16"), ("cache dtype", "ids int64"), ("Smax % 64", "ids shape"),
                      ("ids shape", "counts shape"), ("Smax=2^31", "ids beyond int32"), ("Smax=2^31", "k_lens None"),
                      ("ids beyond int32", "k_lens None"), ("counts strided", "Smax=2^31"), ("k_lens float", "new_lens float"),
                      ("new_lens 0-d", "q token stride"), ("q unaligned", "k last stride"), ("Hq=0", "ids shape"),
                      ("counts None", "T=0"), ("k_scale str", "q last stride"), ("v_scale meta", "k unaligned"),
                      ("page 8", "ids K=0"), ("sink alone", "counts None")],
}


def refused_cases():
    """(call, case, defect names): every single defect that applies to a call, then its kind's pairs."""
    cases = []
    for call in CALLS:
        for name, (applies, _) in DEFECTS.items():
            if applies(call):
                cases.append((call, name, (name,)))
        for pair in PAIRS[kind(call)]:
            if all(DEFECTS[name][0](call) for name in pair):
                cases.append((call, " + ".join(pair), pair))
    return cases


def replay_refused(matmuls, call, defects):
    kw = valid(call)
    for name in defects:
        DEFECTS[name][1](call, kw)
    try:
        getattr(matmuls, call.name)(**kw)
    except Exception as exc:  # noqa: BLE001  (the type is the record)
        text = str(exc)
        cut = len(call.name) if text.startswith(call.name) else 0  # (in two pieces, so that the calls share the second)
        return [type(exc).__name__, text[:cut], text[cut:]]
    return ["no exception", "", ""]


def replay(call_names=None):
    """The whole corpus, or the part of the named calls, on the code at hand: ({call: {form: record}}, {call: {case: [type,
    message]}}), the message cut in two behind the call's name."""
    accepted, refused = {}, {}
    with stand_in() as (matmuls, fake):
        for call, form, kw in accepted_cases():
            if call_names is None or call.name in call_names:
                accepted.setdefault(call.name, {})[form] = replay_accepted(matmuls, fake, call, kw)
    with real_extension() as matmuls:
        for call, case, defects in refused_cases():
            if call_names is None or call.name in call_names:
                refused.setdefault(call.name, {})[case] = replay_refused(matmuls, call, defects)
    return accepted, refused


# The golden file keeps every distinct string once: a leaf of the records is its index in "strings".  Nothing is cut or rewritten.

def pack(tree, strings):
    if isinstance(tree, str):
        return strings.setdefault(tree, len(strings))
    if isinstance(tree, dict):
        return {k: pack(v, strings) for k, v in tree.items()}
    return [pack(v, strings) for v in tree]


def unpack(tree, strings):
    if isinstance(tree, int):
        return strings[tree]
    if isinstance(tree, dict):
        return {k: unpack(v, strings) for k, v in tree.items()}
    return [unpack(v, strings) for v in tree]


# ---- the two extensions, as tests/test_window_attention_host.py's `mm` and `real` fixtures load them -------------------------------

@contextlib.contextmanager
def stand_in():
    """(matmuls bound to the stand-in, the stand-in)."""
    import fake_custom_mm_window as fake
    saved = {k: sys.modules.get(k) for k in ("custom_mm", "matmuls")}
    sys.modules["custom_mm"] = fake
    sys.modules.pop("matmuls", None)
    try:
        matmuls = importlib.import_module("matmuls")
        fake.calls.clear()
        fake.spec_calls.clear()
        fake.window_calls.clear()
        yield matmuls, fake
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


@contextlib.contextmanager
def real_extension():
    """matmuls on the built extension: its device check refuses host tensors."""
    for k in ("custom_mm", "matmuls"):
        sys.modules.pop(k, None)
    try:
        import matmuls
        assert matmuls._REAL_EXTENSION, "the refusals are recorded on the built extension"
        yield matmuls
    finally:
        for k in ("custom_mm", "matmuls"):
            sys.modules.pop(k, None)
