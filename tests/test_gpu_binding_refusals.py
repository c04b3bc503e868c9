"""Argument refusals of the custom_mm bindings, as a table: every entry point that takes a CSR triplet or a dense value
operand × every defect that applies to it.  Each row asserts the exception type and a message substring, and that nothing
ran: the output tensor is pre-filled with a sentinel and must still hold it.  Each entry point also runs one valid tiny
call.  Every tensor is tiny; no row reaches a kernel with bad input.

Defects: wrong index dtype, wrong value dtype, mixed value dtypes, short offsets, nnzA beyond the arrays, non-contiguous
columns, a negative size, a size beyond INT32_MAX (as an integer only, where the binding takes int64), B rows != A_cols,
the wrong C shape, a host operand."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
M, K, N, BATCH = 4, 5, 8, 2
ROWPTR = [0, 2, 3, 5, 6]
COLS = [0, 3, 1, 2, 4, 0]
NNZ = len(COLS)
BIG = 2 ** 31
# value operands: the ones value_dtype rules over (all converted for "val", one of them narrowed for "mixed")
VALUE_KEYS = ("vals", "B", "C", "dC", "G", "X", "inp", "out", "src", "A", "bias")

PATTERN = {
    "idx": "int32",
    "val": "float32",
    "mixed": r"(?s)(?=.*\bFloat\b)(?=.*\bBFloat16\b)",
    "short": r"\+ 1",
    "nnz": "exceeds",
    "noncontig": "contiguous",
    "negative": "negative size",
    "big": "dimension too large",
    "b_rows": r"B (must|\[)",
    "c_shape": r"C (must|\[)",
    "host": "device",
}


def full(*shape, dev, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=dev)


def base(dev):
    g = torch.Generator().manual_seed(0)
    i32 = dict(dtype=torch.int32, device=dev)
    off = torch.tensor(ROWPTR, **i32)
    # Aᵀ of the same pattern (rows = A's columns), and for every entry of Aᵀ its index in A
    t = torch.sparse_csr_tensor(torch.tensor(ROWPTR), torch.tensor(COLS), torch.arange(1, NNZ + 1, dtype=torch.float32),
                                (M, K)).to_dense().t().contiguous().to_sparse_csr()
    return {
        "vals": torch.rand(NNZ, generator=g).to(dev), "cols": torch.tensor(COLS, **i32), "offs": off,
        "boffs": torch.cat([off, off + NNZ]).reshape(BATCH, M + 1), "bvals": torch.rand(BATCH * NNZ, generator=g).to(dev),
        "bcols": torch.tensor(COLS * BATCH, **i32), "perm": torch.arange(NNZ, **i32), "bperm": torch.arange(BATCH * NNZ, **i32),
        "toffs": t.crow_indices().to(**i32), "tcols": t.col_indices().to(**i32), "tperm": (t.values() - 1).to(**i32),
        "nnz": NNZ, "M": M, "K": K,
        "B": torch.rand(K, N, generator=g).to(dev), "C": full(M, N, dev=dev), "bias": torch.rand(N, generator=g).to(dev),
        "A": torch.rand(M, K, generator=g).to(dev), "dC": torch.rand(M, N, generator=g).to(dev),
        "G": torch.rand(M, N, generator=g).to(dev), "inp": torch.rand(M, N, generator=g).to(dev), "out": full(M, N, dev=dev),
        "src": torch.rand(M, N, generator=g).to(dev),
    }


def batched(d, dev):
    """The batched form: two items with A's pattern, offsets [BATCH, M + 1] global over the batch."""
    g = torch.Generator().manual_seed(1)
    d.update(vals=d.pop("bvals"), cols=d.pop("bcols"), offs=d.pop("boffs"), perm=d.pop("bperm"), nnz=BATCH * NNZ,
             B=torch.rand(BATCH, K, N, generator=g).to(dev), C=full(BATCH, M, N, dev=dev),
             X=torch.rand(BATCH, M, N, generator=g).to(dev), dC=torch.rand(BATCH, M, N, generator=g).to(dev),
             out=full(BATCH * NNZ, dev=dev))
    return d


class Entry:
    """call(cmm, d) runs the entry point on the operands in d; `out` names the output that must keep the sentinel."""

    def __init__(self, name, call, defects, out=None, idx="cols", mix="B", host="B", big="K", neg="nnz", patterns=None,
                 prep=None):
        self.name, self.call, self.defects, self.out = name, call, defects, out
        self.idx, self.mix, self.host, self.big, self.neg = idx, mix, host, big, neg
        self.patterns = {**PATTERN, **(patterns or {})}
        self.prep = prep


ALL = ("idx", "val", "mixed", "short", "nnz", "noncontig", "negative", "big", "b_rows", "c_shape", "host")
NO_BIG = tuple(x for x in ALL if x != "big")


def spmm_args(d):
    return d["vals"], d["cols"], d["offs"], d["nnz"], d["M"], d["K"], d["B"]


def amax_arg(cmm, d):
    arg = torch.empty(M, N, dtype=torch.int32, device=d["C"].device)
    cmm.naive_spmm_reduce(*spmm_args(d), torch.empty(M, N, device=d["C"].device), "amax", arg)
    d["arg"] = arg
    return d


def inspected(cmm, d):
    cmm.cusparse_inspect(d["offs"], d["cols"], d["vals"], NNZ, M, N, K, "refusals")
    d.update(B=torch.rand(K * N, device=d["C"].device), C=full(M * N, dev=d["C"].device))
    return d


ENTRIES = [
    Entry("naive_spmm", lambda c, d: c.naive_spmm(*spmm_args(d), d["C"]), NO_BIG, out="C"),
    Entry("cusparse_mmul", lambda c, d: c.cusparse_mmul(*spmm_args(d), d["C"]), NO_BIG, out="C"),
    Entry("naive_spmm_ex", lambda c, d: c.naive_spmm_ex(*spmm_args(d), d["C"], -1), ALL, out="C"),
    Entry("naive_spmm_bias", lambda c, d: c.naive_spmm_bias(*spmm_args(d), d["bias"], d["C"]), ALL, out="C"),
    Entry("naive_spmm_bias_ex", lambda c, d: c.naive_spmm_bias_ex(*spmm_args(d), d["bias"], d["C"], 0), ALL, out="C"),
    Entry("naive_spmm_reduce", lambda c, d: c.naive_spmm_reduce(*spmm_args(d), d["C"], "amax"), ALL, out="C"),
    Entry("validate_csr", lambda c, d: c.validate_csr(d["vals"], d["cols"], d["offs"], d["nnz"], d["M"], d["K"]),
          ("idx", "val", "short", "nnz", "noncontig", "negative", "big", "host"), host="vals"),
    Entry("gather_perm", lambda c, d: c.gather_perm(d["vals"], d["perm"]), ("idx", "val", "noncontig", "host"), idx="perm",
          host="vals"),
    Entry("spmm_schedule", lambda c, d: c.spmm_schedule(d["offs"], d["nnz"], d["M"], N, d["cols"], d["K"]),
          ("idx", "short", "nnz", "noncontig", "negative", "big", "host"), host="offs"),
    Entry("spmm_plan", lambda c, d: c.spmm_plan(d["nnz"], d["M"], d["K"], d["B"], d["C"]),
          ("val", "mixed", "negative", "big", "host")),
    Entry("column_sums", lambda c, d: c.column_sums(d["src"]), ("val", "host"), host="src"),
    Entry("cublas_mmul_bias", lambda c, d: c.cublas_mmul_bias(d["A"], d["B"], d["bias"], d["C"], False, False),
          ("val", "mixed", "c_shape", "host"), out="C", mix="bias", host="bias", patterns={"mixed": "bias must be float32"}),
    Entry("naive_spmm_batched", lambda c, d: c.naive_spmm_batched(d["vals"], d["cols"], d["offs"], d["nnz"], BATCH, d["M"],
                                                                   d["K"], d["B"], d["C"]), ALL, out="C",
          prep=lambda c, d: batched(d, d["C"].device)),
    Entry("naive_spmm_batched_perm", lambda c, d: c.naive_spmm_batched_perm(d["vals"], d["perm"], d["cols"], d["offs"], d["nnz"],
                                                                             BATCH, d["M"], d["K"], d["B"], d["C"]), ALL, out="C",
          prep=lambda c, d: batched(d, d["C"].device)),
    Entry("naive_spmm_batched_at", lambda c, d: c.naive_spmm_batched_at(d["vals"], d["cols"], d["offs"], d["nnz"], BATCH, d["M"],
                                                                         d["K"], d["X"], d["C"]), ALL, out="C", mix="X", host="X",
          patterns={"b_rows": "X must"},
          prep=lambda c, d: dict(batched(d, d["C"].device), C=full(BATCH, K, N, dev=d["C"].device))),
    Entry("csr_transpose", lambda c, d: c.csr_transpose(d["vals"], d["cols"], d["offs"], d["nnz"], d["M"], d["K"]),
          ("idx", "val", "short", "nnz", "noncontig", "negative", "big", "host"), host="vals"),
    Entry("csr_transpose_batched", lambda c, d: c.csr_transpose_batched(d["vals"], d["cols"], d["offs"], d["nnz"], BATCH, d["M"],
                                                                         d["K"]),
          ("idx", "val", "short", "nnz", "noncontig", "negative", "big", "host"), host="vals",
          prep=lambda c, d: batched(d, d["C"].device)),
    Entry("sddmm_batched", lambda c, d: c.sddmm_batched(d["cols"], d["offs"], d["nnz"], BATCH, d["M"], d["K"], d["dC"], d["B"],
                                                         d["out"]), ALL, out="out",
          prep=lambda c, d: batched(d, d["C"].device)),
    Entry("sddmm", lambda c, d: c.sddmm(d["cols"], d["offs"], d["nnz"], d["M"], d["K"], d["dC"], d["B"]), ALL),
    Entry("naive_spmm_dense", lambda c, d: c.naive_spmm_dense(d["A"], d["B"], d["C"]),
          ("val", "mixed", "b_rows", "c_shape", "host"), out="C"),
    Entry("spmm_rows_divide", lambda c, d: c.spmm_rows_divide(d["offs"], d["M"], d["inp"], d["out"]),
          ("idx", "val", "mixed", "short", "noncontig", "negative", "big", "c_shape", "host"), out="out", idx="offs",
          mix="out", host="inp", big="M", neg="M", patterns={"c_shape": "out must"}),
    Entry("spmm_reduce_grad_val", lambda c, d: c.spmm_reduce_grad_val(d["cols"], d["offs"], d["nnz"], d["M"], d["K"], d["B"],
                                                                       d["G"], d["arg"]), ALL, mix="G",
          patterns={"c_shape": "G and arg must"}, prep=amax_arg),
    Entry("spmm_reduce_grad_b", lambda c, d: c.spmm_reduce_grad_b(d["offs"], d["cols"], d["perm"], d["vals"], d["nnz"], d["M"],
                                                                   d["K"], d["G"], d["arg"]),
          tuple(x for x in ALL if x != "b_rows"), mix="G", host="G", patterns={"c_shape": "G and arg must"},
          prep=lambda c, d: dict(amax_arg(c, d), offs=d["toffs"], cols=d["tcols"], perm=d["tperm"])),
    Entry("cusparse_inspect", lambda c, d: c.cusparse_inspect(d["offs"], d["cols"], d["vals"], d["nnz"], d["M"], N, d["K"], "bad"),
          ("idx", "val", "short", "nnz", "negative", "host"), host="vals"),
    Entry("cusparse_mmul_opt", lambda c, d: c.cusparse_mmul_opt(d["B"], d["C"], "refusals"),
          ("val", "mixed", "b_rows", "c_shape", "host"), out="C", prep=inspected),
]


def apply(defect, e, d, dev):
    """d with one defect."""
    if defect == "idx":
        d[e.idx] = d[e.idx].long()
    elif defect == "val":
        for k in VALUE_KEYS:
            if k in d:
                d[k] = d[k].double()
    elif defect == "mixed":
        d[e.mix] = d[e.mix].bfloat16()
    elif defect == "short":
        d["offs"] = d["offs"].reshape(-1)[:-1]
    elif defect == "nnz":
        d["nnz"] = d["vals"].numel() + 1
    elif defect == "noncontig":
        d[e.idx] = torch.stack([d[e.idx], d[e.idx]], -1)[..., 0]
        assert not d[e.idx].is_contiguous()
    elif defect == "negative":
        d[e.neg] = -1
    elif defect == "big":
        d[e.big] = BIG
    elif defect == "b_rows":
        k = "X" if e.name == "naive_spmm_batched_at" else "B"
        shape = list(d[k].shape)
        if e.name == "cusparse_mmul_opt":
            shape[0] += 1
        else:
            shape[-2] += 1
        d[k] = torch.rand(*shape, device=dev)
    elif defect == "c_shape":
        k = {"sddmm": "dC", "sddmm_batched": "dC", "spmm_rows_divide": "out", "spmm_reduce_grad_val": "G",
             "spmm_reduce_grad_b": "G", "cublas_mmul_bias": "C"}.get(e.name, "C")
        shape = list(d[k].shape)
        if e.name == "cusparse_mmul_opt":
            shape[0] += 1
        else:
            shape[-2] += 1
        d[k] = full(*shape, dev=dev)
    elif defect == "host":
        d[e.host] = d[e.host].cpu()
    return d


def setup(cmm, e, dev):
    d = base(dev)
    if e.prep is not None:
        d = e.prep(cmm, d)
    return d


ROWS = [(e, defect) for e in ENTRIES for defect in e.defects]


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_valid_tiny_call(cmm, dev, entry):
    d = setup(cmm, entry, dev)
    entry.call(cmm, d)
    torch.cuda.synchronize()
    if entry.out is not None and entry.name not in ("naive_spmm_dense", "naive_spmm_batched_perm", "naive_spmm_batched_at",
                                                    "sddmm_batched"):
        assert not torch.any(d[entry.out] == SENTINEL), entry.name  # it ran
    cmm.cusparse_clean()


@pytest.mark.parametrize("entry,defect", ROWS, ids=[f"{e.name}-{defect}" for e, defect in ROWS])
def test_refusal(cmm, dev, entry, defect):
    d = apply(defect, entry, setup(cmm, entry, dev), dev)
    with pytest.raises(RuntimeError, match=entry.patterns[defect]):
        entry.call(cmm, d)
    torch.cuda.synchronize()
    if entry.out is not None:
        assert torch.all(d[entry.out] == SENTINEL), (entry.name, defect)  # nothing ran
    cmm.cusparse_clean()


def test_schedule_reports_no_long_rows_below_the_split_threshold(cmm, dev):
    """A row long enough for the longest length class to reach past the long-row threshold, in a matrix whose nnz does not:
    no long-row list exists there, and the schedule says so instead of reading one back."""
    threshold = cmm.long_row_threshold()
    rows, hub = 32, 7800
    lens = [hub] + [10] * (rows - 1)
    nnz = sum(lens)
    assert nnz <= threshold
    g = torch.Generator().manual_seed(2)
    cols = torch.cat([torch.randperm(8000, generator=g)[:n].sort().values for n in lens]).int()
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lens).cumsum(0)]).int()
    sched = cmm.spmm_schedule(offs.to(dev), nnz, rows, 64)
    info = sched.info()
    longest = info["longest_at_least"]
    assert longest + longest // 8 + 1 > threshold  # (where make_schedule considers listing long rows)
    assert info["long_rows"] == 0 and info["long_rows_prepared"] is False
    vals, B = torch.rand(nnz, device=dev), torch.rand(8000, 64, device=dev)
    C0, C1 = torch.empty(rows, 64, device=dev), torch.empty(rows, 64, device=dev)
    cmm.naive_spmm_ex(vals, cols.to(dev), offs.to(dev), nnz, rows, 8000, B, C0, -1)
    cmm.naive_spmm_scheduled(sched, vals, cols.to(dev), offs.to(dev), nnz, rows, 8000, B, C1)
    assert torch.equal(C0, C1)
