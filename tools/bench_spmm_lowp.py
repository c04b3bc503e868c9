"""bfloat16 / float16 CSR × dense against fp32 on the shapes the fp32 path is measured on.

    python tools/bench_spmm_lowp.py [--only TAG] [--log FILE]
    bash tools/kstats.sh lowp_c3 python $PWD/tools/bench_spmm_lowp.py --profile C3   (per-kernel table of C3 bf16 fwd + bwd)

Shapes: C3 and C2 (synthetic.py's pinned generator, as bench.py builds them), tools/bench_skew.py's hub-row matrix
(100 K rows of 100 entries plus rows of 10^5, 3·10^5 and 10^6 entries, K = 1 M, N = 256) and the three GNN-like shapes
of tools/bench_degree_skew.py (Pareto row lengths clipped at 8000, its generators).  Per shape, interleaved medians (ms):
the forward in fp32 as matmuls runs it (custom_mm.naive_spmm: the automatic row schedule from the second product of a
matrix on), fp32 unscheduled (naive_spmm_ex(..., -1): what MI_AUTO_SCHEDULE=0 gives), bf16 and fp16 (custom_mm.naive_spmm
on the same pattern, values and B rounded to T), and forward + backward through matmuls.naiveSpMM in each dtype.  Ratios
are to fp32 as matmuls runs it, and to fp32 unscheduled.  Algorithmic bytes of the low-precision product:
nnz·(2N+6) + 4(M+1) + 2MN.  Sampled rows (the longest included) of bf16 / fp16 are checked bit for bit against
rne_T of the fp32 product on the widened operands (naive_spmm_ex(..., 1)).
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matrix-multiplication_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import custom_mm  # noqa: E402
import matmuls  # noqa: E402
import synthetic  # noqa: E402
from bench_degree_skew import csr_from_lengths, pareto_lengths  # noqa: E402
from bench_hbm_regime import time_interleaved  # noqa: E402

dev = torch.device("cuda")
LOWP = {"bf16": torch.bfloat16, "fp16": torch.float16}


def shape_csr(name):
    """(M, K, N, rowptr, col, val) on the device."""
    if name in ("C3", "C2"):
        M, dens, N = {"C3": (1 << 20, 1e-4, 256), "C2": (1 << 16, 1e-3, 128)}[name]
        rowptr, col, val = synthetic.make_csr(M, M, dens, seed=0)
        return M, M, N, torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev)
    if name == "hub":  # tools/bench_skew.py's matrix
        M, K, N = 100_000, 1_000_000, 256
        g = torch.Generator(device=dev).manual_seed(0)
        lens = torch.full((M,), 100, dtype=torch.int64)
        lens[7], lens[5000], lens[99_999] = 1_000_000, 100_000, 300_000
        rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32).to(dev)
        nnz = int(lens.sum())
        col = torch.randint(0, K, (nnz,), device=dev, dtype=torch.int32, generator=g)
        val = torch.rand(nnz, device=dev, generator=g)
        return M, K, N, rowptr, col, val
    M, N, mean = {"arxiv": (170_000, 128, 14), "reddit": (233_000, 602, 490), "products": (2_400_000, 100, 50)}[name]
    return (M, M, N) + csr_from_lengths(pareto_lengths(M, mean, 8000, M, seed=1), M, 5)


def check_rows(rowptr, col, M, K, vals_t, B_t, C_t, n=64, seed=0):
    """Sampled rows (the longest three included) of a low-precision product vs rne_T of the fp32 product."""
    C32 = torch.empty(C_t.shape, device=dev)
    custom_mm.naive_spmm_ex(vals_t.float(), col, rowptr, col.numel(), M, K, B_t.float(), C32, 1)
    lens = (rowptr[1:] - rowptr[:-1]).long()
    rows = torch.unique(torch.cat([torch.topk(lens, 3).indices.cpu(),
                                   torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).choice(M, n, replace=False))]))
    got, want = C_t[rows.to(dev)].cpu(), C32[rows.to(dev)].cpu().to(C_t.dtype)
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    return torch.equal(gn, wn) and torch.equal(got.view(torch.int16)[~gn], want.view(torch.int16)[~wn])


def fwd_bwd(a, b, G):
    def step():
        a.grad = b.grad = None
        matmuls.naiveSpMM.apply(a, b).backward(G)
    return step


def run(name, out):
    t0 = time.time()
    M, K, N, rowptr, col, val = shape_csr(name)
    nnz = col.numel()
    g = torch.Generator(device=dev).manual_seed(7)
    B = torch.rand(K, N, device=dev, generator=g)
    ops = {"fp32": (val, B)}
    for k, dt in LOWP.items():
        ops[k] = (val.to(dt), B.to(dt))
    C = {k: torch.empty(M, N, device=dev, dtype=b.dtype) for k, (_, b) in ops.items()}
    C["fp32_unsched"] = torch.empty(M, N, device=dev)
    ent = {k: (lambda v=v, b=b, c=C[k]: custom_mm.naive_spmm(v, col, rowptr, nnz, M, K, b, c)) for k, (v, b) in ops.items()}
    ent["fp32_unsched"] = lambda: custom_mm.naive_spmm_ex(val, col, rowptr, nnz, M, K, B, C["fp32_unsched"], -1)
    t = time_interleaved(ent)
    ok = {k: check_rows(rowptr, col, M, K, ops[k][0], ops[k][1], C[k]) for k in LOWP}
    bwd = {}
    for k, (v, b) in ops.items():
        a = torch.sparse_csr_tensor(rowptr, col, v, (M, K)).requires_grad_()
        bb = b.clone().requires_grad_()
        bwd[k] = fwd_bwd(a, bb, torch.rand(M, N, device=dev, generator=g).to(b.dtype))
    tb = time_interleaved(bwd, rounds=2)
    byts = nnz * (2 * N + 6) + 4 * (M + 1) + 2 * M * N
    longest = int((rowptr[1:] - rowptr[:-1]).max())
    parts = [f"{name:9s} M={M} K={K} N={N} nnz={nnz} longest={longest}",
             f"fwd ms: fp32 {t['fp32']:.3f} fp32-unsched {t['fp32_unsched']:.3f} bf16 {t['bf16']:.3f} fp16 {t['fp16']:.3f}",
             f"bf16/fp32 {t['bf16'] / t['fp32']:.2f} (unsched {t['bf16'] / t['fp32_unsched']:.2f}) "
             f"fp16/fp32 {t['fp16'] / t['fp32']:.2f} (unsched {t['fp16'] / t['fp32_unsched']:.2f})",
             f"bf16 {byts / 1e9:.2f} GB -> {byts / t['bf16'] / 1e9:.2f} TB/s = {byts / t['bf16'] / 1e9 / 8:.2f} of 8 TB/s",
             f"fwd+bwd ms: fp32 {tb['fp32']:.2f} bf16 {tb['bf16']:.2f} fp16 {tb['fp16']:.2f} "
             f"(bf16/fp32 {tb['bf16'] / tb['fp32']:.2f}, fp16/fp32 {tb['fp16'] / tb['fp32']:.2f})",
             f"sampled rows vs rne_T(fp32): bf16 {'ok' if ok['bf16'] else 'FAIL'}, fp16 {'ok' if ok['fp16'] else 'FAIL'} "
             f"[{time.time() - t0:.0f} s]"]
    line = " | ".join(parts)
    print(line, flush=True)
    out.append(line)
    del ops, C, B, rowptr, col, val, bwd
    torch.cuda.empty_cache()
    return all(ok.values())


def profile(name, steps=3):
    """One shape in bf16, forward + backward through matmuls.naiveSpMM, `steps` times: the program tools/kstats.sh runs for
    the per-kernel tables (C3: profiles/r08_spmm_lowp_c3_kstats.log)."""
    M, K, N, rowptr, col, val = shape_csr(name)
    a = torch.sparse_csr_tensor(rowptr, col, val.to(torch.bfloat16), (M, K)).requires_grad_()
    b = torch.rand(K, N, device=dev).to(torch.bfloat16).requires_grad_()
    G = torch.rand(M, N, device=dev).to(torch.bfloat16)
    step = fwd_bwd(a, b, G)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print(f"{name} bf16 forward + backward x {steps} done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default="")
    ap.add_argument("--profile", default="", help="only run this shape's bf16 forward + backward 3 times (for kstats.sh)")
    a = ap.parse_args()
    if a.profile:
        profile(a.profile)
        return
    head = (f"# device {torch.cuda.get_device_name(0)}; interleaved medians, ms per call; low-precision algorithmic bytes "
            f"nnz·(2N+6)+4(M+1)+2MN; fp32 = naive_spmm (automatic schedule), fp32-unsched = naive_spmm_ex(-1)")
    print(head, flush=True)
    out, ok = [head], True
    for name in ("C3", "C2", "hub", "arxiv", "reddit", "products"):
        if a.only and a.only != name:
            continue
        ok = run(name, out) and ok
    if a.log:
        Path(a.log).parent.mkdir(parents=True, exist_ok=True)
        Path(a.log).write_text("\n".join(out) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
