#!/usr/bin/env python3
"""The block-sparse linear layer against its yardsticks, timed side by side in one run.

    python tools/bench_block_linear.py [--rounds 5] [--iters 5] [--log profiles/r16_block_linear.log]
                                       [--split-grid] [--ab-lib LABEL=PATH …]

Layers: per (tokens, in → out, bfloat16) and fraction of the 64 × 64 blocks of the weight kept at random (50 / 25 / 10 %):
forward and forward + backward (d x, d values, d bias) of fc_layers.blockSparseLinear, of cublasLinear on the densified
weight, and of the route there was before — block_sparse_mm(values, layout, x.t().contiguous()).t() plus the bias, two
transposed copies of the activations per product.
--split-grid: custom_mm.bsr_wgrad with every S ∈ {1, 2, 4, 8, 16, 32} on a grid of kept-block counts × token counts, the
count of mi_bsr_wgrad_split_count beside the best one, and the worst case of every (target, minimum range) pair of the
rule's two constants against the best S of each point.
--ab-lib LABEL=PATH (repeatable): other builds of libmi_spmm.so (a developer's edit of csrc/bsr_linear.hip, linked into a
library of its own) beside the shipped one, called through the C-ABI on the same operands, y and d x, on the layers and
on shapes either side of the token-tile threshold; the log is profiles/r16_block_linear_builds.log.
The contestants of a case are timed in interleaved rounds (one after the other inside every round, so that clock and
cache state drift over all alike); each figure is the median over the rounds of the mean of `iters` back-to-back calls
between two events, with the spread (min … max over the rounds) beside it.
"""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
PKG = REPO / "matrix-multiplication_amd"
sys.path.insert(0, str(PKG))

LAYERS = [(16384, 768, 3072), (16384, 3072, 768), (8192, 4096, 4096)]  # tokens, in, out
FRACTIONS = [0.50, 0.25, 0.10]
AB_SHAPES = [(512, 768, 3072), (1024, 768, 3072), (2048, 768, 3072), (4096, 768, 3072), (2048, 3072, 768), (4096, 3072, 768),
             (8192, 3072, 768), (256, 4096, 4096), (512, 4096, 4096), (1024, 4096, 4096), (2048, 4096, 4096)]
GRID_BLOCKS = [16, 64, 144, 288, 576, 1152]
GRID_TOKENS = [2048, 4096, 8192, 16384, 32768]
SPLITS = [1, 2, 4, 8, 16, 32]
BLOCK = 64


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def interleaved(runs, rounds, iters):
    for fn in runs.values():  # warm-up: every kernel loaded, the layout's kept lists built
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            samples[name].append(timed(fn, iters))
    return samples


def random_layout(rb, cb, keep, dev, g):
    bm = torch.zeros(rb, cb, dtype=torch.bool, device=dev)
    bm.scatter_(1, torch.rand(rb, cb, device=dev, generator=g).topk(keep, dim=-1).indices, True)
    return bm.to(torch.float32).to_sparse_csr()


def rule(nnz, tokens, target=1024, min_range=512, min_tokens=2048):
    if nnz <= 0 or tokens < min_tokens:
        return 1
    cap = min(target // nnz, tokens // min_range, 32)
    s = 1
    while 2 * s <= cap:
        s *= 2
    while s > 1 and tokens % (32 * s):
        s //= 2
    return s


def bench_layers(args, emit, dev):
    import fc_layers
    import matmuls
    for tokens, fin, fout in LAYERS:
        g = torch.Generator(device=dev).manual_seed(8)
        x = torch.randn(tokens, fin, device=dev, generator=g).bfloat16().requires_grad_(True)
        w = torch.randn(tokens, fout, device=dev, generator=g).bfloat16()
        for frac in FRACTIONS:
            rb, cb = fout // BLOCK, fin // BLOCK
            keep = max(1, round(frac * cb))
            layout = random_layout(rb, cb, keep, dev, g)
            dense = fc_layers.cublasLinear(fin, fout).to(dev).to(torch.bfloat16)
            layer = fc_layers.blockSparseLinear.from_dense(dense.weight.detach(), layout, dense.bias.detach())
            with torch.no_grad():
                dense.weight.copy_(layer.dense_weight())
            n, lay = layer.values.shape[0], layer.layout()

            def old_fn():  # the only route before: A·b on the transposed activations, then the bias
                return matmuls.block_sparse_mm(layer.values, lay, x.t().contiguous()).t() + layer.bias

            def step(fn, leaves):
                def run():
                    torch.autograd.grad(fn(), leaves, grad_outputs=w)
                return run

            sparse_leaves = (x, layer.values, layer.bias)
            runs = {"block linear fwd": lambda: layer(x), "block linear fwd+bwd": step(lambda: layer(x), sparse_leaves),
                    "dense linear fwd": lambda: dense(x), "dense linear fwd+bwd": step(lambda: dense(x), (x, dense.weight, dense.bias)),
                    "block mm on x^T fwd": old_fn, "block mm on x^T fwd+bwd": step(old_fn, sparse_leaves)}
            samples = interleaved(runs, args.rounds, args.iters)
            emit(f"\n{tokens} tokens, {fin} -> {fout}, {frac:.0%} of the blocks: {n} of {rb * cb} kept ({keep} per block row), "
                 f"weight-gradient ranges {matmuls.custom_mm.bsr_wgrad_split_count(n, tokens)}")
            med = {}
            for name, xs in samples.items():
                med[name] = statistics.median(xs)
                emit(f"  {name:26s} {med[name]:9.3f}  [{min(xs):.3f} … {max(xs):.3f}]")
            flops = 2.0 * n * BLOCK * BLOCK * tokens
            emit(f"  block linear MFMA TFLOP/s over the kept blocks: fwd {flops / med['block linear fwd'] / 1e9:.1f}, "
                 f"fwd+bwd {3 * flops / med['block linear fwd+bwd'] / 1e9:.1f}")
            emit(f"  ratio dense / block linear: fwd {med['dense linear fwd'] / med['block linear fwd']:.2f}, "
                 f"fwd+bwd {med['dense linear fwd+bwd'] / med['block linear fwd+bwd']:.2f}")
            emit(f"  ratio block mm on x^T / block linear: fwd {med['block mm on x^T fwd'] / med['block linear fwd']:.2f}, "
                 f"fwd+bwd {med['block mm on x^T fwd+bwd'] / med['block linear fwd+bwd']:.2f}")
            del runs, layer, dense
            torch.cuda.empty_cache()


def bench_split_grid(args, emit, dev):
    import custom_mm
    import matmuls
    table = {}
    emit("\nweight gradient, ms per S (median [min … max]); * = the rule's count")
    for nnz in GRID_BLOCKS:
        rb = 24 if nnz % 24 == 0 else 16
        cb = 48
        g = torch.Generator(device=dev).manual_seed(nnz)
        layout = random_layout(rb, cb, nnz // rb, dev, g)
        _, columns, ids, entry_row, n = matmuls._bsr_layout(layout, dev, matmuls._csr_state(layout))["fwd"]
        assert n == nnz
        dvalues = torch.empty(n, BLOCK, BLOCK, device=dev, dtype=torch.bfloat16)
        for tokens in GRID_TOKENS:
            x = torch.randn(tokens, cb * BLOCK, device=dev, generator=g).bfloat16()
            dy = torch.randn(tokens, rb * BLOCK, device=dev, generator=g).bfloat16()
            runs = {s: (lambda s=s: custom_mm.bsr_wgrad(entry_row, columns, ids, n, dy, x, dvalues, s))
                    for s in SPLITS if tokens % (32 * s) == 0}
            samples = interleaved(runs, args.rounds, args.iters)
            med = {s: statistics.median(xs) for s, xs in samples.items()}
            table[(nnz, tokens)] = med
            chosen, best = custom_mm.bsr_wgrad_split_count(n, tokens), min(med, key=med.get)
            cells = "  ".join(f"{'*' if s == chosen else ''}S={s}: {med[s]:.3f} [{min(samples[s]):.3f} … {max(samples[s]):.3f}]" for s in med)
            emit(f"  {nnz:5d} blocks × {tokens:6d} tokens: {cells}")
            emit(f"        best S={best}; rule S={chosen}: {med[chosen] / med[best]:.2f} × the best, {med[chosen] / med[1]:.2f} × S=1")
            del x, dy
    emit("\nthe rule's constants: worst and mean (rule / best S) over the grid, and worst (rule / S=1)")
    for target in (512, 1024, 2048, 4096, 8192):
        for min_range in (128, 256, 512, 1024):
            ratios = [(med[rule(nnz, tokens, target, min_range)] / min(med.values()), med[rule(nnz, tokens, target, min_range)] / med[1])
                      for (nnz, tokens), med in table.items()]
            emit(f"  target {target:5d}, minimum range {min_range:5d}: worst {max(r[0] for r in ratios):.2f}, "
                 f"mean {statistics.mean(r[0] for r in ratios):.3f}, worst against S=1 {max(r[1] for r in ratios):.2f}")


def bench_ab(args, emit, dev):
    import matmuls
    libs = {"shipped": ctypes.CDLL(str(PKG / "libmi_spmm.so"))}
    for spec in args.ab_lib:
        label, _, path = spec.partition("=")
        libs[label] = ctypes.CDLL(path)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    for lib in libs.values():
        lib.mi_bsr_linear_bf16.argtypes = [vp, vp, vp, i64] + 4 * [i32] + [vp, i64, vp, i64, vp, vp, i64, vp]
    emit("\nbuilds of the product kernel through the C-ABI on the same operands, ms (median [min … max]); "
         "tiles = out/64 (in/64 for d x) × ceil(tokens / 128)")
    cases = [(shape, frac) for shape in LAYERS for frac in FRACTIONS] + [(shape, 0.25) for shape in AB_SHAPES]
    for (tokens, fin, fout), frac in cases:
        g = torch.Generator(device=dev).manual_seed(9)
        x = torch.randn(tokens, fin, device=dev, generator=g).bfloat16()
        dy = torch.randn(tokens, fout, device=dev, generator=g).bfloat16()
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        rb, cb = fout // BLOCK, fin // BLOCK
        layout = random_layout(rb, cb, max(1, round(frac * cb)), dev, g)
        rec = matmuls._bsr_layout(layout, dev, matmuls._csr_state(layout))
        offsets, columns, ids, _, n = rec["fwd"]
        t_off, t_col, t_ids = matmuls._bsr_layout_transposed(rec, rb, cb)
        values = torch.randn(n, BLOCK, BLOCK, device=dev, generator=g).bfloat16()
        stream = torch.cuda.current_stream().cuda_stream

        def fwd(lib):
            st = lib.mi_bsr_linear_bf16(offsets.data_ptr(), columns.data_ptr(), ids.data_ptr(), n, 0, tokens, fin, fout,
                                        values.data_ptr(), n, x.data_ptr(), fin, None, y.data_ptr(), fout, stream)
            assert st == 0, st

        def bwd(lib):
            st = lib.mi_bsr_linear_bf16(t_off.data_ptr(), t_col.data_ptr(), t_ids.data_ptr(), n, 1, tokens, fout, fin,
                                        values.data_ptr(), n, dy.data_ptr(), fout, None, dx.data_ptr(), fin, stream)
            assert st == 0, st

        t128 = (tokens + 127) // 128
        emit(f"  {tokens} tokens, {fin} -> {fout}, {frac:.0%} kept ({n} blocks); tiles: y {rb * t128}, d x {cb * t128}")
        for what, fn in (("y", fwd), ("d x", bwd)):
            samples = interleaved({name: (lambda lib=lib: fn(lib)) for name, lib in libs.items()}, args.rounds, args.iters)
            emit("    " + f"{what:4s}" + "  ".join(f"{name}: {statistics.median(xs):.4f} [{min(xs):.4f} … {max(xs):.4f}]"
                                                   for name, xs in samples.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--split-grid", action="store_true", help="the weight gradient's split grid instead of the layers")
    ap.add_argument("--ab-lib", action="append", default=[], metavar="LABEL=PATH",
                    help="another build of libmi_spmm.so to time beside the shipped one, instead of the layers")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mode = "--split-grid" if args.split_grid else "--ab-lib" if args.ab_lib else "layers"
    lines = [f"# tools/bench_block_linear.py ({mode}) --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds "
             f"[min … max]; bfloat16, block {BLOCK}; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    if args.split_grid:
        bench_split_grid(args, emit, dev)
    elif args.ab_lib:
        bench_ab(args, emit, dev)
    else:
        bench_layers(args, emit, dev)
    default = {"layers": "r16_block_linear.log", "--split-grid": "r16_block_linear_split_grid.log", "--ab-lib": "r16_block_linear_builds.log"}
    log = Path(args.log) if args.log else REPO / "profiles" / default[mode]
    log.parent.mkdir(parents=True, exist_ok=True)
    log.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
