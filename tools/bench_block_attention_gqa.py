#!/usr/bin/env python3
"""Grouped-query heads and per-item lengths of block-sparse attention, measured.

    python tools/bench_block_attention_gqa.py [--rounds 7] [--iters 10] [--parent-lib PATH]
                                              [--log profiles/r18_block_attention_gqa.log]

Everything bfloat16, D = 64, block 64; contestants of a case are timed in interleaved rounds, each figure the median over
the rounds of the mean of `iters` back-to-back calls between two events, with the spread (min … max) beside it.
 1. Grouped against the only route without it: 8 × 32 query heads over 8 and over 1 k / v heads, 2048², a window of 3
    blocks and the window plus a global column; forward and forward + backward of block_sparse_attention on grouped k, v
    against the same call on k.repeat_interleave(G, -3), the repeat and autograd's sum over the group inside the timed
    region.
 2. The existing path: the rows of profiles/r14_block_attention.log through the plain C entries (forward, backward) of
    this build and — with --parent-lib, a libmi_spmm.so built from the parent commit — of the parent's, in the same rounds.
 3. Lengths: the 48 × 2048² window batch with lengths uniform in [S/4, S] beside the full-length call.
"""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tests"))

from bench_block_attention import SHAPES, block_masks, timed  # noqa: E402

D, BLOCK = 64, 64


def measure(runs, rounds, iters):
    for fn in runs.values():  # warm-up: every kernel loaded, the layouts' kept forms built
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in runs}
    for _ in range(rounds):
        for n, fn in runs.items():
            samples[n].append(timed(fn, iters))
    return {n: (statistics.median(xs), min(xs), max(xs)) for n, xs in samples.items()}


def c_entries(path):
    """(fwd, bwd) plain bfloat16 entries of a libmi_spmm.so with their argument types."""
    lib = ctypes.CDLL(str(path))
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t
    dense = [vp, i64, i64]
    lib.mi_block_attention_fwd_bf16.argtypes = [vp, vp, i64] + 6 * [i32] + 3 * dense + [f32] + dense + [vp, vp]
    lib.mi_block_attention_bwd_bf16.argtypes = [vp, vp, vp, vp, i64] + 6 * [i32] + 5 * dense + [vp, f32] + 3 * dense + [vp, sz, vp]
    return lib.mi_block_attention_fwd_bf16, lib.mi_block_attention_bwd_bf16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r18_block_attention_gqa.log"))
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_block_attention_gqa.py --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds "
             f"[min … max]; bfloat16, D = {D}, block {BLOCK}; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    def show(res):
        for n, (med, lo, hi) in res.items():
            emit(f"  {n:34s} {med:8.3f}  [{lo:.3f} … {hi:.3f}]")

    # ---- 1. grouped against repeat_interleave -----------------------------------------------------------------------
    B, Hq, S = 8, 32, 2048
    nb = S // BLOCK
    g = torch.Generator(device=dev).manual_seed(8)
    q = torch.randn(B, Hq, S, D, device=dev, generator=g).bfloat16().requires_grad_(True)
    w = torch.randn(B, Hq, S, D, device=dev, generator=g).bfloat16()
    masks = block_masks(nb, dev, 9)
    for Hkv in (8, 1):
        G = Hq // Hkv
        k, v = (torch.randn(B, Hkv, S, D, device=dev, generator=g).bfloat16().requires_grad_(True) for _ in range(2))
        for name in ("window 3", "window 3 + global column"):
            layout = masks[name][0].float().to_sparse_csr()

            def grouped():
                return matmuls.block_sparse_attention(q, k, v, layout)

            def repeated():
                return matmuls.block_sparse_attention(q, k.repeat_interleave(G, -3), v.repeat_interleave(G, -3), layout)

            def step(fn):
                return lambda: torch.autograd.grad(fn(), (q, k, v), grad_outputs=w)

            res = measure({"grouped fwd": grouped, "repeat_interleave fwd": repeated, "grouped fwd+bwd": step(grouped),
                           "repeat_interleave fwd+bwd": step(repeated)}, args.rounds, args.iters)
            emit(f"\n{B} x {Hq} query heads over {Hkv} k/v heads (G = {G}), {S}^2, {name}")
            show(res)
            emit(f"  ratio grouped / repeat_interleave: fwd {res['grouped fwd'][0] / res['repeat_interleave fwd'][0]:.3f}, "
                 f"fwd+bwd {res['grouped fwd+bwd'][0] / res['repeat_interleave fwd+bwd'][0]:.3f}")
        del k, v
    del q, w

    # ---- 2. the existing path, this build beside the parent's ----------------------------------------------------------
    libs = {"this build": c_entries(REPO / "matrix-multiplication_amd" / "libmi_spmm.so")}
    if args.parent_lib:
        libs["parent"] = c_entries(args.parent_lib)
    stream = torch.cuda.current_stream().cuda_stream
    for items, S in SHAPES:
        nb = S // BLOCK
        g = torch.Generator(device=dev).manual_seed(8)
        q, k, v, w = (torch.randn(items, S, D, device=dev, generator=g).bfloat16() for _ in range(4))
        out, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
        lse, ws = torch.empty(items, S, device=dev), torch.empty(items * S * 4, dtype=torch.uint8, device=dev)
        for name, (bm, causal) in block_masks(nb, dev, 9).items():
            layout = bm.float().to_sparse_csr()
            rec = matmuls._block_layout(layout, dev, 1, matmuls._csr_state(layout))
            off, col, nnz, L = rec["fwd"]
            t_off, t_col = matmuls._block_layout_transposed(rec, nb, nb)
            dense = lambda t: (t.data_ptr(), D, S * D)  # noqa: E731
            runs = {}
            for which, (fwd, bwd) in libs.items():
                runs[f"{which}: fwd"] = lambda fwd=fwd: fwd(off.data_ptr(), col.data_ptr(), nnz, L, items, S, S, D, int(causal), *dense(q),
                                                           *dense(k), *dense(v), 0.125, *dense(out), lse.data_ptr(), stream)
                runs[f"{which}: bwd"] = lambda bwd=bwd: bwd(off.data_ptr(), col.data_ptr(), t_off.data_ptr(), t_col.data_ptr(), nnz, L,
                                                           items, S, S, D, int(causal), *dense(q), *dense(k), *dense(v), *dense(out),
                                                           *dense(w), lse.data_ptr(), 0.125, *dense(dq), *dense(dk), *dense(dv),
                                                           ws.data_ptr(), ws.numel(), stream)
            res = measure(runs, args.rounds, args.iters)
            emit(f"\n{items} x {S}^2, {name}: the plain C entries")
            show(res)
            if args.parent_lib:
                for leg in ("fwd", "bwd"):
                    a, b = res[f"this build: {leg}"], res[f"parent: {leg}"]
                    spread = max(a[2] - a[1], b[2] - b[1])
                    emit(f"  {leg}: this build − parent {a[0] - b[0]:+.4f} ms (ratio {a[0] / b[0]:.3f}); spread of a build's own "
                         f"rounds {spread:.4f} ms: {'within' if abs(a[0] - b[0]) <= spread else 'OUTSIDE'}")

    # ---- 3. lengths ---------------------------------------------------------------------------------------------------
    items, S = 48, 2048
    nb = S // BLOCK
    g = torch.Generator(device=dev).manual_seed(8)
    q, k, v = (torch.randn(items, S, D, device=dev, generator=g).bfloat16().requires_grad_(True) for _ in range(3))
    w = torch.randn(items, S, D, device=dev, generator=g).bfloat16()
    layout = block_masks(nb, dev, 9)["window 3"][0].float().to_sparse_csr()
    lens = torch.randint(S // 4, S + 1, (items,), device=dev, generator=g)

    def full():
        return matmuls.block_sparse_attention(q, k, v, layout)

    def ragged():
        return matmuls.block_sparse_attention(q, k, v, layout, q_lens=lens, k_lens=lens)

    def step(fn):
        return lambda: torch.autograd.grad(fn(), (q, k, v), grad_outputs=w)

    res = measure({"full length fwd": full, "lengths fwd": ragged, "full length fwd+bwd": step(full), "lengths fwd+bwd": step(ragged)},
                  args.rounds, args.iters)
    visible = float(((lens + BLOCK - 1) // BLOCK).float().mean()) / nb
    emit(f"\n{items} x {S}^2, window 3, lengths uniform in [{S // 4}, {S}]: {visible:.1%} of the block rows exist")
    show(res)
    emit(f"  ratio lengths / full length: fwd {res['lengths fwd'][0] / res['full length fwd'][0]:.3f}, "
         f"fwd+bwd {res['lengths fwd+bwd'][0] / res['full length fwd+bwd'][0]:.3f}")
    Path(args.log).parent.mkdir(parents=True, exist_ok=True)
    Path(args.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
