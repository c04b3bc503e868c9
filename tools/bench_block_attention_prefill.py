#!/usr/bin/env python3
"""Block-sparse prefill attention over the KV cache, measured.

    python tools/bench_block_attention_prefill.py [--rounds 3] [--iters 3] [--limit 240]
                                                  [--log profiles/r26_block_attention_prefill.log] [--append]
    python tools/bench_block_attention_prefill.py --case whole:4096:1 --log …        (one case, in this process)

bfloat16, D = 128, Hq = 32 query heads over Hkv = 8 k / v heads, block 64; layouts over the whole [nb, nb] grid: a window of 16
blocks + 1 global block, random 10 % of the lower triangle (+ the diagonal), fully kept.  Cases:
  whole:K:B   a whole prompt, T = k_len = K, batch B.  Yardstick: block_sparse_attention(causal=True) on the contiguous bf16
              cache — the same instruction stream but for addressing; expectation: the contiguous 2-byte form within 1.10 × of it.
  chunk:K:T   a chunk of T tokens against k_len = K (B = 1).  Yardstick: block_sparse_attention_decode with the same T, the
              only route before this call; the ratio is reported, no figure fixed in advance.
In every case the four cache forms — contiguous, paged (pages of 16 and of 256 keys, pool pages shuffled), fp8 with per-head
scales, paged fp8 (page 16) — run in the SAME interleaved rounds as the yardstick; each figure is the median over the rounds
of the mean of `iters` back-to-back calls between two events, with the spread (min … max) beside it, the ratio to the
contiguous 2-byte form and the matrix-core rate over the blocks computed (4 · 64 · 64 · D flop per block pair and query head).
The paged call is checked once per row against the bits of the contiguous call, the whole-prompt call against those of the
training call.  Without --case every case runs as a fresh child process under its own time limit (--limit seconds); the
first child that fails or runs out of time ends the run.  The grouped placement of the heads (8 workgroups apart) against
plain row-major order has no switch in the kernel and is NOT measured here.
"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention import timed  # noqa: E402

D, BLOCK, HQ, HKV = 128, 64, 32, 8
CASES = [f"whole:{K}:{B}" for K in (4096, 16384) for B in (1, 8)] + [f"chunk:{K}:{T}" for T in (512, 2048) for K in (8192, 32768, 131072)]
LAYOUTS = ("window 16 + global", "random 10 %", "fully kept")


def block_mask(name, nb, dev, seed):
    """Boolean [nb, nb]: the kept blocks of the lower triangle (what a causal walk computes), the diagonal always kept."""
    i = torch.arange(nb, device=dev)
    lower = i[:, None] >= i[None, :]
    if name == "window 16 + global":
        keep = (i[:, None] - i[None, :] < 16) | (i[None, :] == 0)
    elif name == "random 10 %":
        keep = torch.rand((nb, nb), device=dev, generator=torch.Generator(device=dev).manual_seed(seed)) < 0.10
    else:
        keep = torch.ones((nb, nb), dtype=torch.bool, device=dev)
    return (keep & lower) | (i[:, None] == i[None, :])


def scattered(x, page, table):
    """The cache x [B, Hkv, Smax, D] as a pool [P, Hkv, page, D] with logical page (b, w) at pool page table[b, w]."""
    B, H, S, _ = x.shape
    W = S // page
    pool = torch.empty(B * W, H, page, D, device=x.device, dtype=x.dtype)
    pool[table.long().reshape(-1)] = x.reshape(B, H, W, page, D).permute(0, 2, 1, 3, 4).reshape(B * W, H, page, D)
    return pool


def measure(runs, rounds, iters):
    for fn in runs.values():  # warm-up: every kernel loaded, the layouts' lists built
        fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in runs}
    for _ in range(rounds):
        for n, fn in runs.items():
            samples[n].append(timed(fn, iters))
    return {n: (statistics.median(xs), min(xs), max(xs)) for n, xs in samples.items()}


def run_case(case, rounds, iters, emit):
    import matmuls
    kind, K, X = case.split(":")
    K, X = int(K), int(X)
    B, T = (X, K) if kind == "whole" else (1, X)
    dev = torch.device("cuda:0")
    nb = K // BLOCK
    g = torch.Generator(device=dev).manual_seed(26)
    q = torch.randn(B, HQ, T, D, device=dev, generator=g).bfloat16()
    k = torch.randn(B, HKV, K, D, device=dev, dtype=torch.bfloat16, generator=g)
    v = torch.randn(B, HKV, K, D, device=dev, dtype=torch.bfloat16, generator=g)
    lens = torch.full((B,), K, device=dev, dtype=torch.int32)
    pools = {}
    for page in (16, 256):
        table = torch.randperm(B * (K // page), device=dev, generator=g).reshape(B, K // page).to(torch.int32)
        pools[page] = (scattered(k, page, table), scattered(v, page, table), table)
    k8, ks = matmuls.kv_to_fp8(k)
    v8, vs = matmuls.kv_to_fp8(v)
    kp8, vp8 = (scattered(x.view(torch.uint8), 16, pools[16][2]).view(torch.float8_e4m3fn) for x in (k8, v8))
    for name in LAYOUTS:
        mask = block_mask(name, nb, dev, 27)
        layout = mask.float().to_sparse_csr()
        first = (K - T) // BLOCK  # the layout rows of the T tokens
        pairs = int(mask[first:].sum()) * B * HQ
        runs = {"contiguous": lambda: matmuls.block_sparse_attention_prefill(q, k, v, layout, lens)}
        for page, (kp, vp, table) in pools.items():
            runs[f"paged, page {page}"] = lambda kp=kp, vp=vp, table=table: matmuls.block_sparse_attention_prefill_paged(
                q, kp, vp, table, layout, lens)
        runs["fp8"] = lambda: matmuls.block_sparse_attention_prefill_fp8(q, k8, v8, layout, lens, k_scale=ks, v_scale=vs)
        runs["paged fp8, page 16"] = lambda: matmuls.block_sparse_attention_prefill_paged_fp8(q, kp8, vp8, pools[16][2], layout, lens,
                                                                                              k_scale=ks, v_scale=vs)
        if kind == "whole":
            runs["training call"] = lambda: matmuls.block_sparse_attention(q, k, v, layout, causal=True)
        else:
            runs["decode call"] = lambda: matmuls.block_sparse_attention_decode(q, k, v, layout, lens)
        want = runs["contiguous"]().view(torch.int16)
        checks = [f"{n}: bits {'equal' if torch.equal(runs[n]().view(torch.int16), want) else 'DIFFER'}"
                  for n in runs if n.startswith("paged, ") or n == "training call"]
        res = measure(runs, rounds, iters)
        emit(f"\n{case}, B = {B}, T = {T}, k_len = {K}, {name}: {pairs // (B * HQ)} block pairs per head; " + "; ".join(checks))
        base = res["contiguous"][0]
        for n, (med, lo, hi) in res.items():
            emit(f"  {n:20s} {med:10.4f}  [{lo:.4f} … {hi:.4f}]  x{med / base:6.3f} of contiguous  "
                 f"{pairs * 4 * BLOCK * BLOCK * D / (med * 1e-3) / 1e12:7.1f} TFLOP/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r26_block_attention_prefill.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    if args.case is None:
        with open(path, "a" if args.append else "w") as f:
            f.write(f"# tools/bench_block_attention_prefill.py --rounds {args.rounds} --iters {args.iters}: ms, median over the rounds "
                    f"[min … max]; bfloat16, D = {D}, Hq = {HQ}, Hkv = {HKV}, block {BLOCK}; ratio: to the contiguous 2-byte form of "
                    f"the same rounds; {torch.cuda.get_device_name(0)}\n")
        for case in args.cases.split(","):
            try:  # a fresh child per case, under its own time limit; nothing more is started after a failure
                rc = subprocess.run([sys.executable, __file__, "--case", case, "--rounds", str(args.rounds), "--iters", str(args.iters),
                                     "--log", str(path)], timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                with open(path, "a") as f:
                    f.write(f"\n{case}: ended with status {rc}; the run stops here\n")
                sys.exit(rc)
        return
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    run_case(args.case, args.rounds, args.iters, emit)
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
