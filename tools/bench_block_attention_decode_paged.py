#!/usr/bin/env python3
"""Block-sparse attention for decoding over a paged KV cache, measured.

    python tools/bench_block_attention_decode_paged.py [--batches 1,8,64] [--lens 4096,32768,131072] [--pages 16,64,256]
                                                       [--rounds 5] [--iters 10]
                                                       [--log profiles/r21_block_attention_decode_paged.log] [--append]

The shapes of tools/bench_block_attention_decode.py: bfloat16, D = 128, Hq = 32 query heads over Hkv = 8 k / v heads, T = 1
new token at pos = k_len − 1 of a full cache (Smax = k_len), block 64, chunk=None; layouts: a window of 16 blocks + 1 global
block, random 10 % of the blocks (+ the diagonal), fully kept.  For every page size the cache is scattered into a pool
[P, Hkv, page, D] of P = B · k_len / page pages under a seeded SHUFFLE of the pool pages, so physical neighbours are not
logical neighbours.  The yardstick is matmuls.block_sparse_attention_decode on the same content stored contiguously, timed
in the SAME interleaved rounds as the paged calls; each figure is the median over the rounds of the mean of `iters`
back-to-back calls between two events, with the spread (min … max) beside it.  Per row: the time, the ratio to the
contiguous call, and the kept k / v bytes of the token's layout row over 8 TB/s as a fraction of the HBM roofline.  The
results are checked once per row: the paged call must give the bits of the contiguous call.
"""
import argparse
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention_decode import BLOCK, D, HBM_BYTES_PER_S, HKV, HQ, last_row, measure, square_layout  # noqa: E402


def scattered(x, page, table):
    """The cache x [B, Hkv, Smax, D] as a pool [P, Hkv, page, D] with logical page (b, w) at pool page table[b, w]."""
    B, H, S, _ = x.shape
    W = S // page
    pool = torch.empty(B * W, H, page, D, device=x.device, dtype=x.dtype)
    pool[table.long().reshape(-1)] = x.reshape(B, H, W, page, D).permute(0, 2, 1, 3, 4).reshape(B * W, H, page, D)
    return pool


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=ints, default=[1, 8, 64])
    ap.add_argument("--lens", type=ints, default=[4096, 32768, 131072])
    ap.add_argument("--pages", type=ints, default=[16, 64, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r21_block_attention_decode_paged.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_block_attention_decode_paged.py --batches {args.batches} --lens {args.lens} --pages {args.pages} "
             f"--rounds {args.rounds} --iters {args.iters}: ms, median over the rounds [min … max]; bfloat16, D = {D}, Hq = {HQ}, "
             f"Hkv = {HKV}, T = 1, block {BLOCK}, chunk=None; pool pages shuffled; ratio: to the contiguous call of the same "
             f"rounds; roofline: kept k / v bytes over 8 TB/s; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    ratios = {p: [] for p in args.pages}
    for klen in args.lens:
        nb = klen // BLOCK
        for B in args.batches:
            g = torch.Generator(device=dev).manual_seed(20)
            q = torch.randn(B, HQ, 1, D, device=dev, generator=g).bfloat16()
            k = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            v = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
            pools = {}
            for page in args.pages:
                W = klen // page
                table = torch.randperm(B * W, device=dev, generator=g).reshape(B, W).to(torch.int32)
                pools[page] = (scattered(k, page, table), scattered(v, page, table), table)
            for name in ("window 16 + global", "random 10 %", "fully kept"):
                row = last_row(name, nb, dev, 21)
                kept = int(row.sum())
                layout = square_layout(row, nb)
                runs = {"contiguous": lambda: matmuls.block_sparse_attention_decode(q, k, v, layout, lens)}
                for page, (kp, vp, table) in pools.items():
                    runs[f"paged, page {page}"] = lambda kp=kp, vp=vp, table=table: matmuls.block_sparse_attention_decode_paged(
                        q, kp, vp, table, layout, lens)
                want = runs["contiguous"]()
                for n, fn in runs.items():
                    assert torch.equal(fn().view(torch.int16), want.view(torch.int16)), f"{n}: bits differ from the contiguous call"
                res = measure(runs, args.rounds, args.iters)
                kept_bytes = B * HKV * kept * BLOCK * D * 2 * 2
                floor_ms = kept_bytes / HBM_BYTES_PER_S * 1e3
                emit(f"\nB = {B}, k_len = {klen}, {name}: {kept} of {nb} blocks kept, {kept_bytes / 2 ** 20:.1f} MiB of k / v, "
                     f"{floor_ms:.4f} ms at 8 TB/s")
                base = res["contiguous"][0]
                for n, (med, lo, hi) in res.items():
                    emit(f"  {n:18s} {med:9.4f}  [{lo:.4f} … {hi:.4f}]  x{med / base:5.3f} of contiguous  {floor_ms / med:6.1%} of the roofline")
                for page in args.pages:
                    ratios[page].append(res[f"paged, page {page}"][0] / base)
            del q, k, v, pools
            torch.cuda.empty_cache()
    emit("\n# ratio to the contiguous call over the rows: min … max")
    for page, xs in ratios.items():
        emit(f"  page {page}: {min(xs):.3f} … {max(xs):.3f}" + ("" if max(xs) <= 1.10 else "   (above 1.10 in "
             f"{sum(x > 1.10 for x in xs)} of {len(xs)} rows)"))
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
