#!/usr/bin/env python3
"""Block-sparse attention for decoding, measured.

    python tools/bench_block_attention_decode.py [--batches 1,8,64] [--lens 4096,32768,131072] [--rounds 5] [--iters 10]
                                                 [--chunks 4,8,16,32,64] [--log profiles/r20_block_attention_decode.log] [--append]

bfloat16, D = 128, Hq = 32 query heads over Hkv = 8 k / v heads, T = 1 new token at pos = k_len − 1 of a full cache
(Smax = k_len), block 64.  Layouts: a window of 16 blocks + 1 global block; random 10 % of the blocks (+ the diagonal);
fully kept.  Contestants of a row are timed in interleaved rounds, each figure the median over the rounds of the mean of
`iters` back-to-back calls between two events, with the spread (min … max) beside it:
  decode            matmuls.block_sparse_attention_decode with chunk=None, and with every chunk of --chunks (the sweep the
                    default is fitted on);
  padded            the route the parent has: the token padded into a 64-row query block, block_sparse_attention on the
                    one-row layout with k_lens;
  dense sdpa        torch's scaled_dot_product_attention on the cache with the token's dense boolean mask and enable_gqa
                    (left out, and said so, above --dense-cap-gib of cache: it expands what it reads).
Per row: the time, and the kept k / v bytes of the token's layout row over 8 TB/s as a fraction of the HBM roofline.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention import timed  # noqa: E402

D, BLOCK, HQ, HKV = 128, 64, 32, 8
HBM_BYTES_PER_S = 8e12


def last_row(name, nb, dev, seed):
    """The kept block columns of layout row nb − 1 (the decode token's), as a boolean [nb]."""
    keep = torch.zeros(nb, dtype=torch.bool, device=dev)
    if name == "window 16 + global":
        keep[max(0, nb - 16):] = True
        keep[0] = True
    elif name == "random 10 %":
        g = torch.Generator(device=dev).manual_seed(seed)
        keep[torch.randperm(nb, device=dev, generator=g)[:max(1, round(0.1 * nb))]] = True
        keep[nb - 1] = True
    else:
        keep[:] = True
    return keep


def square_layout(row, nb):
    """A CSR layout [nb, nb] whose last row is `row` and whose other rows keep their diagonal block: what decode reads
    of a layout is the row of pos alone."""
    dev = row.device
    cols = torch.cat([torch.arange(nb - 1, device=dev), torch.nonzero(row).flatten()])
    crow = torch.cat([torch.arange(nb, device=dev), torch.tensor([nb - 1 + int(row.sum())], device=dev)])
    return torch.sparse_csr_tensor(crow, cols, torch.ones(cols.numel(), device=dev), size=(nb, nb))


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


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=ints, default=[1, 8, 64])
    ap.add_argument("--lens", type=ints, default=[4096, 32768, 131072])
    ap.add_argument("--chunks", type=ints, default=[4, 8, 16, 32, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dense-cap-gib", type=float, default=4.0)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r20_block_attention_decode.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_block_attention_decode.py --batches {args.batches} --lens {args.lens} --rounds {args.rounds} --iters "
             f"{args.iters}: ms, median over the rounds [min … max]; bfloat16, D = {D}, Hq = {HQ}, Hkv = {HKV}, T = 1, block "
             f"{BLOCK}; roofline: kept k / v bytes over 8 TB/s; {torch.cuda.get_device_name(0)}"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    best = {}  # k_len -> {chunk: [time / best time of the row]}
    for klen in args.lens:
        nb = klen // BLOCK
        for B in args.batches:
            g = torch.Generator(device=dev).manual_seed(20)
            q = torch.randn(B, HQ, 1, D, device=dev, generator=g).bfloat16()
            k = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            v = torch.randn(B, HKV, klen, D, device=dev, dtype=torch.bfloat16, generator=g)
            lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
            qpad = torch.zeros(B, HQ, BLOCK, D, device=dev, dtype=torch.bfloat16)
            qpad[:, :, -1:] = q
            cache_gib = 2 * k.numel() * 2 / 2 ** 30
            for name in ("window 16 + global", "random 10 %", "fully kept"):
                row = last_row(name, nb, dev, 21)
                kept = int(row.sum())
                layout = square_layout(row, nb)
                one_row = torch.sparse_csr_tensor(torch.tensor([0, kept], device=dev), torch.nonzero(row).flatten(),
                                                  torch.ones(kept, device=dev), size=(1, nb))
                runs = {"decode chunk=None": lambda: matmuls.block_sparse_attention_decode(q, k, v, layout, lens)}
                for c in args.chunks:
                    runs[f"decode chunk={c}"] = lambda c=c: matmuls.block_sparse_attention_decode(q, k, v, layout, lens, chunk=c)
                runs["padded block_sparse_attention"] = lambda: matmuls.block_sparse_attention(qpad, k, v, one_row, k_lens=lens)
                if cache_gib <= args.dense_cap_gib:
                    mask = row.repeat_interleave(BLOCK)[None, None, None, :]
                    runs["dense sdpa"] = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, enable_gqa=True)
                res = measure(runs, args.rounds, args.iters)
                kept_bytes = B * HKV * kept * BLOCK * D * 2 * 2
                floor_ms = kept_bytes / HBM_BYTES_PER_S * 1e3
                emit(f"\nB = {B}, k_len = {klen}, {name}: {kept} of {nb} blocks kept, {kept_bytes / 2 ** 20:.1f} MiB of k / v, "
                     f"{floor_ms:.4f} ms at 8 TB/s")
                for n, (med, lo, hi) in res.items():
                    emit(f"  {n:32s} {med:9.4f}  [{lo:.4f} … {hi:.4f}]  {floor_ms / med:6.1%} of the roofline")
                if cache_gib > args.dense_cap_gib:
                    emit(f"  dense sdpa                       left out: {cache_gib:.1f} GiB of cache is above the cap")
                sweep = {c: res[f"decode chunk={c}"][0] for c in args.chunks}
                low = min(sweep.values())
                for c, t in sweep.items():
                    best.setdefault(klen, {}).setdefault(c, []).append(t / low)
            del q, k, v, qpad
            torch.cuda.empty_cache()
    emit("\n# the chunk sweep: geometric mean over the rows of a k_len of (time / the row's best time)")
    for klen, per in best.items():
        gm = {c: statistics.geometric_mean(xs) for c, xs in per.items()}
        emit(f"  k_len = {klen}: " + ", ".join(f"chunk {c}: {x:.3f}" for c, x in gm.items()) + f"  -> best {min(gm, key=gm.get)}")
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
