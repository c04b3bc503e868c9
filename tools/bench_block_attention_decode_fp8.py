#!/usr/bin/env python3
"""Block-sparse attention for decoding over an FP8 (e4m3fn) KV cache, measured.

    python tools/bench_block_attention_decode_fp8.py [--batches 1,8,64] [--lens 4096,32768,131072] [--pages 16,256]
                                                     [--rounds 5] [--iters 10]
                                                     [--log profiles/r22_block_attention_decode_fp8.log] [--append]

The shapes of tools/bench_block_attention_decode_paged.py: bfloat16 queries, D = 128, Hq = 32 query heads over Hkv = 8 k / v
heads, T = 1 new token at pos = k_len − 1 of a full cache, block 64, chunk=None; the three layouts; the contiguous form and
the paged form at every page size over a shuffled pool.  The fp8 calls run with per-head k and v scales.  The yardstick of
every fp8 call is the bfloat16 call of the same form on the WIDENED cache (the same values in 2 bytes), timed in the SAME
interleaved rounds; each figure is the median over the rounds of the mean of `iters` back-to-back calls between two
events, with the spread (min … max) beside it.  Per row: the time, the kept k / v bytes of that side over 8 TB/s as a
fraction of the HBM roofline, and for the fp8 calls the ratio fp8 / bf16 — flagged where the fp8 call is slower than its
yardstick by more than the yardstick's own min … max spread.  Every row first checks the contract: without scales the fp8
call gives the bits of the yardstick.
"""
import argparse
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention_decode import BLOCK, D, HBM_BYTES_PER_S, HKV, HQ, last_row, measure, square_layout  # noqa: E402
from bench_block_attention_decode_paged import scattered  # noqa: E402

F8 = torch.float8_e4m3fn


def random_codes(shape, dev, g):
    """Finite e4m3fn codes with |x| < 4 and a random sign, uint8 on the device (no fp8 operator of torch is used)."""
    c = torch.randint(0, 0x48, shape, device=dev, dtype=torch.uint8, generator=g)
    return c | (torch.randint(0, 2, shape, device=dev, dtype=torch.uint8, generator=g) << 7)


def widened(codes, lut):
    """The codes as bfloat16 through a 256-entry table made on the CPU, one batch item at a time."""
    out = torch.empty(codes.shape, device=codes.device, dtype=torch.bfloat16)
    for b in range(codes.shape[0]):
        out[b] = lut[codes[b].long()]
    return out


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=ints, default=[1, 8, 64])
    ap.add_argument("--lens", type=ints, default=[4096, 32768, 131072])
    ap.add_argument("--pages", type=ints, default=[16, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r22_block_attention_decode_fp8.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    lut = torch.arange(256, dtype=torch.uint8).view(F8).to(torch.bfloat16).to(dev)
    lines = [f"# tools/bench_block_attention_decode_fp8.py --batches {args.batches} --lens {args.lens} --pages {args.pages} "
             f"--rounds {args.rounds} --iters {args.iters}: ms, median over the rounds [min … max]; bfloat16 queries, D = {D}, "
             f"Hq = {HQ}, Hkv = {HKV}, T = 1, block {BLOCK}, chunk=None; per-head k / v scales; pool pages shuffled; fp8 / bf16: to "
             f"the bfloat16 call of the same form on the widened cache in the same rounds; roofline: that side's kept k / v "
             f"bytes over 8 TB/s; {torch.cuda.get_device_name(0)}"]

    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    log = open(path, "a" if args.append else "w")
    log.write(lines[0] + "\n")

    def emit(line):  # (written row by row: a run that is cut short keeps what it measured)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    ratios, slower = {}, []
    for klen in args.lens:
        nb = klen // BLOCK
        for B in args.batches:
            g = torch.Generator(device=dev).manual_seed(22)
            q = torch.randn(B, HQ, 1, D, device=dev, generator=g).bfloat16()
            kc, vc = random_codes((B, HKV, klen, D), dev, g), random_codes((B, HKV, klen, D), dev, g)
            kw, vw = widened(kc, lut), widened(vc, lut)
            ks = 0.25 + torch.rand(HKV, device=dev, generator=g)
            vs = 0.25 + torch.rand(HKV, device=dev, generator=g)
            lens = torch.full((B,), klen, device=dev, dtype=torch.int32)
            pools = {}
            for page in args.pages:
                W = klen // page
                table = torch.randperm(B * W, device=dev, generator=g).reshape(B, W).to(torch.int32)
                pools[page] = tuple(scattered(x, page, table) for x in (kc, vc, kw, vw)) + (table,)
            for name in ("window 16 + global", "random 10 %", "fully kept"):
                row = last_row(name, nb, dev, 21)
                kept = int(row.sum())
                layout = square_layout(row, nb)
                k8, v8 = kc.view(F8), vc.view(F8)
                pairs = {"contiguous": (
                    lambda **kw_: matmuls.block_sparse_attention_decode_fp8(q, k8, v8, layout, lens, **kw_),
                    lambda: matmuls.block_sparse_attention_decode(q, kw, vw, layout, lens))}
                for page, (kp, vp, kpw, vpw, table) in pools.items():
                    pairs[f"page {page}"] = (
                        lambda kp=kp.view(F8), vp=vp.view(F8), table=table, **kw_: matmuls.block_sparse_attention_decode_paged_fp8(
                            q, kp, vp, table, layout, lens, **kw_),
                        lambda kpw=kpw, vpw=vpw, table=table: matmuls.block_sparse_attention_decode_paged(q, kpw, vpw, table, layout, lens))
                runs = {}
                for n, (f8, bf) in pairs.items():
                    assert torch.equal(f8().view(torch.int16), bf().view(torch.int16)), f"{n}: the fp8 call differs from the widened call"
                    runs[f"bf16, {n}"] = bf
                    runs[f"fp8,  {n}"] = lambda f8=f8: f8(k_scale=ks, v_scale=vs)
                res = measure(runs, args.rounds, args.iters)
                kept_elems = B * HKV * kept * BLOCK * D * 2
                emit(f"\nB = {B}, k_len = {klen}, {name}: {kept} of {nb} blocks kept, {kept_elems * 2 / 2 ** 20:.1f} MiB of k / v in "
                     f"bfloat16, {kept_elems / 2 ** 20:.1f} MiB in fp8")
                for n in pairs:
                    (bm, blo, bhi), (fm, flo, fhi) = res[f"bf16, {n}"], res[f"fp8,  {n}"]
                    emit(f"  bf16, {n:11s} {bm:9.4f}  [{blo:.4f} … {bhi:.4f}]  {kept_elems * 2 / HBM_BYTES_PER_S * 1e3 / bm:6.1%} of the roofline")
                    flag = "" if fm <= bm + (bhi - blo) else "   SLOWER than the yardstick by more than its spread"
                    emit(f"  fp8,  {n:11s} {fm:9.4f}  [{flo:.4f} … {fhi:.4f}]  {kept_elems / HBM_BYTES_PER_S * 1e3 / fm:6.1%} of the roofline  "
                         f"fp8 / bf16 = {fm / bm:5.3f}{flag}")
                    ratios.setdefault((n, name), []).append(fm / bm)
                    if flag:
                        slower.append(f"B = {B}, k_len = {klen}, {name}, {n}")
            del q, kc, vc, kw, vw, pools, pairs, runs
            torch.cuda.empty_cache()
    emit("\n# fp8 / bf16 over the rows of a form and a layout: min … max")
    for (n, name), xs in ratios.items():
        emit(f"  {n:11s} {name:20s} {min(xs):.3f} … {max(xs):.3f}")
    emit(f"# rows where fp8 is slower than its yardstick by more than the yardstick's spread: {len(slower)}" +
         "".join(f"\n#   {s}" for s in slower))
    log.close()


if __name__ == "__main__":
    main()
