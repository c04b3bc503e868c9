#!/usr/bin/env python3
"""The fused KV-cache append, measured.

    python tools/bench_kv_cache_append.py [--decode-batches 1,64] [--prompts 2048,16384] [--prompt-batch 8] [--page 16]
                                          [--rounds 5] [--iters 20] [--log profiles/r23_kv_cache_append.log] [--append]

bfloat16 sources, Hkv = 8, D = 128, the four cache forms: contiguous or paged (a shuffled pool), 2-byte or fp8 with per-head
scales.  Decode steps: T = 1 new token per item at pos = k_len − 1 of a cache of 4096 rows, the lengths spread over the
cache.  Prompt appends: T tokens into an empty cache of T rows, B = 8.  Three routes per row, timed in the SAME interleaved
rounds — each figure the median over the rounds of the mean of `iters` back-to-back calls between two events, the spread
(min … max) beside it:
  fused    kv_cache_append / kv_cache_append_paged: one launch;
  torch    what a caller had before: the positions (and, paged, the pages) computed on the device, one index_put_ for k and
           one for v — for the fp8 forms kv_to_fp8 on the device before them, written through uint8 views;
  copy_    the yardstick of the bandwidth-bound case: two plain copy_ calls of the bytes the form writes (the 2-byte rows,
           or the quantised bytes made beforehand) into [:, :, :T] of a contiguous cache.
Per row: the time, and the bytes the route has to move (read + written) over the time.  Flags: a prompt row where fused is
slower than copy_ by more than copy_'s own min … max spread; a decode row where fused is slower than torch.  Every row first
checks that the fused call and the torch route leave the same cache.
"""
import argparse
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "matrix-multiplication_amd"))
sys.path.insert(0, str(REPO / "tools"))

from bench_block_attention_decode import measure  # noqa: E402

F8 = torch.float8_e4m3fn
HKV, D = 8, 128


def torch_route(matmuls, k_new, v_new, k, v, lens, table, scales):
    """The append with torch operators alone; nothing is read back.  k, v: the cache or the pool (fp8: as uint8 views)."""
    B, H, T, _ = k_new.shape
    dev = k_new.device
    pos = lens[:, None] - T + torch.arange(T, device=dev)[None, :]          # [B, T]; in range in every row of this tool
    hi = torch.arange(H, device=dev)[None, :, None]
    if table is None:
        outer, row = torch.arange(B, device=dev)[:, None, None], pos[:, None, :]
    else:
        page = k.shape[2]
        outer, row = table.gather(1, (pos // page).long()).long()[:, None, :], (pos % page)[:, None, :]
    for x, cache, s in ((k_new, k, scales[0]), (v_new, v, scales[1])):
        if cache.dtype == torch.uint8:
            x = matmuls.kv_to_fp8(x, s)[0].view(torch.uint8)
        cache.index_put_((outer, hi, row), x)


def main():
    ints = lambda s: [int(x) for x in s.split(",") if x]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode-batches", type=ints, default=[1, 64])
    ap.add_argument("--decode-smax", type=int, default=4096)
    ap.add_argument("--prompts", type=ints, default=[2048, 16384])
    ap.add_argument("--prompt-batch", type=int, default=8)
    ap.add_argument("--page", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--log", default=str(REPO / "profiles" / "r23_kv_cache_append.log"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import matmuls
    dev = torch.device("cuda:0")
    path = Path(args.log)
    path.parent.mkdir(parents=True, exist_ok=True)
    log = open(path, "a" if args.append else "w")

    def emit(line):  # (written row by row: a run that is cut short keeps what it measured)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    emit(f"# tools/bench_kv_cache_append.py --decode-batches {args.decode_batches} --decode-smax {args.decode_smax} --prompts "
         f"{args.prompts} --prompt-batch {args.prompt_batch} --page {args.page} --rounds {args.rounds} --iters {args.iters}: ms, "
         f"median over the rounds [min … max]; bfloat16 source, Hkv = {HKV}, D = {D}; GB/s: the bytes the route reads and writes "
         f"over the time; {torch.cuda.get_device_name(0)}")
    cases = [("decode", B, 1, args.decode_smax) for B in args.decode_batches] + [("prompt", args.prompt_batch, T, T) for T in args.prompts]
    missed = []
    for kind, B, T, smax in cases:
        g = torch.Generator(device=dev).manual_seed(23)
        k_new, v_new = (torch.randn(B, HKV, T, D, device=dev, generator=g).bfloat16() for _ in range(2))
        if kind == "decode":
            lens = (torch.randint(smax // 4, smax, (B,), device=dev, generator=g) + 1).to(torch.int32)
        else:
            lens = torch.full((B,), T, device=dev, dtype=torch.int32)
        ks, vs = 0.01 + 0.02 * torch.rand(HKV, device=dev, generator=g), 0.01 + 0.02 * torch.rand(HKV, device=dev, generator=g)
        elems = B * HKV * T * D
        emit(f"\n{kind}: B = {B}, T = {T}, cache rows {smax}: {2 * elems * 2 / 2 ** 20:.2f} MiB of new k and v")
        for fp8 in (False, True):
            for paged in (False, True):
                form = f"{'fp8 ' if fp8 else 'bf16'} {'paged' if paged else 'flat '}"
                cdt = torch.uint8 if fp8 else torch.bfloat16
                W = smax // args.page
                shape = (B * W, HKV, args.page, D) if paged else (B, HKV, smax, D)
                table = torch.randperm(B * W, device=dev, generator=g).reshape(B, W).to(torch.int32) if paged else None
                k, v, k2, v2 = (torch.zeros(shape, device=dev, dtype=cdt) for _ in range(4))
                yk, yv = (torch.zeros((B, HKV, smax, D), device=dev, dtype=cdt) for _ in range(2))
                scales = (ks, vs) if fp8 else (None, None)
                kw = dict(k_scale=ks, v_scale=vs) if fp8 else {}
                view = (lambda t: t.view(F8)) if fp8 else (lambda t: t)
                if paged:
                    fused = lambda k=k, v=v: matmuls.kv_cache_append_paged(k_new, v_new, view(k), view(v), table, lens, **kw)  # noqa: E731
                else:
                    fused = lambda k=k, v=v: matmuls.kv_cache_append(k_new, v_new, view(k), view(v), lens, **kw)  # noqa: E731
                runs = {"fused": fused}
                try:
                    torch_route(matmuls, k_new, v_new, k2, v2, lens, table, scales)
                    fused()
                    torch.cuda.synchronize()
                    assert torch.equal(k, k2) and torch.equal(v, v2), f"{form}: the fused call and the torch route differ"
                    runs["torch"] = lambda k2=k2, v2=v2: torch_route(matmuls, k_new, v_new, k2, v2, lens, table, scales)
                except (RuntimeError, NotImplementedError) as e:  # (an fp8 operator torch lacks on this device)
                    emit(f"  {form}: the torch route does not run here: {str(e).splitlines()[0][:120]}")
                src_k, src_v = (matmuls.kv_to_fp8(x, s)[0].view(torch.uint8) for x, s in ((k_new, ks), (v_new, vs))) if "torch" in runs and fp8 \
                    else (k_new, v_new)
                if src_k.dtype == cdt:
                    def copies(yk=yk, yv=yv, src_k=src_k, src_v=src_v):
                        yk[:, :, :T].copy_(src_k)
                        yv[:, :, :T].copy_(src_v)
                    runs["copy_"] = copies
                res = measure(runs, args.rounds, args.iters)
                moved = {"fused": 2 * elems * (2 + (1 if fp8 else 2)), "torch": 2 * elems * (2 + (1 if fp8 else 2)),
                         "copy_": 2 * elems * 2 * (1 if fp8 else 2)}
                for n, (m, lo, hi) in res.items():
                    emit(f"  {form}  {n:6s} {m:9.4f}  [{lo:.4f} … {hi:.4f}]  {moved[n] / m / 1e6:9.1f} GB/s")
                fm = res["fused"][0]
                if kind == "prompt" and "copy_" in res:
                    cm, clo, chi = res["copy_"]
                    ok = fm <= cm + (chi - clo)
                    emit(f"  {form}  fused / copy_ = {fm / cm:5.3f}" + ("" if ok else "   SLOWER than the yardstick by more than its spread"))
                    if not ok:
                        missed.append(f"{kind} B = {B}, T = {T}, {form}: fused {fm:.4f} ms, copy_ {cm:.4f} ms [{clo:.4f} … {chi:.4f}]")
                if "torch" in res:
                    tm = res["torch"][0]
                    ok = kind != "decode" or fm <= tm
                    emit(f"  {form}  fused / torch = {fm / tm:5.3f}" + ("" if ok else "   SLOWER than the torch route"))
                    if not ok:
                        missed.append(f"{kind} B = {B}, T = {T}, {form}: fused {fm:.4f} ms, torch {tm:.4f} ms")
                del k, v, k2, v2, yk, yv, runs, fused
                torch.cuda.empty_cache()
    emit(f"\n# rows that miss the condition (prompt: fused ≤ copy_ + copy_'s spread; decode: fused ≤ torch): {len(missed)}" +
         "".join(f"\n#   {s}" for s in missed))
    log.close()


if __name__ == "__main__":
    main()
