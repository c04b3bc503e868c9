#!/usr/bin/env python3
"""The fused rotary embedding + KV-cache append, measured.

    python tools/bench_rope_kv_append.py [--decode-batches 1,64] [--prompts 2048,16384] [--prompt-batch 8] [--page 16]
                                         [--rounds 5] [--iters 20] [--log profiles/r25_rope_kv_append.log] [--append]

bfloat16, Hq = 32, Hkv = 8, D = 128 = rotary_dim (the NeoX halves), the four cache forms: contiguous or paged (page 16 over a
shuffled pool), 2-byte or fp8 with per-head scales.  Decode steps: T = 1 new token per item at pos = k_len − 1 of a cache of
4096 rows, the lengths spread over the cache.  Prompt steps: T tokens into an empty cache of T rows, B = 8.  Three routes per
row, timed in the SAME interleaved rounds — each figure the median over the rounds of the mean of `iters` back-to-back calls
between two events, the spread (min … max) beside it:
  a  fused  rope_kv_cache_append / rope_kv_cache_append_paged: one launch;
  b  torch  what a caller had before: the positions from k_lens on the device, cos[pos] / sin[pos] gathered, the halves
            sliced, (a.float() * c − b.float() * s).to(dtype) and its partner for q and again for k, a cat each — then
            kv_cache_append of the rotated k and v;
  c  bytes  kv_cache_append of the same tokens (unrotated) plus one copy_ of q's bytes: the bytes the fused call cannot avoid
            moving, in the two launches that move them.
Every row first checks that routes a and b leave the same cache and the same q.  Flags: a decode row where a is slower than b;
a prompt row where a is slower than c by more than c's own min … max spread.
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
HQ, HKV, D = 32, 8, 128


def rotate(x, c, s):
    """The contract's torch expression on the device: x [B, H, T, D], c and s [B, 1, T, D/2] float32."""
    a, b = x[..., :D // 2].float(), x[..., D // 2:].float()
    return torch.cat([(a * c - b * s).to(x.dtype), (b * c + a * s).to(x.dtype)], -1)


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
    ap.add_argument("--log", default=str(REPO / "profiles" / "r25_rope_kv_append.log"))
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

    emit(f"# tools/bench_rope_kv_append.py --decode-batches {args.decode_batches} --decode-smax {args.decode_smax} --prompts "
         f"{args.prompts} --prompt-batch {args.prompt_batch} --page {args.page} --rounds {args.rounds} --iters {args.iters}: ms, "
         f"median over the rounds [min … max]; bfloat16, Hq = {HQ}, Hkv = {HKV}, D = rotary_dim = {D}, NeoX halves; "
         f"{torch.cuda.get_device_name(0)}")
    cases = [("decode", B, 1, args.decode_smax) for B in args.decode_batches] + [("prompt", args.prompt_batch, T, T) for T in args.prompts]
    missed = []
    for kind, B, T, smax in cases:
        g = torch.Generator(device=dev).manual_seed(25)
        qkv = torch.randn(B, T, HQ + 2 * HKV, D, device=dev, generator=g).bfloat16()      # one fused projection, sliced
        q, k_new, v_new = (qkv[:, :, lo:hi].transpose(1, 2) for lo, hi in ((0, HQ), (HQ, HQ + HKV), (HQ + HKV, HQ + 2 * HKV)))
        if kind == "decode":
            lens = (torch.randint(smax // 4, smax, (B,), device=dev, generator=g) + 1).to(torch.int32)
        else:
            lens = torch.full((B,), T, device=dev, dtype=torch.int32)
        ang = torch.arange(smax, device=dev, dtype=torch.float64)[:, None] * \
            10000.0 ** (-2.0 * torch.arange(D // 2, device=dev, dtype=torch.float64) / D)
        cos, sin = ang.cos().float(), ang.sin().float()
        ks, vs = 0.01 + 0.02 * torch.rand(HKV, device=dev, generator=g), 0.01 + 0.02 * torch.rand(HKV, device=dev, generator=g)
        iters = args.iters if kind == "decode" else max(args.iters // 2, 1)
        emit(f"\n{kind}: B = {B}, T = {T}, cache rows {smax}: {q.numel() * 2 / 2 ** 20:.2f} MiB of q, "
             f"{2 * k_new.numel() * 2 / 2 ** 20:.2f} MiB of new k and v")
        for fp8 in (False, True):
            for paged in (False, True):
                form = f"{'fp8 ' if fp8 else 'bf16'} {'paged' if paged else 'flat '}"
                cdt = torch.uint8 if fp8 else torch.bfloat16
                W = smax // args.page
                shape = (B * W, HKV, args.page, D) if paged else (B, HKV, smax, D)
                table = torch.randperm(B * W, device=dev, generator=g).reshape(B, W).to(torch.int32) if paged else None
                k, v, k2, v2, k3, v3 = (torch.zeros(shape, device=dev, dtype=cdt) for _ in range(6))
                qa, qc = (torch.empty(B, HQ, T, D, device=dev, dtype=torch.bfloat16) for _ in range(2))
                kw = dict(k_scale=ks, v_scale=vs) if fp8 else {}
                view = (lambda t: t.view(F8)) if fp8 else (lambda t: t)

                def append(kn, kc, vc):
                    if paged:
                        matmuls.kv_cache_append_paged(kn, v_new, view(kc), view(vc), table, lens, **kw)
                    else:
                        matmuls.kv_cache_append(kn, v_new, view(kc), view(vc), lens, **kw)

                def fused():
                    if paged:
                        return matmuls.rope_kv_cache_append_paged(q, k_new, v_new, cos, sin, view(k), view(v), table, lens, q_out=qa, **kw)
                    return matmuls.rope_kv_cache_append(q, k_new, v_new, cos, sin, view(k), view(v), lens, q_out=qa, **kw)

                def torch_route():
                    pos = (lens[:, None] - T + torch.arange(T, device=dev)[None, :]).long()      # in range in every row of this tool
                    c, s = cos[pos][:, None], sin[pos][:, None]
                    q_rot = rotate(q, c, s)
                    append(rotate(k_new, c, s), k2, v2)
                    return q_rot

                def bytes_route():
                    append(k_new, k3, v3)
                    qc.copy_(q)

                fused()
                q_rot = torch_route()
                torch.cuda.synchronize()
                assert torch.equal(qa, q_rot) and torch.equal(k, k2) and torch.equal(v, v2), f"{form}: routes a and b differ"
                del q_rot
                res = measure({"a fused": fused, "b torch": torch_route, "c bytes": bytes_route}, args.rounds, iters)
                for n, (m, lo, hi) in res.items():
                    emit(f"  {form}  {n:8s} {m:9.4f}  [{lo:.4f} … {hi:.4f}]")
                (am, _, _), (bm, _, _), (cm, clo, chi) = res["a fused"], res["b torch"], res["c bytes"]
                ok = am <= bm if kind == "decode" else am <= cm + (chi - clo)
                emit(f"  {form}  a / b = {am / bm:5.3f}   a / c = {am / cm:5.3f}" +
                     ("" if ok else ("   SLOWER than the torch route" if kind == "decode" else "   SLOWER than the bytes' route by more than its spread")))
                if not ok:
                    missed.append(f"{kind} B = {B}, T = {T}, {form}: a {am:.4f} ms, b {bm:.4f} ms, c {cm:.4f} ms [{clo:.4f} … {chi:.4f}]")
                del k, v, k2, v2, k3, v3, qa, qc
                torch.cuda.empty_cache()
        del qkv, q, k_new, v_new
        torch.cuda.empty_cache()
    emit(f"\n# rows that miss the expectation (decode: a ≤ b; prompt: a ≤ c + c's spread): {len(missed)}" + "".join(f"\n#   {s}" for s in missed))
    log.close()


if __name__ == "__main__":
    main()
