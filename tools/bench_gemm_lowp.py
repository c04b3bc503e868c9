"""bfloat16 / float16 dense products against our fp32 path and torch.matmul in bf16 (hipBLASLt), in one process.

    python tools/bench_gemm_lowp.py [--only TAG] [--log FILE]
    bash tools/kstats.sh lowp_attn python $PWD/tools/bench_gemm_lowp.py --profile attn   (per-kernel table of the bf16
                                                                                         attention step)

Shapes: 4096³ and 8192³ NN and NT (uniform [−1, 1)); BERT-base attention (B 32, H 12, S 512, D 64): q·kᵀ, probs·V and the
step of bench.py's C5 (scores = cublasTransbMM.apply(q, k), ctx = cublasMM.apply(probs, v), both backward) — the same
step through torch.matmul for torch; the FC layer 16384 × 3072 → 768 (NT) and its weight gradient (TN, k = 16384); the
ragged / unaligned 197-token probs·V (384 items) and 4095³.  Per shape, interleaved medians (ms) of ours in bf16, fp16
and fp32 (custom_mm.cublas_mmul / cublas_bmm, or the classes for the step) and torch.matmul in bf16, TFLOP/s, and the
ratios ours-bf16 / torch-bf16 and ours-bf16 / ours-fp32.  Sampled output rows of bf16 and fp16 are checked against
|C − E| ≤ u_T·|E| + k·2⁻²³·(|A|·|B|) (+ 2⁻²⁵ for fp16), E the float64 product (tests/test_gpu_gemm_lowp.py, test 3).
"""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "matrix-multiplication_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import custom_mm  # noqa: E402
import matmuls  # noqa: E402
from bench_hbm_regime import time_interleaved  # noqa: E402

dev = torch.device("cuda")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ABS = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}


def uniform(shape, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(shape, device=dev, generator=g) * 2 - 1


def op(x, t):
    return x.transpose(-1, -2) if t else x


def ours(a, b, c, ta, tb):
    '''Our product on STORED operands (A stored k×m when ta, B stored n×k when tb), any rank up to 4.'''
    if a.dim() == 2:
        return lambda: custom_mm.cublas_mmul(a, b, c, ta, tb)
    return lambda: custom_mm.cublas_bmm(a, b, c, a.dim(), ta, tb)


def check(a, b, c, ta, tb, rows=48, seed=0):
    '''Sampled rows of C (of the first item when batched) within the accuracy bound against the float64 product.'''
    a0, b0, c0 = (x.reshape((-1,) + tuple(x.shape[-2:]))[0] for x in (a, b, c))
    A, B = op(a0, ta), op(b0, tb)
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(A.shape[0], generator=g)[:rows].to(dev)
    E = A[idx].double() @ B.double()
    S = A[idx].double().abs() @ B.double().abs()
    tol = U[c.dtype] * E.abs() + A.shape[1] * 2.0 ** -23 * S + ABS[c.dtype]
    return bool(((c0[idx].double() - E).abs() <= tol).all())


def product_shape(tag, shape_a, shape_b, ta, tb, flops, gen=uniform, out=None):
    t0 = time.time()
    a32, b32 = gen(shape_a, 1), gen(shape_b, 2)
    ops = {k: (a32.to(dt), b32.to(dt)) for k, dt in DT.items()}
    m = shape_a[-1] if ta else shape_a[-2]
    n = shape_b[-2] if tb else shape_b[-1]
    lead = tuple(shape_a[:-2])
    C = {k: torch.empty(lead + (m, n), device=dev, dtype=dt) for k, dt in DT.items()}
    ent = {k: ours(a, b, C[k], ta, tb) for k, (a, b) in ops.items()}
    ta_bf, tb_bf = ops["bf16"]
    c_torch = torch.empty(lead + (m, n), device=dev, dtype=torch.bfloat16)
    ent["torch_bf16"] = lambda: torch.matmul(op(ta_bf, ta), op(tb_bf, tb), out=c_torch)
    t = time_interleaved(ent)
    ok = {k: check(ops[k][0], ops[k][1], C[k], ta, tb) for k in ("bf16", "fp16")}
    line = report(tag, t, flops, ok, t0)
    out.append(line)
    return all(ok.values())


def report(tag, t, flops, ok, t0):
    tf = {k: flops / v / 1e9 for k, v in t.items()}
    parts = [f"{tag:22s}",
             "ms: " + " ".join(f"{k} {v:.3f}" for k, v in t.items()),
             "TF: " + " ".join(f"{k} {v:.0f}" for k, v in tf.items()),
             f"ours-bf16/torch-bf16 {t['bf16'] / t['torch_bf16']:.2f} ours-fp16/torch-bf16 {t['fp16'] / t['torch_bf16']:.2f} "
             f"ours-bf16/ours-fp32 {t['bf16'] / t['fp32']:.2f}",
             "bound: " + (" ".join(f"{k} {'ok' if v else 'FAIL'}" for k, v in ok.items()) if ok else "-") +
             f" [{time.time() - t0:.0f} s]"]
    line = " | ".join(parts)
    print(line, flush=True)
    return line


def attention_tensors(dt, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    Bz, H, S, D = 32, 12, 512, 64
    q, k, v = (torch.rand(Bz, H, S, D, device=dev, generator=g).to(dt).requires_grad_(True) for _ in range(3))
    probs = torch.softmax(torch.rand(Bz, H, S, S, device=dev, generator=g), dim=-1).to(dt).requires_grad_(True)
    d_scores = torch.rand(Bz, H, S, S, device=dev, generator=g).to(dt)
    d_ctx = torch.rand(Bz, H, S, D, device=dev, generator=g).to(dt)
    return q, k, v, probs, d_scores, d_ctx


def attention_step(dt, torch_path=False):
    '''bench.py's C5 step in dtype dt: through our classes, or through torch.matmul.'''
    q, k, v, probs, d_scores, d_ctx = attention_tensors(dt)

    def step():
        for t in (q, k, v, probs):
            t.grad = None
        if torch_path:
            scores = torch.matmul(q, k.transpose(-1, -2))
        else:
            scores = matmuls.cublasTransbMM.apply(q, k)
        scores.backward(d_scores)
        ctx = torch.matmul(probs, v) if torch_path else matmuls.cublasMM.apply(probs, v)
        ctx.backward(d_ctx)
    return step


def attention(out):
    t0 = time.time()
    Bz, H, S, D = 32, 12, 512, 64
    ok = True
    # the two products on their own
    ok = product_shape("attn q.kT (NT)", (Bz, H, S, D), (Bz, H, S, D), False, True, 2.0 * Bz * H * S * S * D,
                       gen=lambda s, seed: torch.rand(s, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)),
                       out=out) and ok
    ok = product_shape("attn probs.V (NN)", (Bz, H, S, S), (Bz, H, S, D), False, False, 2.0 * Bz * H * S * S * D,
                       gen=lambda s, seed: torch.softmax(torch.rand(s, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)), -1)
                       if s[-1] == S else torch.rand(s, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)),
                       out=out) and ok
    # the whole forward + backward step
    ent = {"bf16": attention_step(torch.bfloat16), "fp16": attention_step(torch.float16),
           "fp32": attention_step(torch.float32), "torch_bf16": attention_step(torch.bfloat16, torch_path=True)}
    t = time_interleaved(ent, rounds=3)
    out.append(report("attn step fwd+bwd", t, 6 * 2.0 * Bz * H * S * S * D, {}, t0))
    return ok


def profile(name, steps=3):
    '''The bf16 attention step `steps` times: the program tools/kstats.sh profiles for the per-kernel table.'''
    assert name == "attn", name
    step = attention_step(torch.bfloat16)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print(f"bf16 attention step x {steps} done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default="")
    ap.add_argument("--profile", default="", help="only run the bf16 attention step 3 times (for kstats.sh)")
    a = ap.parse_args()
    if a.profile:
        profile(a.profile)
        return
    head = (f"# device {torch.cuda.get_device_name(0)}; interleaved medians, ms per call; TF = 2mnk / time; "
            f"ours = custom_mm (mi_gemm_bf16 / _f16 / the fp32 family), torch_bf16 = torch.matmul in bf16")
    print(head, flush=True)
    out, ok = [head], True
    shapes = {
        "sq": lambda: all([product_shape(f"{n}^3 {nm}", (n, n), (n, n), False, tb, 2.0 * n ** 3, out=out)
                           for n in (4096, 8192) for nm, tb in (("NN", False), ("NT", True))]),
        "attn": lambda: attention(out),
        "fc": lambda: all([product_shape("FC 16384x3072->768 NT", (16384, 3072), (768, 3072), False, True,
                                         2.0 * 16384 * 3072 * 768, out=out),
                           product_shape("FC dW TN k=16384", (16384, 768), (16384, 3072), True, False,
                                         2.0 * 16384 * 3072 * 768, out=out)]),
        "ragged": lambda: all([product_shape("197-tok probs.V (NN)", (384, 197, 197), (384, 197, 64), False, False,
                                             2.0 * 384 * 197 * 197 * 64, out=out),
                               product_shape("4095^3 NN", (4095, 4095), (4095, 4095), False, False, 2.0 * 4095 ** 3,
                                             out=out)]),
    }
    for tag, fn in shapes.items():
        if a.only and a.only != tag:
            continue
        ok = fn() and ok
        torch.cuda.empty_cache()
    if a.log:
        Path(a.log).parent.mkdir(parents=True, exist_ok=True)
        Path(a.log).write_text("\n".join(out) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
