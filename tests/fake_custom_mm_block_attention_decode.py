"""fake_custom_mm_block_attention_gqa plus the decode entry — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention_gqa.py and adds a float64 numpy form of custom_mm.block_attention_decode
with the real entry's argument list (offsets, columns, nnz, q, k, v, k_lens, scale, chunk, out, lse): q and out [B, Hq, T, D]
contiguous, k and v [B, Hkv, Smax, D] AS THEY ARRIVE (the call is recorded with their data_ptr and strides, so a test sees
that the cache was not copied), k_lens contiguous int32 [B] or [1], clamped to [0, Smax] as the kernel clamps it.  Token t
of k / v item c = (b, h) stands at pos = k_len − T + t and sees key j iff j ≤ pos and the 64-block list of layout c mod L,
row pos // 64, holds j // 64; a token that sees nothing gives a zero row and lse −inf.  Keys a token does not see are
never touched (NaN there reaches nothing).  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_attention_gqa import *  # noqa: F401,F403
from fake_custom_mm_block_attention_gqa import TILE, calls  # noqa: F401


def block_attention_decode(offsets, columns, nnz, q, k, v, k_lens, scale, chunk, out, lse):
    calls.append(("block_attention_decode", {
        "q": tuple(q.shape), "k": tuple(k.shape), "layouts": offsets.shape[0], "nnz": nnz, "chunk": chunk, "scale": scale,
        "k_ptr": k.data_ptr(), "k_stride": tuple(k.stride()), "v_ptr": v.data_ptr(), "v_stride": tuple(v.stride()),
        "k_lens": k_lens.clone(), "offsets_ptr": offsets.data_ptr()}))
    assert offsets.dtype == torch.int32 and columns.dtype == torch.int32 and columns.numel() == nnz
    assert q.dim() == 4 and k.dim() == 4 and v.shape == k.shape and q.is_contiguous() and out.is_contiguous()
    B, Hq, T, D = q.shape
    Hkv, Smax = k.shape[1], k.shape[2]
    assert k.shape[0] == B and k.shape[3] == D and Hq % Hkv == 0 and Smax % TILE == 0
    G, blocks = Hq // Hkv, Smax // TILE
    assert 1 <= G <= 16 and isinstance(chunk, int) and chunk >= 1
    assert offsets.dim() == 2 and offsets.shape[1] == blocks + 1 and int(offsets[-1, -1]) == nnz
    assert k_lens.dtype == torch.int32 and k_lens.dim() == 1 and k_lens.is_contiguous() and k_lens.numel() in (1, B)
    assert out.shape == q.shape and lse.shape == (B, Hq, T) and lse.dtype == torch.float32
    for t in (k, v):
        assert t.stride(3) == 1 and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0
    off = offsets.numpy().astype(np.int64)
    col = columns.numpy().astype(np.int64)
    lens = np.clip(k_lens.numpy().astype(np.int64), 0, Smax)
    res, ls = np.zeros((B, Hq, T, D)), np.full((B, Hq, T), -np.inf)
    for b in range(B):
        for h in range(Hkv):
            c = b * Hkv + h
            o = off[c % off.shape[0]]
            for t in range(T):
                pos = int(lens[b if len(lens) > 1 else 0]) - T + t
                if pos < 0:
                    continue
                listed = col[o[pos // TILE]:o[pos // TILE + 1]]
                assert len(set(listed.tolist())) == len(listed), "a block stored twice"
                keys = np.array([j for J in listed if 0 <= J < blocks for j in range(J * TILE, (J + 1) * TILE) if j <= pos], np.int64)
                if len(keys) == 0:
                    continue
                kn, vn = k[b, h][keys].double().numpy(), v[b, h][keys].double().numpy()
                qn = q[b, h * G:(h + 1) * G, t].double().numpy()
                s = float(scale) * (qn @ kn.T)
                m = s.max(1, keepdims=True)
                e = np.exp(s - m)
                res[b, h * G:(h + 1) * G, t] = (e / e.sum(1, keepdims=True)) @ vn
                ls[b, h * G:(h + 1) * G, t] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
    out.copy_(torch.from_numpy(res).to(out.dtype))
    lse.copy_(torch.from_numpy(ls).to(lse.dtype))
    return out
