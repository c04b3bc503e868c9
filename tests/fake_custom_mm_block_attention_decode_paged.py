"""fake_custom_mm_block_attention_decode plus the paged decode entry — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention_decode.py and adds a float64 numpy form of
custom_mm.block_attention_decode_paged with the real entry's argument list (offsets, columns, nnz, q, k_pages, v_pages,
block_table, k_lens, scale, chunk, out, lse): q and out [B, Hq, T, D] contiguous, the pool [P, Hkv, page, D] and the int32
table [B, W] AS THEY ARRIVE (the call is recorded with their data_ptr, strides and dtype, so a test sees that neither was
copied and that an int64 table was narrowed), Smax = W · page.  Key j of item (b, h) is row j % page of head h of pool page
block_table[b, j // page]; a key whose entry lies outside [0, P) is invisible, and so is every key the contiguous stand-in
would not see.  The entries of pages no token sees are never consulted and the pool rows of unseen keys never touched (NaN
and out-of-range values there reach nothing).  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_attention_decode import *  # noqa: F401,F403
from fake_custom_mm_block_attention_decode import TILE, calls  # noqa: F401


def block_attention_decode_paged(offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, scale, chunk, out, lse):
    calls.append(("block_attention_decode_paged", {
        "q": tuple(q.shape), "pool": tuple(k_pages.shape), "layouts": offsets.shape[0], "nnz": nnz, "chunk": chunk, "scale": scale,
        "k_ptr": k_pages.data_ptr(), "k_stride": tuple(k_pages.stride()), "v_ptr": v_pages.data_ptr(),
        "v_stride": tuple(v_pages.stride()), "table_ptr": block_table.data_ptr(), "table_stride": tuple(block_table.stride()),
        "table_dtype": block_table.dtype, "table_shape": tuple(block_table.shape), "k_lens": k_lens.clone(),
        "offsets_ptr": offsets.data_ptr()}))
    assert offsets.dtype == torch.int32 and columns.dtype == torch.int32 and columns.numel() == nnz
    assert q.dim() == 4 and k_pages.dim() == 4 and v_pages.shape == k_pages.shape and q.is_contiguous() and out.is_contiguous()
    B, Hq, T, D = q.shape
    P, Hkv, page = k_pages.shape[:3]
    assert k_pages.shape[3] == D and Hq % Hkv == 0 and page >= 16 and page & (page - 1) == 0
    assert block_table.dtype == torch.int32 and block_table.dim() == 2 and block_table.shape[0] == B
    W = block_table.shape[1]
    assert (W <= 1 or block_table.stride(1) == 1) and (B <= 1 or block_table.stride(0) >= W)
    Smax = W * page
    assert Smax % TILE == 0
    G, blocks = Hq // Hkv, Smax // TILE
    assert 1 <= G <= 16 and isinstance(chunk, int) and chunk >= 1
    assert offsets.dim() == 2 and offsets.shape[1] == blocks + 1 and int(offsets[-1, -1]) == nnz
    assert k_lens.dtype == torch.int32 and k_lens.dim() == 1 and k_lens.is_contiguous() and k_lens.numel() in (1, B)
    assert out.shape == q.shape and lse.shape == (B, Hq, T) and lse.dtype == torch.float32
    for t in (k_pages, v_pages):
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
                keys = [j for J in listed if 0 <= J < blocks for j in range(J * TILE, (J + 1) * TILE) if j <= pos]
                entry = {lp: int(block_table[b, lp]) for lp in sorted({j // page for j in keys})}  # only these are consulted
                keys = [j for j in keys if 0 <= entry[j // page] < P]
                if len(keys) == 0:
                    continue
                kn = np.stack([k_pages[entry[j // page], h, j % page].double().numpy() for j in keys])
                vn = np.stack([v_pages[entry[j // page], h, j % page].double().numpy() for j in keys])
                qn = q[b, h * G:(h + 1) * G, t].double().numpy()
                s = float(scale) * (qn @ kn.T)
                m = s.max(1, keepdims=True)
                e = np.exp(s - m)
                res[b, h * G:(h + 1) * G, t] = (e / e.sum(1, keepdims=True)) @ vn
                ls[b, h * G:(h + 1) * G, t] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
    out.copy_(torch.from_numpy(res).to(out.dtype))
    lse.copy_(torch.from_numpy(ls).to(lse.dtype))
    return out
