"""fake_custom_mm_block_attention_decode_fp8 plus the four prefill entries — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention_decode_fp8.py and adds float64 numpy forms of
custom_mm.block_attention_prefill (offsets, columns, nnz, q, k, v, k_lens, new_lens, scale, out, lse), …_paged (… k_pages,
v_pages, block_table, k_lens, new_lens, scale, out, lse), …_fp8 (… k_lens, new_lens, scale, k_scale, v_scale, out, lse) and
…_paged_fp8 with the real entries' argument lists.  q, the cache and the table ARRIVE AS THEY ARE: every call is recorded with
their data_ptr, strides and dtypes, so a test sees that nothing was copied.  k_lens is a contiguous int32 [B] or [1], clamped
to [0, Smax] as the kernel clamps it; new_lens None or a contiguous int32 [B], clamped to [0, T].  Token t of k / v item
c = (b, h) stands at pos = k_len − T + t; slot t holds a token iff t ≥ T − new_len and pos ≥ 0; a token sees key j iff j ≤ pos,
the 64-block list of layout c mod L, row pos // 64, holds j // 64 and (paged) the table entry of j's page lies in [0, P).  A
slot without a token, or a token that sees nothing, gives a zero row and lse −inf.  Keys a token does not see are never
touched (NaN there reaches nothing).  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_attention_decode_fp8 import *  # noqa: F401,F403
from fake_custom_mm_block_attention_decode_fp8 import TILE, _dequantised, _scale_record, calls  # noqa: F401


def _prefill(name, offsets, columns, nnz, q, k, v, table, k_lens, new_lens, scale, k_scale, v_scale, out, lse):
    fp8 = k.dtype == torch.float8_e4m3fn
    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    rec = {"q": tuple(q.shape), "q_ptr": q.data_ptr(), "q_stride": tuple(q.stride()), "k": tuple(k.shape), "k_ptr": k.data_ptr(),
           "k_stride": tuple(k.stride()), "k_dtype": k.dtype, "v_ptr": v.data_ptr(), "v_stride": tuple(v.stride()),
           "layouts": offsets.shape[0], "nnz": nnz, "scale": scale, "k_lens": k_lens.clone(),
           "new_lens": None if new_lens is None else new_lens.clone(), "offsets_ptr": offsets.data_ptr(),
           "k_scale": _scale_record(k_scale, Hkv), "v_scale": _scale_record(v_scale, Hkv)}
    if table is not None:
        rec.update(table_ptr=table.data_ptr(), table_stride=tuple(table.stride()), table_dtype=table.dtype)
    calls.append((name, rec))
    assert offsets.dtype == torch.int32 and columns.dtype == torch.int32 and columns.numel() == nnz
    assert q.dim() == 4 and k.dim() == 4 and v.shape == k.shape and out.is_contiguous() and out.shape == q.shape
    assert q.stride(3) == 1 and all(s % 8 == 0 and s >= 0 for n, s in zip(q.shape[:3], q.stride()[:3]) if n > 1) and q.data_ptr() % 16 == 0
    unit = 16 if fp8 else 8
    for t in (k, v):
        assert t.stride(3) == 1 and all(s % unit == 0 for n, s in zip(t.shape[:3], t.stride()[:3]) if n > 1) and t.data_ptr() % 16 == 0
    if table is None:
        Smax, page, P = k.shape[2], k.shape[2], None
        assert k.shape[0] == B
    else:
        page, P = k.shape[2], k.shape[0]
        assert table.dtype == torch.int32 and table.dim() == 2 and table.shape[0] == B and page >= 16 and page & (page - 1) == 0
        Smax = table.shape[1] * page
    assert k.shape[3] == D and Hkv >= 1 and Hq % Hkv == 0 and Smax % TILE == 0 and T >= 1
    G, blocks = Hq // Hkv, Smax // TILE
    assert offsets.dim() == 2 and offsets.shape[1] == blocks + 1 and int(offsets[-1, -1]) == nnz
    assert k_lens.dtype == torch.int32 and k_lens.dim() == 1 and k_lens.is_contiguous() and k_lens.numel() in (1, B)
    assert new_lens is None or (new_lens.dtype == torch.int32 and new_lens.is_contiguous() and tuple(new_lens.shape) == (B,))
    assert lse.shape == (B, Hq, T) and lse.dtype == torch.float32
    kd = _dequantised(k, k_scale, Hkv) if fp8 else k.double()
    vd = _dequantised(v, v_scale, Hkv) if fp8 else v.double()
    off = offsets.numpy().astype(np.int64)
    col = columns.numpy().astype(np.int64)
    lens = np.clip(k_lens.numpy().astype(np.int64), 0, Smax)
    news = np.full(B, T) if new_lens is None else np.clip(new_lens.numpy().astype(np.int64), 0, T)
    res, ls = np.zeros((B, Hq, T, D)), np.full((B, Hq, T), -np.inf)
    for b in range(B):
        klen = int(lens[b if len(lens) > 1 else 0])
        for h in range(Hkv):
            o = off[(b * Hkv + h) % off.shape[0]]
            for t in range(T - int(news[b]), T):
                pos = klen - T + t
                if pos < 0:
                    continue
                listed = col[o[pos // TILE]:o[pos // TILE + 1]]
                assert len(set(listed.tolist())) == len(listed), "a block stored twice"
                keys = [j for J in listed if 0 <= J < blocks for j in range(J * TILE, (J + 1) * TILE) if j <= pos]
                if table is not None:
                    keys = [j for j in keys if 0 <= int(table[b, j // page]) < P]
                if not keys:
                    continue
                if table is None:
                    kn, vn = kd[b, h][keys].numpy(), vd[b, h][keys].numpy()
                else:
                    pg = [int(table[b, j // page]) for j in keys]
                    rw = [j % page for j in keys]
                    kn, vn = kd[pg, h, rw].numpy(), vd[pg, h, rw].numpy()
                qn = q[b, h * G:(h + 1) * G, t].double().numpy()
                s = float(scale) * (qn @ kn.T)
                m = s.max(1, keepdims=True)
                e = np.exp(s - m)
                res[b, h * G:(h + 1) * G, t] = (e / e.sum(1, keepdims=True)) @ vn
                ls[b, h * G:(h + 1) * G, t] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
    out.copy_(torch.from_numpy(res).to(out.dtype))
    lse.copy_(torch.from_numpy(ls).to(lse.dtype))
    return out


def block_attention_prefill(offsets, columns, nnz, q, k, v, k_lens, new_lens, scale, out, lse):
    return _prefill("block_attention_prefill", offsets, columns, nnz, q, k, v, None, k_lens, new_lens, scale, None, None, out, lse)


def block_attention_prefill_paged(offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, new_lens, scale, out, lse):
    return _prefill("block_attention_prefill_paged", offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, new_lens, scale,
                    None, None, out, lse)


def block_attention_prefill_fp8(offsets, columns, nnz, q, k, v, k_lens, new_lens, scale, k_scale, v_scale, out, lse):
    return _prefill("block_attention_prefill_fp8", offsets, columns, nnz, q, k, v, None, k_lens, new_lens, scale, k_scale, v_scale,
                    out, lse)


def block_attention_prefill_paged_fp8(offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, new_lens, scale, k_scale,
                                      v_scale, out, lse):
    return _prefill("block_attention_prefill_paged_fp8", offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, new_lens,
                    scale, k_scale, v_scale, out, lse)
