"""fake_custom_mm_block_attention_decode_paged plus the five entries of the query-aware selection — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention_decode_paged.py and adds float64 numpy forms of custom_mm.kv_block_bounds,
kv_block_bounds_paged, block_select, block_attention_decode_lists and block_attention_decode_lists_paged with the real
entries' argument lists.  Every call is recorded with the data_ptr, strides and dtype of the operands AS THEY ARRIVE, so a
test sees that the cache, the pool, q, the bounds and the lists were not copied.  Rows a rule does not see are never touched
(NaN there reaches nothing).  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_attention_decode_paged import *  # noqa: F401,F403
from fake_custom_mm_block_attention_decode_paged import TILE, calls  # noqa: F401


def _lens(k_lens, B, Smax):
    assert k_lens.dtype == torch.int32 and k_lens.dim() == 1 and k_lens.is_contiguous() and k_lens.numel() in (1, B)
    lens = np.clip(k_lens.numpy().astype(np.int64), 0, Smax)
    return [int(lens[b if len(lens) > 1 else 0]) for b in range(B)]


def _bounds(name, k, table, k_lens, last, bounds):
    calls.append((name, {"k_ptr": k.data_ptr(), "k_stride": tuple(k.stride()), "k_shape": tuple(k.shape), "last": last,
                         "bounds_ptr": bounds.data_ptr(), "k_lens": k_lens.clone(),
                         "table_ptr": None if table is None else table.data_ptr(),
                         "table_dtype": None if table is None else table.dtype,
                         "table_stride": None if table is None else tuple(table.stride())}))
    assert k.dim() == 4 and bounds.dim() == 5 and bounds.is_contiguous() and bounds.dtype == k.dtype
    assert k.stride(3) == 1 and all(s % 8 == 0 for s in k.stride()[:3]) and k.data_ptr() % 16 == 0
    assert isinstance(last, int) and last >= 0
    B, Hkv, blocks, two, D = bounds.shape
    page = k.shape[2] if table is not None else None
    Smax = k.shape[2] if table is None else table.shape[1] * page
    assert two == 2 and k.shape[1] == Hkv and k.shape[3] == D and blocks * TILE == Smax
    if table is not None:
        assert table.dtype == torch.int32 and tuple(table.shape[:1]) == (B,)
    for b, klen in enumerate(_lens(k_lens, B, Smax)):
        first = max(klen - last, 0) // TILE if last > 0 else 0
        for J in range(first, blocks):
            rows = [j for j in range(J * TILE, min(J * TILE + TILE, klen))]
            if table is not None:
                rows = [j for j in rows if 0 <= int(table[b, j // page]) < k.shape[0]]
            if not rows:
                continue
            for h in range(Hkv):
                seen = torch.stack([k[b, h, j] if table is None else k[int(table[b, j // page]), h, j % page] for j in rows])
                bounds[b, h, J, 0] = seen.double().amin(0).to(k.dtype)
                bounds[b, h, J, 1] = seen.double().amax(0).to(k.dtype)


def kv_block_bounds(k, k_lens, last, bounds):
    _bounds("kv_block_bounds", k, None, k_lens, last, bounds)


def kv_block_bounds_paged(k_pages, block_table, k_lens, last, bounds):
    _bounds("kv_block_bounds_paged", k_pages, block_table, k_lens, last, bounds)


def block_select(q, bounds, k_lens, K, sink, local, block_ids, block_counts, scores):
    calls.append(("block_select", {"q_ptr": q.data_ptr(), "q_stride": tuple(q.stride()), "bounds_ptr": bounds.data_ptr(), "K": K,
                                   "sink": sink, "local": local, "scores": scores is not None, "k_lens": k_lens.clone()}))
    assert q.dim() == 4 and bounds.dim() == 5 and bounds.is_contiguous() and bounds.dtype == q.dtype
    assert q.stride(3) == 1 and q.data_ptr() % 16 == 0
    B, Hq, T, D = q.shape
    Hkv, blocks = bounds.shape[1], bounds.shape[2]
    G = Hq // Hkv
    assert tuple(bounds.shape) == (B, Hkv, blocks, 2, D) and Hq == G * Hkv and 1 <= G <= 16
    assert all(isinstance(x, int) for x in (K, sink, local)) and K >= 1 and sink >= 0 and local >= 1 and sink + local <= K
    assert block_ids.dtype == torch.int32 and tuple(block_ids.shape) == (B, Hkv, T, K) and block_ids.is_contiguous()
    assert block_counts.dtype == torch.int32 and tuple(block_counts.shape) == (B, Hkv, T) and block_counts.is_contiguous()
    assert scores is None or (scores.dtype == torch.float32 and tuple(scores.shape) == (B, Hkv, T, blocks))
    block_ids.fill_(-1)
    block_counts.zero_()
    if scores is not None:
        scores.fill_(-np.inf)
    for b, klen in enumerate(_lens(k_lens, B, blocks * TILE)):
        for h in range(Hkv):
            for t in range(T):
                pos = klen - T + t
                if pos < 0:
                    continue
                n = min(pos // TILE + 1, blocks)
                lo, hi = (bounds[b, h, :n, i].double().numpy() for i in (0, 1))   # only the candidates are touched
                qn = q[b, h * G:(h + 1) * G, t].double().numpy()
                s = np.maximum(qn[:, None, :] * lo[None], qn[:, None, :] * hi[None]).sum(-1)   # [G, n]
                sc = np.fmax.reduce(s, axis=0) + 0.0
                forced = [J for J in range(n) if J < sink or J > n - 1 - local]
                rest = sorted((J for J in range(n) if J not in forced),
                              key=lambda J: (not np.isnan(sc[J]), sc[J] if not np.isnan(sc[J]) else 0.0, -J), reverse=True)
                count = min(K, n)
                chosen = sorted(forced + rest[:count - len(forced)])
                block_ids[b, h, t, :count] = torch.tensor(chosen, dtype=torch.int32)
                block_counts[b, h, t] = count
                if scores is not None:
                    scores[b, h, t, :n] = torch.from_numpy(sc).float()


def _lists(name, block_ids, block_counts, q, k, v, table, k_lens, scale, chunk, out, lse):
    calls.append((name, {"ids_ptr": block_ids.data_ptr(), "counts_ptr": block_counts.data_ptr(), "q": tuple(q.shape), "chunk": chunk,
                         "scale": scale, "k_ptr": k.data_ptr(), "k_stride": tuple(k.stride()), "v_ptr": v.data_ptr(),
                         "v_stride": tuple(v.stride()), "k_lens": k_lens.clone(),
                         "table_ptr": None if table is None else table.data_ptr(),
                         "table_dtype": None if table is None else table.dtype}))
    assert q.dim() == 4 and k.dim() == 4 and v.shape == k.shape and q.is_contiguous() and out.is_contiguous()
    B, Hq, T, D = q.shape
    Hkv = k.shape[1]
    page = k.shape[2] if table is not None else None
    Smax = k.shape[2] if table is None else table.shape[1] * page
    G, blocks = Hq // Hkv, Smax // TILE
    assert Smax % TILE == 0 and 1 <= G <= 16 and isinstance(chunk, int) and chunk >= 1
    assert block_ids.dtype == torch.int32 and block_ids.dim() == 4 and tuple(block_ids.shape[:3]) == (B, Hkv, T) and block_ids.is_contiguous()
    assert block_counts.dtype == torch.int32 and tuple(block_counts.shape) == (B, Hkv, T) and block_counts.is_contiguous()
    K = block_ids.shape[3]
    assert out.shape == q.shape and lse.shape == (B, Hq, T) and lse.dtype == torch.float32
    for x in (k, v):
        assert x.stride(3) == 1 and all(s % 8 == 0 for s in x.stride()[:3]) and x.data_ptr() % 16 == 0
    res, ls = np.zeros((B, Hq, T, D)), np.full((B, Hq, T), -np.inf)
    for b, klen in enumerate(_lens(k_lens, B, Smax)):
        for h in range(Hkv):
            for t in range(T):
                pos = klen - T + t
                if pos < 0:
                    continue
                listed = block_ids[b, h, t, :max(0, min(int(block_counts[b, h, t]), K))].tolist()
                keys = [j for J in listed if 0 <= J < blocks for j in range(J * TILE, (J + 1) * TILE) if j <= pos]  # twice: twice
                if table is not None:
                    entry = {lp: int(table[b, lp]) for lp in sorted({j // page for j in keys})}
                    keys = [j for j in keys if 0 <= entry[j // page] < k.shape[0]]
                if not keys:
                    continue
                row = (lambda x, j: x[b, h, j]) if table is None else (lambda x, j: x[entry[j // page], h, j % page])
                kn = np.stack([row(k, j).double().numpy() for j in keys])
                vn = np.stack([row(v, j).double().numpy() for j in keys])
                qn = q[b, h * G:(h + 1) * G, t].double().numpy()
                s = float(scale) * (qn @ kn.T)
                m = s.max(1, keepdims=True)
                e = np.exp(s - m)
                res[b, h * G:(h + 1) * G, t] = (e / e.sum(1, keepdims=True)) @ vn
                ls[b, h * G:(h + 1) * G, t] = (m + np.log(e.sum(1, keepdims=True)))[:, 0]
    out.copy_(torch.from_numpy(res).to(out.dtype))
    lse.copy_(torch.from_numpy(ls).to(lse.dtype))
    return out


def block_attention_decode_lists(block_ids, block_counts, q, k, v, k_lens, scale, chunk, out, lse):
    return _lists("block_attention_decode_lists", block_ids, block_counts, q, k, v, None, k_lens, scale, chunk, out, lse)


def block_attention_decode_lists_paged(block_ids, block_counts, q, k_pages, v_pages, block_table, k_lens, scale, chunk, out, lse):
    return _lists("block_attention_decode_lists_paged", block_ids, block_counts, q, k_pages, v_pages, block_table, k_lens, scale,
                  chunk, out, lse)
