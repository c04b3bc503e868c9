"""fake_custom_mm_block_select plus the tile-level selection of chunked prefill — TEST ONLY.

Re-exports tests/fake_custom_mm_block_select.py and adds a float64 numpy form of custom_mm.block_select_tiles with the real
entry's argument list.  Every call is recorded with the data_ptr, strides and dtype of the operands AS THEY ARRIVE, so a test
sees that q, the bounds and new_lens were not copied.  Bounds of non-candidates and q of slots without a token are never
touched (NaN there reaches nothing).  A plain Python module: matmuls takes it for the stand-in it is.
"""
import numpy as np
import torch

from fake_custom_mm_block_select import *  # noqa: F401,F403
from fake_custom_mm_block_select import TILE, _lens, calls  # noqa: F401


def block_select_tiles(q, bounds, k_lens, new_lens, K, sink, local, block_ids, block_counts, scores):
    calls.append(("block_select_tiles", {"q_ptr": q.data_ptr(), "q_stride": tuple(q.stride()), "bounds_ptr": bounds.data_ptr(), "K": K,
                                         "sink": sink, "local": local, "scores": scores is not None, "k_lens": k_lens.clone(),
                                         "new_lens": None if new_lens is None else new_lens.clone(),
                                         "new_lens_dtype": None if new_lens is None else new_lens.dtype}))
    assert q.dim() == 4 and bounds.dim() == 5 and bounds.is_contiguous() and bounds.dtype == q.dtype
    assert q.stride(3) == 1 and q.data_ptr() % 16 == 0
    B, Hq, T, D = q.shape
    Hkv, blocks = bounds.shape[1], bounds.shape[2]
    G, X = Hq // Hkv, -(-T // TILE) + 1
    assert tuple(bounds.shape) == (B, Hkv, blocks, 2, D) and Hq == G * Hkv and 1 <= G <= 16
    assert all(isinstance(x, int) for x in (K, sink, local)) and K >= 1 and sink >= 0 and local >= 1 and sink + local <= K
    assert new_lens is None or (new_lens.dtype == torch.int32 and new_lens.is_contiguous() and new_lens.numel() in (1, B))
    assert block_ids.dtype == torch.int32 and tuple(block_ids.shape) == (B, Hkv, X, K) and block_ids.is_contiguous()
    assert block_counts.dtype == torch.int32 and tuple(block_counts.shape) == (B, Hkv, X) and block_counts.is_contiguous()
    assert scores is None or (scores.dtype == torch.float32 and tuple(scores.shape) == (B, Hkv, X, blocks))
    block_ids.fill_(-1)
    block_counts.zero_()
    if scores is not None:
        scores.fill_(-np.inf)
    for b, klen in enumerate(_lens(k_lens, B, blocks * TILE)):
        new = T if new_lens is None else min(max(int(new_lens[b if new_lens.numel() > 1 else 0]), 0), T)
        start, first = klen - T, max(klen - new, 0)
        for x in range(X):
            r = start // TILE + x
            slots = [p - start for p in range(max(first, r * TILE), min(klen, r * TILE + TILE))]
            if not slots:
                continue
            n = min(r + 1, blocks)
            for h in range(Hkv):
                lo, hi = (bounds[b, h, :n, i].double().numpy() for i in (0, 1))   # only the candidates are touched
                qn = q[b, h * G:(h + 1) * G][:, slots].double().numpy().reshape(-1, D)   # only the slots that hold a token
                s = np.minimum(qn, 0) @ lo.T + np.maximum(qn, 0) @ hi.T           # [G · tokens, n]
                sc = np.fmax.reduce(s, axis=0) + 0.0
                forced = [J for J in range(n) if J < sink or J > n - 1 - local]
                rest = sorted((J for J in range(n) if J not in forced),
                              key=lambda J: (not np.isnan(sc[J]), sc[J] if not np.isnan(sc[J]) else 0.0, -J), reverse=True)
                count = min(K, n)
                chosen = sorted(forced + rest[:count - len(forced)])
                block_ids[b, h, x, :count] = torch.tensor(chosen, dtype=torch.int32)
                block_counts[b, h, x] = count
                if scores is not None:
                    scores[b, h, x, :n] = torch.from_numpy(sc).float()
