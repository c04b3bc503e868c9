"""The yardstick of rope_kv_cache_append — TEST ONLY, torch on the CPU, nothing of the kernel.

The rotation is the plain torch expression the contract names: (a.float() * c − b.float() * s).to(dtype) — on the CPU torch
computes each product and the sum as a float32 operation of its own (no fma), keeps float32 subnormals and narrows with one
round-to-nearest-even.  Everything works on RAW int16 bits so that NaN payloads and −0 survive the copies.
"""
import torch


def rotate(x16, dtype, c, s, R, interleaved):
    """x16 [..., D] int16 bits of `dtype`; c, s float32, broadcastable to [..., R/2].  Returns int16 bits: the first R elements
    rotated, the tail d ≥ R a bit copy."""
    out = x16.clone()
    x = x16.view(dtype)
    if interleaved:
        a, b = x[..., 0:R:2].float(), x[..., 1:R:2].float()
    else:
        a, b = x[..., :R // 2].float(), x[..., R // 2:R].float()
    ra = (a * c - b * s).to(dtype).view(torch.int16)
    rb = (b * c + a * s).to(dtype).view(torch.int16)
    if interleaved:
        out[..., 0:R:2], out[..., 1:R:2] = ra, rb
    else:
        out[..., :R // 2], out[..., R // 2:R] = ra, rb
    return out


def token_slots(B, T, k_lens, pmax, new_lens=None):
    """(pos [B, T] int64, token [B, T] bool): pos = k_lens[b] − T + t; a slot holds a token iff t ≥ T − clamp(new_lens[b], 0, T)
    and 0 ≤ pos < pmax."""
    lens = torch.as_tensor([k_lens] * B if isinstance(k_lens, int) else list(k_lens), dtype=torch.int64)
    t = torch.arange(T, dtype=torch.int64)
    pos = lens[:, None] - T + t[None, :]
    n = torch.full((B,), T, dtype=torch.int64) if new_lens is None else torch.as_tensor(list(new_lens), dtype=torch.int64).clamp(0, T)
    token = (t[None, :] >= T - n[:, None]) & (pos >= 0) & (pos < pmax)
    return pos, token


def rotated(x16, dtype, cos, sin, pos, token, R, interleaved):
    """x16 [B, H, T, D] int16 bits rotated by table rows pos [B, T]; the rows of slots without a token are zeros."""
    safe = pos.clamp(0, max(cos.shape[0] - 1, 0))
    if cos.shape[0] == 0:
        return torch.zeros_like(x16)
    c, s = cos[safe][:, None, :, :R // 2], sin[safe][:, None, :, :R // 2]       # [B, 1, T, R/2]
    out = rotate(x16, dtype, c, s, R, interleaved)
    out[~token[:, None, :].expand(x16.shape[:3])] = 0
    return out


def place_tokens(place, cache, rows, k_lens, token, table=None):
    """`place` — the append's rule from tests/test_gpu_kv_cache_append.py — for the slots that hold a token: per item its
    tokens are one run [lo, hi) of the T slots, placed as that many new tokens of a length k_lens[b] − (T − hi).  Returns the
    number of (item, token) pairs written."""
    B, _, T, _ = rows.shape
    lens = [k_lens] * B if isinstance(k_lens, int) else list(k_lens)
    written = 0
    for b in range(B):
        slots = torch.nonzero(token[b]).reshape(-1).tolist()
        if not slots:
            continue
        lo, hi = slots[0], slots[-1] + 1
        assert slots == list(range(lo, hi))
        target = cache if table is not None else cache[b:b + 1]
        written += place(target, rows[b:b + 1, :, lo:hi], [int(lens[b]) - (T - hi)], None if table is None else table[b:b + 1])
    return written
