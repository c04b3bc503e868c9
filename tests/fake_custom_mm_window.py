"""The stand-ins of the sixteen reading bindings plus their window forms — TEST ONLY.

Re-exports tests/fake_custom_mm_spec_decode.py (the eight decode bindings and their tree forms) and
tests/fake_custom_mm_block_attention_prefill_split.py (the four prefill bindings and their split forms) UNCHANGED — a call that
reaches one of them with another argument list than today's raises TypeError —, adds the four block_attention_lists_prefill…
bindings with today's argument lists (they record the call and store zero rows: no stand-in of them existed), and the sixteen
block_attention_window_… bindings with the real bindings' argument lists.  A window binding records (name, arguments, window,
sink) in `window_calls` with the operands as they arrive, then runs its parent without the two ints (the stand-in does not
apply the window).  A plain Python module."""
import torch

from fake_custom_mm_block_attention_prefill_split import *  # noqa: F401,F403
from fake_custom_mm_spec_decode import *  # noqa: F401,F403
from fake_custom_mm_spec_decode import calls, spec_calls  # noqa: F401

window_calls = []

DECODE = ("block_attention_decode", "block_attention_decode_paged", "block_attention_decode_fp8", "block_attention_decode_paged_fp8",
          "block_attention_decode_lists", "block_attention_decode_lists_paged", "block_attention_lists_decode_fp8",
          "block_attention_lists_decode_paged_fp8")
PREFILL = ("block_attention_prefill", "block_attention_prefill_paged", "block_attention_prefill_fp8", "block_attention_prefill_paged_fp8",
           "block_attention_lists_prefill", "block_attention_lists_prefill_paged", "block_attention_lists_prefill_fp8",
           "block_attention_lists_prefill_paged_fp8")


def window_name(parent):
    return "block_attention_window_" + parent[len("block_attention_"):]


def _lists_prefill(name, block_ids, block_counts, q, k, table, k_lens, new_lens, out, lse):
    B, Hq, T, D = q.shape
    X = -(-T // 64) + 1
    assert block_ids.dtype == torch.int32 and block_ids.is_contiguous() and tuple(block_ids.shape[:3]) == (B, k.shape[1], X)
    assert block_counts.dtype == torch.int32 and block_counts.is_contiguous() and tuple(block_counts.shape) == (B, k.shape[1], X)
    assert k_lens.dtype == torch.int32 and (new_lens is None or new_lens.dtype == torch.int32)
    assert table is None or table.dtype == torch.int32
    calls.append((name, {"ids_ptr": block_ids.data_ptr(), "counts_ptr": block_counts.data_ptr(), "q_ptr": q.data_ptr()}))
    out.zero_()
    lse.fill_(-float("inf"))
    return out


def block_attention_lists_prefill(block_ids, block_counts, q, k, v, k_lens, new_lens, scale, out, lse):
    return _lists_prefill("block_attention_lists_prefill", block_ids, block_counts, q, k, None, k_lens, new_lens, out, lse)


def block_attention_lists_prefill_paged(block_ids, block_counts, q, k_pages, v_pages, block_table, k_lens, new_lens, scale, out, lse):
    return _lists_prefill("block_attention_lists_prefill_paged", block_ids, block_counts, q, k_pages, block_table, k_lens, new_lens, out, lse)


def block_attention_lists_prefill_fp8(block_ids, block_counts, q, k, v, k_lens, new_lens, scale, k_scale, v_scale, out, lse):
    return _lists_prefill("block_attention_lists_prefill_fp8", block_ids, block_counts, q, k, None, k_lens, new_lens, out, lse)


def block_attention_lists_prefill_paged_fp8(block_ids, block_counts, q, k_pages, v_pages, block_table, k_lens, new_lens, scale, k_scale,
                                            v_scale, out, lse):
    return _lists_prefill("block_attention_lists_prefill_paged_fp8", block_ids, block_counts, q, k_pages, block_table, k_lens, new_lens,
                          out, lse)


def _window(parent, at):
    """The window form of `parent`: window and sink stand at args[at], args[at + 1] (at < 0), right before the parent's tail."""
    fn = globals()[parent]

    def binding(*args):
        window, sink = args[at], args[at + 1]
        assert type(window) is int and type(sink) is int and 1 <= window < 2 ** 31 and 0 <= sink < 2 ** 31
        window_calls.append((window_name(parent), {"args": args, "window": window, "sink": sink}))
        return fn(*args[:at], *args[at + 2:])
    binding.__name__ = window_name(parent)
    return binding


for _name in DECODE:   # (window, sink, chunk, out, lse)
    globals()[window_name(_name)] = _window(_name, -5)
for _name in PREFILL:  # (window, sink, out, lse)
    globals()[window_name(_name)] = _window(_name, -4)
