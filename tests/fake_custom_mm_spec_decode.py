"""The stand-ins of the decode, selection and rope families plus the bindings of the speculative step — TEST ONLY.

Re-exports tests/fake_custom_mm_block_select_fp8.py (the eight decode bindings) and tests/fake_custom_mm_rope_kv_append.py (the
appends) UNCHANGED — a call that reaches one of them with another argument list than today's raises TypeError — and adds the
eight block_attention_tree_… bindings, rope_kv_append{,_paged}_pos and kv_compact{,_paged} with the real bindings' argument lists.  Every new
binding records (name, arguments) in `spec_calls` with the operands as they arrive; a tree binding then runs its parent (the
causal result: the stand-in does not apply the mask), a *_pos binding its parent, kv_compact the rule on host tensors.
A plain Python module."""
import torch

from fake_custom_mm_block_select_fp8 import *  # noqa: F401,F403
from fake_custom_mm_rope_kv_append import *  # noqa: F401,F403
import fake_custom_mm_block_select_fp8 as _decode
import fake_custom_mm_rope_kv_append as _rope

spec_calls = []


def tree_name(parent):
    return "block_attention_tree_" + parent[len("block_attention_"):]


def _tree(parent, mask_at):
    def binding(*args):
        mask = args[mask_at]
        assert isinstance(mask, torch.Tensor) and mask.dtype == torch.int64 and mask.is_contiguous()
        spec_calls.append((tree_name(parent), {"args": args, "mask_ptr": mask.data_ptr(), "mask_shape": tuple(mask.shape)}))
        return getattr(_decode, parent)(*args[:mask_at], *args[mask_at + 1:])
    binding.__name__ = tree_name(parent)
    return binding


# (the mask stands right before chunk, out, lse)
for _name in ("block_attention_decode", "block_attention_decode_paged", "block_attention_decode_fp8", "block_attention_decode_paged_fp8",
              "block_attention_decode_lists", "block_attention_decode_lists_paged", "block_attention_lists_decode_fp8",
              "block_attention_lists_decode_paged_fp8"):
    globals()[tree_name(_name)] = _tree(_name, -4)


def rope_kv_append_pos(*args):
    assert len(args) == 16 and args[-1].dtype == torch.int32 and args[-1].is_contiguous() and args[-1].dim() == 2
    spec_calls.append(("rope_kv_append_pos", {"args": args, "positions_ptr": args[-1].data_ptr()}))
    return _rope.rope_kv_append(*args[:-1])


def rope_kv_append_paged_pos(*args):
    assert len(args) == 17 and args[-1].dtype == torch.int32 and args[-1].is_contiguous() and args[-1].dim() == 2
    spec_calls.append(("rope_kv_append_paged_pos", {"args": args, "positions_ptr": args[-1].data_ptr()}))
    return _rope.rope_kv_append_paged(*args[:-1])


def _compact(name, k, v, table, k_lens, accept, counts, T):
    assert k_lens.dtype == torch.int32 and accept.dtype == torch.int32 and counts.dtype == torch.int32
    assert accept.is_contiguous() and counts.is_contiguous() and accept.shape[1] == T
    spec_calls.append((name, {"k_ptr": k.data_ptr(), "k_stride": tuple(k.stride()), "v_ptr": v.data_ptr(), "accept_ptr": accept.data_ptr(),
                              "counts_ptr": counts.data_ptr(), "k_lens": k_lens.clone(), "T": T}))
    page = k.shape[2]
    smax = page * table.shape[1] if table is not None else k.shape[2]
    for x in (k, v):
        old = x.clone()
        for b in range(accept.shape[0]):
            base = int(k_lens[b if k_lens.numel() > 1 else 0]) - T
            for i in range(max(0, min(int(counts[b]), T))):
                off = int(accept[b, i])
                src, dst = base + off, base + i
                if not (0 <= off < T and 0 <= src < smax and 0 <= dst < smax):
                    continue
                if table is None:
                    x[b, :, dst] = old[b, :, src]
                    continue
                es, ed = int(table[b, src // page]), int(table[b, dst // page])
                if 0 <= es < x.shape[0] and 0 <= ed < x.shape[0]:
                    x[ed, :, dst % page] = old[es, :, src % page]


def kv_compact(k, v, k_lens, accept, accept_counts, T):
    _compact("kv_compact", k, v, None, k_lens, accept, accept_counts, T)


def kv_compact_paged(k_pages, v_pages, block_table, k_lens, accept, accept_counts, T):
    assert block_table.dtype == torch.int32
    _compact("kv_compact_paged", k_pages, v_pages, block_table, k_lens, accept, accept_counts, T)
