"""fake_custom_mm_block_attention_prefill plus the four split prefill bindings — TEST ONLY.

Re-exports tests/fake_custom_mm_block_attention_prefill.py and adds float64 numpy forms of
custom_mm.block_attention_prefill_split, …_split_paged, …_split_fp8 and …_split_paged_fp8: the unsplit bindings' argument
lists with `split` behind them.  What a split call computes is what the unsplit call computes — the cut
changes the order of summation, not the rule —, so the arithmetic is the unsplit stand-in's; the call is recorded under the
split binding's name with the unsplit record (data_ptr, strides, dtypes of q, the cache and the table: nothing was copied) and
`split` as the binding received it.  A plain Python module: matmuls takes it for the stand-in it is.
"""
from fake_custom_mm_block_attention_prefill import *  # noqa: F401,F403
from fake_custom_mm_block_attention_prefill import _prefill, calls  # noqa: F401


def _split(name, split, *args):
    assert isinstance(split, int) and not isinstance(split, bool) and 1 <= split < 2 ** 31, split
    out = _prefill(name, *args)
    calls[-1][1]["split"] = split
    return out


def block_attention_prefill_split(offsets, columns, nnz, q, k, v, k_lens, new_lens, scale, out, lse, split):
    return _split("block_attention_prefill_split", split, offsets, columns, nnz, q, k, v, None, k_lens, new_lens, scale, None, None,
                  out, lse)


def block_attention_prefill_split_paged(offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, new_lens, scale, out, lse, split):
    return _split("block_attention_prefill_split_paged", split, offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, new_lens,
                  scale, None, None, out, lse)


def block_attention_prefill_split_fp8(offsets, columns, nnz, q, k, v, k_lens, new_lens, scale, k_scale, v_scale, out, lse, split):
    return _split("block_attention_prefill_split_fp8", split, offsets, columns, nnz, q, k, v, None, k_lens, new_lens, scale, k_scale,
                  v_scale, out, lse)


def block_attention_prefill_split_paged_fp8(offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens, new_lens, scale, k_scale,
                                            v_scale, out, lse, split):
    return _split("block_attention_prefill_split_paged_fp8", split, offsets, columns, nnz, q, k_pages, v_pages, block_table, k_lens,
                  new_lens, scale, k_scale, v_scale, out, lse)
