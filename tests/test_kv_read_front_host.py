"""The Python front of the sixteen KV-cache reading calls keeps its recorded behaviour, without a GPU.

tests/golden/kv_read_front.json was written by tools/record_kv_read_front.py on the commit named in its "recorded_on" — the
front with one body per kind of call — over the corpus of tests/kv_read_front_cases.py.  The corpus is replayed on the code at
hand and compared with ==: for an accepted call the binding reached and every argument as it arrives (dtype, shape, strides,
whose memory it is, or type and value), through the stand-in tests/fake_custom_mm_window.py; for a refused one the exception's
type and its message, character for character, on the real extension — so also WHICH of two defects is reported, and the order
in which the device check names the operands.  The 44 binding names stand below as literal strings: the function that
spells them is pinned by something other than a recording of itself."""
import json
from pathlib import Path

import pytest

import kv_read_front_cases as cases

GOLDEN = Path(__file__).resolve().parent / "golden" / "kv_read_front.json"

# (call, form) → the binding: plain, then each optional piece the call takes
BINDINGS = {
    ("block_sparse_attention_decode", "plain"): "block_attention_decode",
    ("block_sparse_attention_decode", "tree"): "block_attention_tree_decode",
    ("block_sparse_attention_decode", "window"): "block_attention_window_decode",
    ("block_sparse_attention_decode_paged", "plain"): "block_attention_decode_paged",
    ("block_sparse_attention_decode_paged", "tree"): "block_attention_tree_decode_paged",
    ("block_sparse_attention_decode_paged", "window"): "block_attention_window_decode_paged",
    ("block_sparse_attention_decode_fp8", "plain"): "block_attention_decode_fp8",
    ("block_sparse_attention_decode_fp8", "tree"): "block_attention_tree_decode_fp8",
    ("block_sparse_attention_decode_fp8", "window"): "block_attention_window_decode_fp8",
    ("block_sparse_attention_decode_paged_fp8", "plain"): "block_attention_decode_paged_fp8",
    ("block_sparse_attention_decode_paged_fp8", "tree"): "block_attention_tree_decode_paged_fp8",
    ("block_sparse_attention_decode_paged_fp8", "window"): "block_attention_window_decode_paged_fp8",
    ("block_sparse_attention_decode_selected", "plain"): "block_attention_decode_lists",
    ("block_sparse_attention_decode_selected", "tree"): "block_attention_tree_decode_lists",
    ("block_sparse_attention_decode_selected", "window"): "block_attention_window_decode_lists",
    ("block_sparse_attention_decode_selected_paged", "plain"): "block_attention_decode_lists_paged",
    ("block_sparse_attention_decode_selected_paged", "tree"): "block_attention_tree_decode_lists_paged",
    ("block_sparse_attention_decode_selected_paged", "window"): "block_attention_window_decode_lists_paged",
    ("block_sparse_attention_decode_selected_fp8", "plain"): "block_attention_lists_decode_fp8",
    ("block_sparse_attention_decode_selected_fp8", "tree"): "block_attention_tree_lists_decode_fp8",
    ("block_sparse_attention_decode_selected_fp8", "window"): "block_attention_window_lists_decode_fp8",
    ("block_sparse_attention_decode_selected_paged_fp8", "plain"): "block_attention_lists_decode_paged_fp8",
    ("block_sparse_attention_decode_selected_paged_fp8", "tree"): "block_attention_tree_lists_decode_paged_fp8",
    ("block_sparse_attention_decode_selected_paged_fp8", "window"): "block_attention_window_lists_decode_paged_fp8",
    ("block_sparse_attention_prefill", "plain"): "block_attention_prefill",
    ("block_sparse_attention_prefill", "split"): "block_attention_prefill_split",
    ("block_sparse_attention_prefill", "window"): "block_attention_window_prefill",
    ("block_sparse_attention_prefill_paged", "plain"): "block_attention_prefill_paged",
    ("block_sparse_attention_prefill_paged", "split"): "block_attention_prefill_split_paged",
    ("block_sparse_attention_prefill_paged", "window"): "block_attention_window_prefill_paged",
    ("block_sparse_attention_prefill_fp8", "plain"): "block_attention_prefill_fp8",
    ("block_sparse_attention_prefill_fp8", "split"): "block_attention_prefill_split_fp8",
    ("block_sparse_attention_prefill_fp8", "window"): "block_attention_window_prefill_fp8",
    ("block_sparse_attention_prefill_paged_fp8", "plain"): "block_attention_prefill_paged_fp8",
    ("block_sparse_attention_prefill_paged_fp8", "split"): "block_attention_prefill_split_paged_fp8",
    ("block_sparse_attention_prefill_paged_fp8", "window"): "block_attention_window_prefill_paged_fp8",
    ("block_sparse_attention_prefill_selected", "plain"): "block_attention_lists_prefill",
    ("block_sparse_attention_prefill_selected", "window"): "block_attention_window_lists_prefill",
    ("block_sparse_attention_prefill_selected_paged", "plain"): "block_attention_lists_prefill_paged",
    ("block_sparse_attention_prefill_selected_paged", "window"): "block_attention_window_lists_prefill_paged",
    ("block_sparse_attention_prefill_selected_fp8", "plain"): "block_attention_lists_prefill_fp8",
    ("block_sparse_attention_prefill_selected_fp8", "window"): "block_attention_window_lists_prefill_fp8",
    ("block_sparse_attention_prefill_selected_paged_fp8", "plain"): "block_attention_lists_prefill_paged_fp8",
    ("block_sparse_attention_prefill_selected_paged_fp8", "window"): "block_attention_window_lists_prefill_paged_fp8",
}
CALL_NAMES = [call.name for call in cases.CALLS]


@pytest.fixture(scope="module")
def recorded():
    packed = json.loads(GOLDEN.read_text())
    return {half: cases.unpack(packed[half], packed["strings"]) for half in ("accepted", "refused")}


@pytest.fixture(scope="module")
def replayed(built, oracle_mod):
    """The whole corpus once, on the code at hand."""
    accepted, refused = cases.replay()
    return {"accepted": accepted, "refused": refused}


def test_the_corpus_is_the_recorded_one_and_every_refusal_was_one(recorded):
    assert len(CALL_NAMES) == 16 and len(BINDINGS) == 44
    assert {(c.name, m) for c in cases.CALLS for m in cases.modifiers(c)} == set(BINDINGS)
    accepted = {}
    for call, form, _ in cases.accepted_cases():
        accepted.setdefault(call.name, []).append(form)
    refused = {}
    for call, case, _ in cases.refused_cases():
        refused.setdefault(call.name, []).append(case)
    assert {c: sorted(v) for c, v in accepted.items()} == {c: sorted(v) for c, v in recorded["accepted"].items()}
    assert {c: sorted(v) for c, v in refused.items()} == {c: sorted(v) for c, v in recorded["refused"].items()}
    for name in CALL_NAMES:
        assert len(accepted[name]) == 2 * len(cases.modifiers(cases.CALLS[CALL_NAMES.index(name)])) + 1
        assert all(kind in ("ValueError", "RuntimeError") for kind, _, _ in recorded["refused"][name].values()), name
        assert recorded["refused"][name]["valid"][0] == "RuntimeError" and "must be device (HIP) tensors" in recorded["refused"][name]["valid"][2]
    for kind in cases.PAIRS:  # at least ten pairs of defects per kind that every call of the kind takes
        for call in cases.CALLS:
            if cases.kind(call) == kind:
                assert sum(" + " in case for case in refused[call.name]) >= 10, call.name


@pytest.mark.parametrize("name", CALL_NAMES)
def test_accepted_calls_reach_the_recorded_binding_with_the_recorded_arguments(recorded, replayed, name):
    call = cases.CALLS[CALL_NAMES.index(name)]
    got, want = replayed["accepted"][name], recorded["accepted"][name]
    for form in want:
        assert got[form] == want[form], (name, form)
    assert list(got) == list(want)
    for modifier in cases.modifiers(call):  # the names, from the table above
        for lse in (False, True):
            reached = [b[0] for b in got[f"{modifier}, return_lse={lse}"]["bindings"]]
            assert reached == [BINDINGS[name, modifier]], (name, modifier, lse)
    assert got["empty batch"]["bindings"] == []  # out.numel() == 0: no binding call


@pytest.mark.parametrize("name", CALL_NAMES)
def test_refused_calls_raise_the_recorded_exception_with_the_recorded_message(recorded, replayed, name):
    got, want = replayed["refused"][name], recorded["refused"][name]
    for case in want:
        assert got[case] == want[case], (name, case)
    assert list(got) == list(want)
