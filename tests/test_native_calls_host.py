"""The native calls of the 64-wide wrappers, argument by argument (tests/helpers/native_recorder.py): the six forward-side, five
backward-side and five edge-weight wrappers of ops.py run on CPU tensors against a recording stub, and what reaches each entry
point - the caller's pointers, NULL in the same places, scalars, flags, dims, pointer arrays, GpdeNodeAttr and GpdeWeConvDesc
contents, workspace size - and every refusal's type and message equal tests/golden/native_calls_w64.json: 144 forms (128 written
before the forward wrappers shared their body, 16 of the edge-weight wrappers before the backward wrappers shared theirs and every
call its epilogue), 57 of them refusals, 19 (wrapper, entry point) pairs.
Workspace-size queries are left out of the comparison: their number may change.  No GPU, no library."""
import json
import os

import pytest

from tests.helpers import native_recorder as nr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_calls_w64.json")
with open(GOLDEN) as _f:
    EXPECTED = json.load(_f)
FORMS = {f[0]: f for f in nr.forms()}


def test_the_file_holds_exactly_the_table_of_forms():
    assert sorted(EXPECTED) == sorted(FORMS)


def test_the_table_reaches_every_wrapper_and_entry_point():
    pairs = {(rec["wrapper"], c[0]) for rec in EXPECTED.values() for c in nr.operator_calls(rec)["calls"]}
    assert pairs == nr.PAIRS
    refused = {rec["wrapper"] for rec in EXPECTED.values() if "raises" in rec}
    assert refused == {w for w, _ in nr.PAIRS}                 # every wrapper has a recorded refusal
    for rec in EXPECTED.values():                              # a refusal comes before the library: no operator call was made
        if "raises" in rec:
            assert nr.operator_calls(rec)["calls"] == [], rec


@pytest.mark.parametrize("form", sorted(FORMS))
def test_native_calls_equal_the_record(form):
    got = json.loads(json.dumps(nr.record(FORMS[form])))      # (tuples -> lists, as the file has them)
    assert nr.operator_calls(got) == nr.operator_calls(EXPECTED[form])
