"""Host tier of the stream contract (DESIGN.md "Streams"): the cross-stream helper of ops.py on stand-in streams, and the
completeness of the side-stream table of tests/test_gpu_streams.py.  No GPU."""
import inspect
import re
import sys

import pytest
import torch

import graph_pde_amd  # noqa: F401
from graph_pde_amd import hidden_cache, ops
from tests.helpers.streams import EXCLUDED, SIDE_STREAM_TABLE


class _Stream:
    def __init__(self, name):
        self.name = name


class _Event:
    def record(self, stream):
        self.stream = stream


@pytest.fixture
def seams(monkeypatch):
    """ops' stream seams on stand-ins: `now` is the current stream; every wait and every record_stream is logged."""
    state = {"now": _Stream("A"), "capturing": False, "waits": [], "kept": []}
    monkeypatch.setattr(ops, "_current_stream", lambda dev: state["now"])
    monkeypatch.setattr(ops, "_capturing", lambda: state["capturing"])
    monkeypatch.setattr(ops, "_wait_for_build", lambda tag, stream: state["waits"].append((tag, stream)))
    monkeypatch.setattr(ops, "_keep_for", lambda t, stream: state["kept"].append((t, stream)))
    monkeypatch.setattr(ops, "cross_stream_hits", {})
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    return state


def _tag():
    return ops.StreamTag("cuda:0")


def test_a_same_stream_hit_makes_no_event_or_stream_call(seams):
    """The cost clause: over a same-stream sequence of hits the helper's wait and record_stream run zero times, nothing is
    counted and the tag remembers nothing."""
    tag, buf = _tag(), torch.zeros(4)
    for _ in range(1000):
        ops.order_hit(tag, "pack_mlp", (buf,))
    assert seams["waits"] == [] and seams["kept"] == [] and ops.cross_stream_hits == {} and tag.ordered is None


def test_a_cross_stream_hit_waits_once_per_stream_and_keeps_every_buffer(seams):
    tag, b1, b2 = _tag(), torch.zeros(4), torch.zeros(2)
    B, C = _Stream("B"), _Stream("C")
    seams["now"] = B
    for _ in range(3):
        ops.order_hit(tag, "hidden", (b1, None, b2))
    assert seams["waits"] == [(tag, B)] and [(t is b1 or t is b2, s) for t, s in seams["kept"]] == [(True, B), (True, B)]
    assert ops.cross_stream_hits == {"hidden": 1}
    seams["now"] = C
    ops.order_hit(tag, "hidden", (b1,))
    assert [s for _, s in seams["waits"]] == [B, C] and ops.cross_stream_hits == {"hidden": 2}
    seams["now"] = tag.stream                          # back on the builder's stream: nothing
    ops.order_hit(tag, "hidden", (b1,))
    assert len(seams["waits"]) == 2 and len(seams["kept"]) == 3


def test_nothing_is_issued_while_the_stream_is_capturing(seams):
    tag = _tag()
    seams["now"], seams["capturing"] = _Stream("B"), True
    ops.order_hit(tag, "pack_mlp", (torch.zeros(4),))
    assert seams["waits"] == [] and seams["kept"] == [] and ops.cross_stream_hits == {} and not tag.ordered
    seams["capturing"] = False                         # ... and the hit after the capture is ordered as usual
    ops.order_hit(tag, "pack_mlp", (torch.zeros(4),))
    assert len(seams["waits"]) == 1 and ops.cross_stream_hits == {"pack_mlp": 1}


def test_an_entry_built_off_the_gpu_or_without_a_tag_is_left_alone(seams):
    assert ops.stream_tag(torch.device("cpu")) is None
    seams["now"] = _Stream("B")
    ops.order_hit(None, "csr", (torch.zeros(1),))
    assert seams["waits"] == [] and ops.cross_stream_hits == {}


def test_clear_caches_resets_the_counters(seams):
    ops.cross_stream_hits["pack_mlp"] = 3
    ops.clear_caches()
    assert ops.cross_stream_hits == {}


def test_a_tag_records_its_event_on_the_building_stream(seams):
    tag = _tag()
    assert tag.event is not None and tag.event.stream is tag.stream and tag.stream is seams["now"]
    assert ops.StreamTag("cuda:0", synced=True).event is None
    seams["capturing"] = True
    assert ops.StreamTag("cuda:0").event is None           # nothing runs while a stream is being captured


def test_no_cache_module_builds_a_scheme_of_its_own():
    """One mechanism: outside ops.py's helper no module of the package that keeps or reads a cache issues a stream or event call
    (capture.py records graphs: its stream calls are the capture protocol, not cache ordering).  Which hit paths go through the
    helper is what tests/test_gpu_streams.py shows, cache by cache."""
    for name in ("hidden_cache", "nn_conv", "gcn_conv", "diag_conv", "autograd"):
        src = inspect.getsource(sys.modules["graph_pde_amd." + name])
        assert not re.search(r"wait_event|wait_stream|record_stream|cuda\.Event", src), name
    assert hidden_cache.ops is ops
    rest = inspect.getsource(ops)
    for f in (ops.StreamTag, ops.order_hit, ops._wait_for_build, ops._keep_for):       # the helper itself
        rest = rest.replace(inspect.getsource(f), "")
    assert not re.search(r"wait_event|wait_stream|\.record_stream\(|cuda\.Event", rest)


def _launching_functions():
    """Names of the module-level functions of ops.py from which a launch can be reached: those that pass the current stream to the
    library (`_stream_ptr(`), and - transitively - those that call one of them by name."""
    fns = {n: inspect.getsource(f) for n, f in inspect.getmembers(ops, inspect.isfunction) if f.__module__ == ops.__name__}
    launching = {n for n, s in fns.items() if "_stream_ptr(" in s and n != "_stream_ptr"}
    grew = True
    while grew:
        grew = False
        for n, s in fns.items():
            if n not in launching and any(re.search(r"\b" + re.escape(m) + r"\(", s) for m in launching):
                launching.add(n)
                grew = True
    return launching


def test_the_side_stream_table_names_every_public_entry_point():
    """Every public function of ops.py that takes part in a native call is a row of the side-stream table or is listed, with a
    reason, among the exclusions: a new entry point cannot be added without joining one of the two."""
    public = {n for n in _launching_functions() if not n.startswith("_")}
    assert len(public) >= 40, sorted(public)               # the scan itself still finds the wrappers
    missing = public - set(SIDE_STREAM_TABLE) - set(EXCLUDED)
    assert not missing, f"add to tests/helpers/streams.py SIDE_STREAM_TABLE (and tests/test_gpu_streams.py) or EXCLUDED: {sorted(missing)}"
    assert not set(SIDE_STREAM_TABLE) & set(EXCLUDED)
    stale = (set(SIDE_STREAM_TABLE) | set(EXCLUDED)) - public
    assert not stale, f"listed but not a launching public function of ops.py: {sorted(stale)}"
    assert all(isinstance(r, str) and len(r) > 20 for r in EXCLUDED.values())
    # the issue's named extras are rows, not exclusions
    for name in ("hidden_forward_raw", "edge_weights_raw", "edge_weights_backward_raw", "nnconv_forward_edgeweights_group",
                 "nnconv_backward_deferred_raw", "nnconv_backward_light_raw"):
        assert name in SIDE_STREAM_TABLE
    assert all(n in SIDE_STREAM_TABLE for n in public if n.endswith("_raw") and n not in ("radius_csr_raw",))
