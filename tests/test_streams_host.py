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
    # ... and hits outside ops.py go through the record: no tag is made and no hit is ordered by hand
    for name in ("hidden_cache", "gcn_conv", "chain_any"):
        src = inspect.getsource(sys.modules["graph_pde_amd." + name])
        assert "stream_tag(" not in src and "order_hit(" not in src, name


def _rec(nbytes=0):
    return ops.Cached(nbytes=nbytes)


def test_the_lru_entry_bound_evicts_the_least_recently_hit():
    c = ops.Lru("t", max_entries=2)
    a, b, d = _rec(), _rec(), _rec()
    c.put("a", a)
    c.put("b", b)
    assert c.get("a") is a                      # "a" moves to the MRU end: the victim is "b", not the oldest inserted
    c.put("d", d)
    assert list(c) == ["a", "d"] and c.get("b") is None and len(c) == 2
    one = ops.Lru("t", max_entries=0)           # the entry bound has no keep-one guard
    one.put("a", a)
    assert len(one) == 0


def test_the_lru_byte_bound_keeps_one_entry():
    c = ops.Lru("t", max_bytes=100)
    big, small = _rec(500), _rec(10)
    c.put("big", big)
    assert list(c) == ["big"] and c.nbytes == 500              # one oversized entry stays
    c.put("small", small)
    assert list(c) == ["small"] and c.nbytes == 10             # a second insert evicts the first
    c.put("s2", _rec(60))
    assert list(c) == ["small", "s2"]
    c.get("small")
    c.put("s3", _rec(60))                                       # 130 > 100: the least recently hit goes, then 70 fits
    assert list(c) == ["small", "s3"] and c.nbytes == 70


def test_the_lru_byte_total_is_the_sum_over_its_values():
    c = ops.Lru("t", max_entries=5, max_bytes=1000)
    total = lambda: sum(r.nbytes for r in c.values())
    for i, nb in enumerate((10, 200, 300, 40, 50, 600, 70)):
        c.put(i, _rec(nb))
        c.get(i // 2)
        assert c.nbytes == total()
    c.put(3, _rec(5))                           # a key put again replaces its record
    assert c.nbytes == total() and c.pop(3).nbytes == 5 and c.pop(3) is None and c.pop("absent") is None
    assert c.nbytes == total() and len(c) == len(list(c.values()))
    c.clear()
    assert c.nbytes == 0 == len(c) and total() == 0


def test_a_record_orders_its_hits_and_holds_what_it_declared(seams):
    b1, b2, pin = torch.zeros(4), torch.zeros(2), object()
    rec = ops.Cached("v", (b1, None, b2), (pin,)).stamp("cuda:0")
    assert rec.tag is not None and rec.tag.stream is seams["now"]
    for _ in range(1000):
        rec.hit("pack_mlp")
    assert seams["waits"] == [] and seams["kept"] == [] and ops.cross_stream_hits == {}
    B = seams["now"] = _Stream("B")
    rec.hit("hidden")
    rec.hit("hidden")
    assert seams["waits"] == [(rec.tag, B)] and ops.cross_stream_hits == {"hidden": 1}
    assert len(seams["kept"]) == 2 and all(s is B for _, s in seams["kept"])        # exactly the declared buffers, None skipped
    assert seams["kept"][0][0] is b1 and seams["kept"][1][0] is b2
    held = rec.held()
    assert all(any(h is o for h in held) for o in (b1, b2, pin))
    assert ops.Cached().stamp(torch.device("cpu")).tag is None          # off the GPU: no tag, a hit is left alone
    srt = ops.Pair(b2, (b2,), (b1,))
    first, second = srt                                                 # reads as (source tensor, slot-ordered copy)
    assert srt[0] is b1 and srt[1] is b2 and first is b1 and second is b2


class _Token:
    valid = True

    def drop(self):                                             # (HiddenToken.drop: release_all forgets the token's running sums)
        self.dropped = True


def test_a_slot_holds_only_the_value_built_for_this_key_and_these_parameters(seams):
    p, q = torch.zeros(3), torch.zeros(3)
    slot = hidden_cache._Slot()
    assert not slot.holds(("k",), [p, None])
    tok = _Token()
    slot.store(torch.zeros(2), ("k",), [p, None], ("attr", "csr"), tok, (None,))
    assert slot.holds(("k",), [p, None]) and slot.buffers == (slot.value, None) and slot.pins == ("attr", "csr")
    assert not slot.holds(("other",), [p, None])
    assert not slot.holds(("k",), [q, None]) and not slot.holds(("k",), [p]) and not slot.holds(("k",), [p, q])
    tok.valid = False
    assert not slot.holds(("k",), [p, None])                    # its autograd node has run
    tok.valid = True
    slot.clear()
    assert not slot.holds(("k",), [p, None]) and slot.held() == () and slot.key is None and slot.refs is None and slot.tag is None
    slot.store(torch.zeros(2), ("k",), [p, None], ())           # no token: a value that nothing invalidates
    assert slot.holds(("k",), [p, None])
    del p
    p2 = torch.zeros(3)                                         # an equal key whose parameter object was replaced
    assert not slot.holds(("k",), [p2, None])


def test_release_all_drops_h_and_both_edge_weight_forms_and_nothing_else(seams):
    class M(torch.nn.Module):
        pass

    class DToken(_Token):
        hpart = ("H", "hmax", 64)
    m, p = M(), torch.zeros(3)
    ent = hidden_cache._Entry()
    for slot in (ent.h, ent.w, ent.tw, ent.d):
        slot.store(torch.zeros(2), ("k",), [p], ("attr", "csr"), DToken() if slot is ent.d else _Token() if slot is not ent.w else None)
    assert ent.hidden is ent.h.value and ent.we is ent.w.value and ent.twe is ent.tw.value and ent.dvirtual is ent.d.value
    assert ent.token is ent.h.token and ent.twe_token is ent.tw.token and ent.dtoken is ent.d.token and ent.csr == "csr"
    with pytest.raises(AttributeError):                         # the old names are views: a value enters a slot through store() alone
        ent.hidden = torch.zeros(2)
    ent.hn, ent.dcount, ent.repeats, ent.big_key, ent.last_partial, ent.last_key = 64, 2, True, ("big",), (10, 64), ("k",)
    hidden_cache._entries[m] = ent
    h_token = ent.h.token
    try:
        assert hidden_cache.release_all() and h_token.dropped   # (the running sum of dL/dH goes with the H it belongs to)
        for slot in (ent.h, ent.w, ent.tw):
            assert slot.value is None and slot.held() == () and not slot.holds(("k",), [p])
        assert ent.hidden is None and ent.we is None and ent.twe is None and ent.csr is None and ent.dvirtual is not None
        assert ent.d.holds(("k",), [p]) and ent.d.token.hpart is None and ent.dcount == 2
        assert ent.repeats and ent.big_key == ("big",) and ent.last_partial == (10, 64) and ent.last_key == ("k",)
        assert not hidden_cache.release_all()                   # nothing left to release
    finally:
        hidden_cache.clear()


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


def test_lookup_declares_hmax_and_the_snapshot_pins_it(seams, monkeypatch):
    """`token.hmax` is a device scalar the hidden forward reads on every hit of H: `lookup` declares it as a buffer of the slot, so
    a cross-stream hit keeps it and `hidden_cache.snapshot()` pins it (it did not before the buffers were declared in one place)."""
    hmax, built = torch.ones(1), torch.zeros(8, 32)

    class Built:
        @staticmethod
        def apply(edge_attr, csr, pm, precision, token, n, *params):
            token.hmax = hmax
            return built
    monkeypatch.setattr(hidden_cache, "HiddenFunction", Built)
    monkeypatch.setattr(hidden_cache, "BUDGET_BYTES", 1 << 30)
    conv = torch.nn.Linear(2, 2)
    z = torch.zeros(1, dtype=torch.int32)
    csr, ea = ops.Csr(4, 8, z, z, z, z), torch.randn(8, 6)
    w, b = [torch.randn(32, 6), torch.randn(32, 32), torch.randn(4096, 32)], [None, None, None]
    pm = type("Pm", (), {"dims": (6, 32, 32, 4096)})()
    hidden_cache.clear()
    try:
        with torch.no_grad():
            got = hidden_cache.lookup(conv, ea, csr, pm, w, b, precision="f16split", mode="on")
            assert got[0] is built and got[1] is hmax and got[2] == 4
            h = hidden_cache._entries[conv].h
            assert h.buffers[0] is built and h.buffers[1] is hmax and h.pins[0] is ea and h.pins[1] is csr
            flat = [t for held in hidden_cache.snapshot() if held is not None for t in held]
            assert any(t is hmax for t in flat) and any(t is built for t in flat)
            h.stamp("cuda:0")                                   # as if built on the GPU, on stream A: a hit from B keeps both
            seams["now"] = _Stream("B")
            assert hidden_cache.lookup(conv, ea, csr, pm, w, b, precision="f16split", mode="on")[0] is built
        assert [t for t, _ in seams["kept"]][0] is built and seams["kept"][1][0] is hmax and ops.cross_stream_hits == {"hidden": 1}
    finally:
        hidden_cache.clear()
