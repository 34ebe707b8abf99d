"""Host tier of the call-history tests (tests/helpers/history.py): the generator, the literals, the size of every mutation, the
graphs the themes rely on, the checker's own teeth and the identity probe of ops.attr_in_slot_order.  No library call anywhere: the
walked module is the float32 composite itself (history.CompositeConv)."""
import copy

import pytest
import torch

from graph_pde_amd import hidden_cache, ops
from tests.helpers import history as H

SEEDS = (0, 1, 2, 3)


def _world(seed, graphs=("small",)):
    return H.World(seed, "cpu", make_conv=H.CompositeConv, graphs=graphs)


def test_the_generator_is_deterministic_and_literals_round_trip():
    for theme in H.THEMES:
        a, b = H.walk(theme, 1, 40), H.walk(theme, 1, 40)
        assert a == b and repr(a) == repr(b), "same theme and seed: the same walk"
        assert a != H.walk(theme, 2, 40)
        assert 40 <= len(a) <= 43 and a[:len(H.KNOBS[theme])] == H.KNOBS[theme]
        assert {o.name for o in a} <= set(H.ALPHABET)
        lit = repr({"theme": theme, "seed": 1, "ops": [(o.name,) + o.args for o in a]})
        assert H.parse(lit) == (theme, 1, a)
    every = {o.name for t in H.THEMES for s in SEEDS for o in H.walk(t, s, 40)}
    assert every == set(H.ALPHABET), ("the walks of the suite visit the whole alphabet", set(H.ALPHABET) - every)
    # a literal replays: the same operations, the same numbers
    lit = "{'theme': 'host', 'seed': 3, 'ops': [('train', 2, True), ('write_param', 'w2', 'scale'), ('infer', 2), ('new_attr',), ('twice', 2)]}"
    r1, r2 = H.replay(lit, "cpu", H.CompositeConv, graphs=("small",)), H.replay(lit, "cpu", H.CompositeConv, graphs=("small",))
    assert r1.literal() == r2.literal() and H.parse(r1.literal()) == H.parse(lit)
    assert (r1.worst_fwd, r1.worst_bwd, r1.n_calls, r1.n_grads) == (r2.worst_fwd, r2.worst_bwd, r2.n_calls, r2.n_grads)
    assert r1.n_calls == 6 and r1.n_grads == 2 * 9 and 0 < r1.worst_bwd <= H.TOL_BWD
    # the knobs an operation turned are restored when the checker closes
    before = (hidden_cache.MODE, hidden_cache.BUDGET_BYTES, ops.SAVE_H_MIN_EDGES)
    with H.Checker(_world(0), "kept") as ck:
        ck.run_all(H.KNOBS["kept"] + H.KNOBS["h_half"])
        assert hidden_cache.MODE == "auto" and ops.SAVE_H_MIN_EDGES == 0 and hidden_cache.BUDGET_BYTES == (1 << 30) // 2
    assert (hidden_cache.MODE, hidden_cache.BUDGET_BYTES, ops.SAVE_H_MIN_EDGES) == before


def _answer(oracle, w, g, keep, raw_ea):
    ei = torch.stack([w.raw[g]["src"][keep], w.raw[g]["dst"][keep]])
    with torch.no_grad():
        return oracle(w.g[g]["x"].detach().double(), ei, raw_ea[keep].double())


MUTATING = [H.Op("write_param", which, kind) for which in H.PARAMS for kind in ("scale", "noise")] + \
           [H.Op(name, which) for name in ("write_param_data", "replace_param") for which in H.PARAMS] + \
           [H.Op("replace_mlp"), H.Op("write_attr"), H.Op("new_attr"), H.Op("train", 2, True), H.Op("cpu_round_trip")]


def test_every_mutation_moves_the_float64_answer_by_2e_3():
    """A stale operand must not be able to hide under the bars: each mutation of the alphabet (the SGD step of `train`, the writes
    inside `cpu_round_trip` and the 1.5 x of `inference_mode_call` included) changes the float64 composite's output by at least
    MIN_MOVE = 100 x the backward bar, on the edge set that survives the mutation."""
    w = _world(0)
    g = "small"
    smallest = {}
    with H.Checker(w, "host") as ck:
        for op in MUTATING + MUTATING[:16:2]:       # the "scale" writes twice: the alternating amounts (x 2, then / 2) both get their turn
            before = H.oracle_of(w.convs[0], torch.float64, "cpu")
            ea_before = w.raw[g]["ea"][0].clone()
            ck.run(op)
            keep = w.g[g]["keep"]
            moved = H.rel(_answer(H.oracle_of(w.convs[0], torch.float64, "cpu"), w, g, keep, w.raw[g]["ea"][0]),
                          _answer(before, w, g, keep, ea_before))
            smallest[repr(op)] = min(moved, smallest.get(repr(op), 1e9))
        before = H.oracle_of(w.convs[0], torch.float64, "cpu")
        keep = w.g[g]["keep"]
        smallest["inference_mode_call's edge_attr.mul_(1.5)"] = H.rel(_answer(before, w, g, keep, w.raw[g]["ea"][0] * 1.5),
                                                                     _answer(before, w, g, keep, w.raw[g]["ea"][0]))
    print({k: f"{v:.1e}" for k, v in smallest.items()})
    low = {k: v for k, v in smallest.items() if v < H.MIN_MOVE}
    assert not low, low


@pytest.mark.parametrize("seed", SEEDS)
def test_the_thinned_graphs_keep_what_their_themes_need(seed):
    w = _world(seed, graphs=tuple(H.GRAPHS))
    for name, cur in w.g.items():
        n, ei = H.GRAPHS[name]["n"], cur["ei"]
        e = int(ei.shape[1])
        deg = torch.bincount(ei[1], minlength=n)
        assert e == int(cur["keep"].sum()) and 0.97 * cur["keep"].numel() <= e, "the kink removal thins, it does not gut"
        assert int((deg == 0).sum()) >= 2, "nodes without in-edges"
        assert int((ei[0] == ei[1]).sum()) >= 4, "self-loops"
        assert int(torch.unique(ei, dim=1).shape[1]) <= e - 4, "duplicate edges"
        assert not torch.equal(ei[1], torch.sort(ei[1]).values), "a shuffled edge order"
        assert int(deg.max()) <= n, "(a larger in-degree selects ops.per_edge_association: no cache on that route)"
        if name == "dense":
            assert e > hidden_cache.WE_SMALL_EDGES and e >= 32 * n, "shared H with the in-kernel dL/dH sum, z_buffer, keep_hidden"
            # half the budget of the whole H: a partial H of whole 64-node tiles, at least n / 8 nodes and not all of them
            rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)])
            rows = (w.full_h_bytes("dense") // 2) // (ops.hidden_width(H.DIMS) * 4)
            hn = (int(torch.searchsorted(rowptr, torch.tensor(rows), right=True)) - 1) // 64 * 64
            assert n // 8 <= hn < n and hn > 0 and e * ops.hidden_width(H.DIMS) * 4 <= w.full_h_bytes("dense")
        elif name == "low":
            assert int(deg.max()) <= 6 and e <= 4 * n and e < 32 * n, "the W_e forms by in-degree, the per-edge last layer"
        else:
            assert 4 * n < e <= hidden_cache.WE_SMALL_EDGES and e < 32 * n, "W_e by size, not by in-degree"
    # a "scale" write of a hidden layer is kink-neutral: the graph tensors stay the objects they were
    with H.Checker(w, "host") as ck:
        kept = {k: (v["ei"], v["generation"]) for k, v in w.g.items()}
        ck.run_all([H.Op("write_param", "w1", "scale"), H.Op("write_param", "b2", "scale"), H.Op("write_param", "w2", "scale")])
        assert all(w.g[k]["ei"] is v[0] and w.g[k]["generation"] == v[1] for k, v in kept.items())


class StaleOnce(H.CompositeConv):
    """Answers ONE call from the parameter values it was told to remember: what a cache hit on a stale operand looks like."""

    def forward(self, x, edge_index, edge_attr):
        old = self.__dict__.pop("remembered", None)         # (kept out of the registered submodules)
        if old is not None:
            return old(x, edge_index, edge_attr)
        return super().forward(x, edge_index, edge_attr)


@pytest.mark.parametrize("mutation", [H.Op("write_param", "w3", "scale"), H.Op("write_param", "w1", "scale"), H.Op("write_param", "bias", "scale")])
def test_the_checker_reports_a_stale_answer_at_exactly_that_operation(mutation):
    w = H.World(1, "cpu", make_conv=StaleOnce, graphs=("small",))
    operations = [H.Op("train", 2, False), H.Op("infer", 2), mutation, H.Op("train", 3, False), H.Op("infer", 1)]
    with H.Checker(w, "teeth") as ck:
        ck.run_all(operations[:2])
        stale = copy.deepcopy(w.convs[0])
        ck.run(operations[2])
        w.convs[0].__dict__["remembered"] = stale  # the next call - the FIRST application of operation 3 - is answered from before the write
        with pytest.raises(AssertionError) as info:
            ck.run(operations[3])
        text = str(info.value)
        assert "application 0" in text and "theme 'teeth', seed 1, operation 3: ('train', 3, False)" in text, text
        lit = text[text.index("history.replay(") + len("history.replay("):text.rindex(")")]
        assert H.parse(lit) == ("teeth", 1, operations[:4]), "the message carries the executed prefix as a literal"
        ck.run(operations[4])                       # ... and only that operation: the module answers correctly again
    # without the stale answer the same history passes
    H.replay({"theme": "teeth", "seed": 1, "ops": [(o.name,) + o.args for o in operations]}, "cpu", H.CompositeConv, graphs=("small",))


def test_the_identity_probe_stays_inside_the_permutation():
    """ops.attr_in_slot_order samples 4096 slots of `perm`.  Built with a float32 linspace the last index rounded up past the end
    (e = 95,530,006 -> 95,530,008; e = 70,000,007 -> 70,000,008) and `perm[probe]` read out of bounds on the device."""
    sizes = [95_530_000, 95_530_006, 70_000_007] + [(1 << 26) + 8 * k + r + 1 for k in (1, 12345, 3_000_000) for r in (5, 6, 7)] + \
            [(1 << 31) + 7, 1, 2, 4095, 4096, 4097, 40000]
    for e in sizes:
        probe = ops.identity_probe(e)
        assert probe.dtype == torch.int64 and probe.numel() == min(e, 4096)
        assert int(probe.min()) == 0 and int(probe[0]) == 0 and int(probe.max()) < e and int(probe[-1]) == e - 1, e
        assert e == 1 or bool((probe[1:] > probe[:-1]).all()), "distinct, increasing slots"
    assert int(torch.linspace(0, 95_530_006 - 1, 4096).to(torch.int32)[-1]) >= 95_530_006, "what the float32 probe did"


def test_a_new_tensor_on_an_old_address_is_not_the_parameter_a_key_names():
    """hidden_cache keys name a parameter by (data_ptr, version); `_param_refs` / `_same_params` add the object's identity.  A
    fresh tensor - a replaced Parameter, the copy ops.stage_const makes again after an eviction - with the same address and
    version must not pass for the old one (the suspects 1 and 2 of DESIGN.md "Call histories")."""
    old = [torch.empty(8, 8), None, torch.empty(24)]
    refs, named = hidden_cache._param_refs(old), [(None if t is None else (t.data_ptr(), t._version)) for t in old]
    assert hidden_cache._same_params(refs, old)
    assert not hidden_cache._same_params(refs, old[:2]) and not hidden_cache._same_params(None, old)
    assert not hidden_cache._same_params(refs, [old[0], old[2], None]), "None and a tensor do not stand in for each other"
    # another OBJECT with the same (address, version) without asking an allocator for it: detach() shares memory and counter
    new = [None if t is None else t.detach() for t in old]
    assert [(None if t is None else (t.data_ptr(), t._version)) for t in new] == named and all(a is not b for a, b in zip(new, old) if a is not None)
    assert not hidden_cache._same_params(refs, new), "equal (address, version), another object"
    assert hidden_cache._same_params(hidden_cache._param_refs(new), new)
    del old
    assert not hidden_cache._same_params(refs, new), "a dead parameter matches nothing"


def test_a_forward_can_tell_a_backward_pass_and_a_checkpointed_segment():
    """autograd.in_backward_pass / saved_tensor_hooks_active: what hidden_cache asks before it touches in-flight sums or builds a
    shared node.  Seen from a custom Function's forward: plain, inside a checkpointed segment, inside its recomputation."""
    from torch.utils.checkpoint import checkpoint
    from graph_pde_amd import autograd as ag
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            seen.append((ag.in_backward_pass(), ag.saved_tensor_hooks_active()))
            ctx.save_for_backward(x)
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append(("backward", ag.in_backward_pass()))
            return g * ctx.saved_tensors[0].new_full((), 2.0)

    assert ag.CAN_TELL_BACKWARD_PASS and not ag.in_backward_pass() and not ag.saved_tensor_hooks_active()
    x = torch.randn(3, requires_grad=True)
    Probe.apply(x).sum().backward()
    assert seen == [(False, False), ("backward", True)]
    del seen[:]
    checkpoint(lambda t: Probe.apply(t), x, use_reentrant=False).sum().backward()
    # forward; the backward, whose access to its saved tensor starts the recomputation inside the pass
    assert seen == [(False, True), ("backward", True), (True, True)], seen
    with torch.autograd.graph.save_on_cpu():
        assert ag.saved_tensor_hooks_active()
    assert not ag.saved_tensor_hooks_active()
