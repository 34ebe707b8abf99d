"""GPU tier: call HISTORIES of a module - no cached state may change its answer (tests/helpers/history.py).

`conv(x, edge_index, edge_attr)` goes through a host-side state machine (hidden_cache._Entry, the in-place sums and the stash of
autograd.py, the address + version keyed caches of ops.py) that decides from the call history which kernels run on which cached
tensors.  Here modules are moved through histories and EVERY call is compared with the float64 composite of the reference's op chain
on the current values: forward <= max(1e-5, 4 e32) per application given the input it received, gradients <= max(2e-5, 4 e32) against
float64 autograd of the whole step.  A call meets the bars or raises an exception that names its cause - never another number.

  * one walk per (theme, seed): ~40 operations drawn deterministically; at its end the walk must have visited what its theme is
    for (counters of hidden_cache.stats / ops / _lib) and at least 3 stale opportunities (a mutation while the entry held a live
    H, W_e, W_e node or virtual-H node; theme "kept" has no entry - GPDE_HIDDEN_CACHE=off - and counts mutations under a live
    weight pack instead);
  * eleven scripted scenarios, the suspects of a code reading among them.
DESIGN.md "Call histories" records the counters, errors and times measured."""
import gc
import time

import pytest
import torch

from graph_pde_amd import _lib, hidden_cache, ops
from oracle.nnconv_oracle import nnconv_forward
from tests.helpers import history as H
from tests.helpers.history import Op

pytestmark = pytest.mark.gpu
LENGTH = 40
SEEDS = (0, 1, 2, 3)


class _Counts(dict):
    def __missing__(self, key):
        return 0


def _fresh():
    assert torch.cuda.is_available(), "GPU tier needs an MI355X"
    gc.collect()
    hidden_cache.clear()
    ops.clear_caches()
    return {"kept": ops.n_kept_hidden, "accumulated": ops.n_grad_hidden_accumulated, "native": _lib.n_native_calls}


def _moved(c0, ck=None):
    st = dict(hidden_cache.stats)
    for k, v in (ck.stats_before_clear.items() if ck is not None else ()):
        st[k] = st.get(k, 0) + v
    st.update(kept=ops.n_kept_hidden - c0["kept"], accumulated=ops.n_grad_hidden_accumulated - c0["accumulated"],
              native=_lib.n_native_calls - c0["native"])
    return _Counts(st)


def _script(theme, seed, operations, graphs=None):
    """KNOBS[theme] + `operations` on a fresh world; returns (checker, counters)."""
    c0 = _fresh()
    world = H.World(seed, "cuda:0", graphs=graphs or H.THEME_GRAPHS[theme])
    with H.Checker(world, theme) as ck:
        t0 = time.perf_counter()
        ck.run_all(list(H.KNOBS[theme]) + list(operations))
        torch.cuda.synchronize()
        ck.seconds = time.perf_counter() - t0
        st = _moved(c0, ck)
    print(f"\n{theme}/{seed}: {len(ck.done)} operations, {ck.n_calls} applications and {ck.n_grads} gradients checked in {ck.seconds:.2f} s; "
          f"worst forward {ck.worst_fwd:.1e}, backward {ck.worst_bwd:.1e}; stale opportunities {ck.stale} (+{ck.stale_pack} weight packs); "
          f"partial H seen {ck.partial_hn_seen}; raised {ck.raised}; collisions {ck.collisions}; counters {dict(st)}")
    return ck, st


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("theme", H.THEMES)
def test_walk(theme, seed):
    operations = H.walk(theme, seed, LENGTH)
    ck, st = _script(theme, seed, operations[len(H.KNOBS[theme]):])
    assert st["native"] > 0 and ck.n_calls >= 40 and ck.n_grads >= 45
    # a call may end in a named cause only from `checkpointed` / `oom_once` (history.named_cause), at most once per such operation
    may = [i for i, o in enumerate(ck.done) if o.name in ("checkpointed", "oom_once")]
    assert {r[0] for r in ck.raised} <= set(may) and len(ck.raised) <= len(may), (ck.raised, may)
    if theme == "kept":
        assert ck.stale_pack >= 3, "mutations while ops.pack_mlp held this module's weights"
        assert st["kept"] >= 3 and st["builds"] == 0 and st["we_builds"] == 0, st
    else:
        assert ck.stale >= 3, "mutations while the entry held a live H / W_e / W_e node / virtual-H node"
    if theme == "h_fits":
        assert st["builds"] >= 3 and st["hits"] >= 3 and st["accumulated"] >= 3 and st["we_builds"] == 0 and st["deferred_builds"] == 0, st
    elif theme == "h_half":
        assert st["deferred_builds"] >= 3 and st["deferred_hits"] >= 3 and ck.partial_hn_seen >= 3 and st["we_builds"] == 0, st
    elif theme == "h_none":
        assert st["deferred_builds"] >= 3 and st["deferred_hits"] >= 3 and ck.partial_hn_seen == 0 and st["builds"] == 0, st
    elif theme == "we":
        assert st["we_builds"] >= 3 and st["we_hits"] >= 3 and st["builds"] >= 3, st
    elif theme == "shifting":
        assert set(ck.regimes) == set(H.THEMES[:-1]), ck.regimes
        assert all(st[k] > 0 for k in ("builds", "we_builds", "deferred_builds", "kept")) and ck.partial_hn_seen > 0, \
            ("every route ran, not only its knobs were set", st, ck.partial_hn_seen)


# ----------------------------------------------------------------------------------------------------------------------------
# scripted scenarios
# ----------------------------------------------------------------------------------------------------------------------------
WARM = [Op("train", 3, False), Op("train", 2, True)]          # the policy has seen the module repeat its key


@pytest.mark.parametrize("route", ["H", "W_e"])
def test_1_a_replaced_parameter_on_a_recycled_address(route):
    """`conv.nn[i].weight = Parameter(...)`: a new object, version 0, on the address the old one freed.  hidden_cache named the
    parameters by (data_ptr, version) only, so the cached H (an inference H pins nothing) / W_e was served for the new values."""
    c0 = _fresh()
    graph, which = ("dense", "w2") if route == "H" else ("small", "w3")
    world = H.World(0, "cuda:0", graphs=(graph,))
    conv = world.convs[0]
    old = getattr(*H.param_slot(conv, which)).detach().cpu()
    values = old + 0.3 * float(old.std()) * torch.randn(old.shape, generator=world.gen)
    if which == "w2":
        # the edges on a kink of the NEW hidden layer leave the graph now: the replacement then changes the parameter alone
        lin = H.linears(conv)
        for w2 in (values, old):                # (both sets stay registered: the surviving edges are the same before and after)
            world.extra_params.append(([lin[0].weight.detach().cpu(), w2, lin[2].weight.detach().cpu()], [l.bias.detach().cpu() for l in lin]))
        world.rethin()
    generation = world.g[graph]["generation"]
    with H.Checker(world, "scenario 1") as ck:
        ck.run_all([Op("set_mode", "MODE", "on"), Op("set_mode", "WE_MODE", "auto" if route == "W_e" else "off"), Op("set_budget", "full")])
        ck.run(Op("infer", 3))
        ent = hidden_cache._entries[conv]
        assert ent.hidden is not None and ent.token.valid and (route == "H" or ent.we is not None), "the entry holds what the route caches"
        collided = ck._replace_param(conv, which, values)
        assert collided, f"the new parameter did not land on the old one's address and version: {ck.collisions}"
        world.rethin()
        assert world.g[graph]["generation"] == generation, "the graph is the one H was built for"
        ck.run(Op("infer", 3))
        ck.run(Op("train", 2, False))
    print(dict(hidden_cache.stats), ck.worst_fwd, ck.worst_bwd)
    assert not ck.raised and hidden_cache.stats["builds"] >= 2 and _lib.n_native_calls > c0["native"]


def test_2_a_cpu_resident_max_module_after_its_staged_weights_were_evicted():
    """model.cpu(), aggr='max', no_grad: the per-edge weights are cached on the keys of the STAGED device copies (ops.stage_const,
    16 entries).  After an in-place CPU update and more than 16 other staged tensors, the new copies start at version 0 on the
    addresses the evicted ones freed."""
    _fresh()
    world = H.World(0, "cuda:0", graphs=("small",), aggr="max", n_convs=1)
    conv, cur = world.convs[0].cpu(), world.g["small"]
    ei, ea, x = cur["ei"].cpu(), cur["ea"][0].cpu(), cur["x"].detach().cpu()
    dev = torch.device("cuda:0")

    def check(what):
        with torch.no_grad():
            y = conv(x, ei, ea)
        lin = H.linears(conv)
        args = (x, ei, ea, [l.weight.detach() for l in lin], [l.bias.detach() for l in lin], conv.root.detach(), conv.bias.detach())
        ref = nnconv_forward(*args, aggr="max", dtype=torch.float64, chunk_edges=1024)
        e32 = H.rel(nnconv_forward(*args, aggr="max", dtype=torch.float32, chunk_edges=1024), ref)
        err = H.rel(y, ref)
        print(f"{what}: {err:.1e} from float64 (float32 oracle {e32:.1e})")
        assert err <= max(H.TOL_FWD, H.FACTOR * e32), (what, err, e32)
        return [t.data_ptr() for t in sum(conv._params_on(dev, False)[:2], [])]

    first = check("first evaluation")
    assert check("second evaluation") == first and hidden_cache.stats["we_hits"] >= 1, "the cached per-edge weights were in use"
    with torch.no_grad():                       # a CPU optimizer step on what the kinks do not depend on
        H.linears(conv)[-1].weight.mul_(1.5)
        H.linears(conv)[-1].bias.add_(0.05)
        conv.root.mul_(1.5)
    built = hidden_cache.stats["we_builds"]
    others = [torch.randn(1000 + 37 * k) for k in range(20)]
    for t in others:
        ops.stage_const(t, dev)
    gc.collect()
    again = check("after the update and 20 other staged tensors")
    assert hidden_cache.stats["we_builds"] == built + 1, "the per-edge weights were built again for the updated weights"
    print("staged weights on the addresses of the evicted copies:", [a == b for a, b in zip(first, again)])
    check("once more")


def test_3_two_modules_on_one_graph_alternating_one_updated():
    for theme in ("h_fits", "we"):
        g = H.THEME_GRAPHS[theme][0]
        c0 = _fresh()
        world = H.World(0, "cuda:0", graphs=(g,))
        plan = [(0, g, 0), (1, g, 0), (0, g, 0), (1, g, 0)]
        with H.Checker(world, theme) as ck:
            ck.run_all(H.KNOBS[theme])
            for _ in range(2):
                assert ck.step(plan, grad="full") and ck.step(plan, grad="none")
            ck.run_all([Op("write_param", "w3", "scale"), Op("write_param", "w1", "scale")])         # module 0 only
            assert ck.step(plan, grad="none") and ck.step(plan, grad="full", sgd=True) and ck.step(plan, grad="full")
        print(theme, dict(hidden_cache.stats), ck.worst_fwd, ck.worst_bwd)
        assert not ck.raised and hidden_cache.stats["hits"] >= 2


@pytest.mark.parametrize("mode", ["auto", "on"])
def test_4_one_module_on_two_graphs_alternately_within_one_step(mode):
    """The MGKN V-cycle pattern: the entry is per module and holds ONE key; alternating graphs drop and rebuild H and its tokens
    while autograd nodes of the same step still hang on the old ones."""
    _fresh()
    world = H.World(1, "cuda:0", graphs=("dense", "small"))
    plan = [(0, "dense", 0), (0, "small", 0), (0, "dense", 0), (0, "small", 0)]
    with H.Checker(world, "scenario 4") as ck:
        ck.run_all([Op("set_mode", "MODE", mode), Op("set_mode", "WE_MODE", "auto"), Op("set_budget", "full")])
        for sgd in (False, True, False):
            assert ck.step(plan, grad="full", sgd=sgd)
        assert ck.step([(0, "dense", 0), (0, "dense", 1), (0, "dense", 0), (0, "dense", 1)], grad="full")       # two edge_attr tensors alternately
        assert ck.step(plan, grad="twice")
    print(mode, dict(hidden_cache.stats), ck.worst_fwd, ck.worst_bwd)
    assert not ck.raised


@pytest.mark.parametrize("theme", ["h_fits", "h_half", "h_none", "kept", "we"])
def test_5_backward_twice(theme):
    ck, st = _script(theme, 0, WARM + [Op("twice", 3), Op("twice", 2), Op("train", 2, False)])
    assert not ck.raised


@pytest.mark.parametrize("route", ["shared H", "W_e", "deferred"])
def test_6_a_checkpointed_application_among_plain_ones(route):
    """torch.utils.checkpoint runs a forward INSIDE the backward pass, while the plain applications of the step have their sums and
    (x, grad_out) pairs in flight on the shared token.  The segment takes the direct operator both times (hidden_cache.lookup) and
    must leave all of that alone; the plain applications around it keep sharing their node."""
    theme = {"shared H": "h_fits", "W_e": "we", "deferred": "h_half"}[route]
    mode = [] if route == "deferred" else [Op("set_mode", "MODE", "on")]
    ck, st = _script(theme, 0, mode + WARM + [Op("checkpointed", 3, 1), Op("checkpointed", 3, 2), Op("train", 3, False)])
    assert not ck.raised, "a checkpointed application of a settled module is served, not refused"
    assert st["hooked_direct"] >= 4, "two segments, forward and recomputation each"
    if route == "shared H":
        assert st["accumulated"] >= 4, "the plain applications of every step summed dL/dH in place"
    elif route == "W_e":
        assert st["we_builds"] >= 3
    else:
        assert st["deferred_hits"] >= 4


@pytest.mark.parametrize("theme", ["h_fits", "h_half", "we"])
def test_6b_the_checkpointed_application_is_the_first_of_its_step(theme):
    """The FIRST application of a step is the one that would build H / the virtual-H node / W_e.  Built inside the checkpointed
    segment, the node saves that segment's placeholders: the recomputation then finds it cached and saves other tensors than the
    forward did (CheckpointError), and a later plain step that hangs on it fails in ITS backward.  A segment under saved-tensor
    hooks therefore takes the direct operator and leaves the entry alone (hidden_cache.lookup)."""
    ck, st = _script(theme, 0, WARM + [Op("checkpointed", 3, 0), Op("train", 3, False), Op("checkpointed", 2, 0), Op("abandon", 2),
                                       Op("train", 2, True), Op("infer", 2)])
    assert not ck.raised and st["hooked_direct"] >= 4, (ck.raised, st)


@pytest.mark.parametrize("what", ["release_all", "clear_caches"])
@pytest.mark.parametrize("theme", ["h_fits", "h_half", "h_none", "kept", "we"])
def test_7_caches_dropped_between_forward_and_backward(theme, what):
    ck, st = _script(theme, 1, WARM + [Op("between", 3, what), Op("train", 3, False), Op("between", 2, what), Op("infer", 2)])
    assert not ck.raised


@pytest.mark.parametrize("theme", ["h_fits", "h_half", "we"])
def test_8_input_gradients_only_then_a_complete_step(theme):
    ck, st = _script(theme, 0, WARM + [Op("input_grads_only", 3), Op("train", 3, False), Op("input_grads_only", 2), Op("train", 2, True), Op("train", 2, False)])
    assert not ck.raised


@pytest.mark.parametrize("theme", ["h_fits", "h_half", "h_none", "kept", "we"])
def test_9_inference_between_a_training_forward_and_its_backward(theme):
    ck, st = _script(theme, 1, WARM + [Op("infer_inside_train", 3), Op("infer_inside_train", 2), Op("train", 2, False)])
    assert not ck.raised


@pytest.mark.parametrize("where", ["hidden_forward_raw", "edge_weights_raw"])
@pytest.mark.parametrize("theme", ["h_fits", "kept", "we"])
def test_10_out_of_memory_once_then_an_ordinary_call(theme, where):
    ck, st = _script(theme, 0, WARM + [Op("oom_once", where), Op("infer", 2), Op("oom_once", where), Op("train", 2, False)])
    if (theme, where) in (("h_fits", "hidden_forward_raw"), ("kept", "hidden_forward_raw"), ("we", "hidden_forward_raw"), ("we", "edge_weights_raw")):
        assert ck._oom.get(where, 0) >= 1, "the site was reached"
    assert all(H.INJECTED in r[2] for r in ck.raised), ck.raised


@pytest.mark.parametrize("theme", ["h_fits", "we"])
def test_11_a_call_that_raises_after_the_entry_changed(theme):
    ck, st = _script(theme, 0, WARM + [Op("raise_in_forward"), Op("train", 2, True), Op("infer", 2)])
    assert not ck.raised
