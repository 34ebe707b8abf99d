"""Which regime a call of the MODULES takes, recorded at the library boundary on the GPU: `_lib.lib()` is replaced by a stand-in
that notes every native call and forwards it to the real library, and each scenario of the table below - a call of `NNConv_old`,
`NNConvDiag` or `nnconv_group` with its regime forced through the module constants the other tests patch - is written down as

  * "calls"    the ordered native entry points it reached (forward and backward), each with its arguments by position: a scalar's
               value, None / "ptr" for a NULL / non-NULL pointer, the elements of a ctypes array, the fields of a descriptor;
  * "stats"    the change of `hidden_cache.stats`, `ops.n_kept_hidden` and `ops.n_grad_hidden_accumulated`;
  * "grad_fn"  the class name of each output's autograd node (None without one);
  * "raises"   for a scenario that must refuse: the exception's type and full text.

tests/golden/module_routes.json is this record (tests/golden/make_module_routes.py), taken BEFORE the module front of nn_conv.py /
diag_conv.py was folded into one path; tests/test_gpu_module_routes.py replays it.  Only public names of `ops`, `hidden_cache`,
`_lib` and the modules' public surface are used: the record can be regenerated at the commit that precedes the fold.

Left out of the record (written "~"), because they follow the device memory that happens to be free:
  * `ws_bytes`      the size of the workspace handed to an entry point (ops sizes workspaces from the free memory);
  * `budget_bytes`, `n_blocks`   the node-block plan of the streamed any-width route (chain_any sizes its blocks from the same);
and the `*workspace_bytes*` queries, as `native_recorder.operator_calls` leaves them out.

`scenario_tensors` is the other use of the table: every output and gradient of a scenario, for a bit-for-bit A/B of two versions of
the module files over one library."""
import contextlib
import ctypes
import re
from unittest import mock

import torch
import torch.utils.checkpoint

import graph_pde_amd as gp
from graph_pde_amd import _lib, hidden_cache, ops, synth

FREE_MEMORY_SCALARS = ("ws_bytes", "budget_bytes", "n_blocks")
SMALL, BIG, TWO = [6, 16, 32, 4096], [6, 256, 256, 4096], [6, 32, 4096]
ANY = [6, 16, 32, 24 * 40]

# every scenario runs under ALL of these (its own overrides on top): nothing is left to the environment
KNOBS = {(hidden_cache, "MODE"): "auto", (hidden_cache, "WE_MODE"): "off", (hidden_cache, "DEFER_MODE"): "auto",
         (hidden_cache, "BUDGET_BYTES"): 1 << 30, (hidden_cache, "WE_SMALL_EDGES"): 8192, (hidden_cache, "WE_BUDGET_BYTES"): 4 << 30,
         (ops, "SAVE_H_BYTES"): 0, (ops, "SAVE_H_MIN_EDGES"): 262144, (ops, "ANY_REASSOC"): "auto"}
_OWNER = {name: owner for owner, name in KNOBS}


# ---------------------------------------------------------------------------------------------------------------------------
# the forwarding stand-in
# ---------------------------------------------------------------------------------------------------------------------------
def _param_names() -> dict:
    """{entry point: [parameter names]} of include/gpde.h (`_lib.header_prototypes` keeps the types only)."""
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"GPDE_API\s+[\w \*]+?\s*\b(gpde_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = " ".join(m.group(2).split())
        out[m.group(1)] = [] if args in ("", "void") else [re.search(r"(\w+)\s*$", a).group(1) for a in args.split(",")]
    return out


def _struct(o):
    if not isinstance(o, ctypes.Structure):
        return "out"                                    # byref(c_int32()) and the like: a result the library writes
    rec = {}
    for name, ct in o._fields_:
        v = getattr(o, name)
        rec[name] = (None if not v else "ptr") if ct is ctypes.c_void_p else [int(s) for s in v] if isinstance(v, ctypes.Array) else int(v)
    return rec


def _argument(ct, a):
    if ct is not ctypes.c_void_p:
        return a if isinstance(a, float) else int(a)
    if a is None or (isinstance(a, int) and a == 0):
        return None
    if isinstance(a, ctypes.Array):
        if issubclass(a._type_, ctypes.Structure):
            return [_struct(v) for v in a]
        return [(None if not v else "ptr") for v in a] if a._type_ is ctypes.c_void_p else [int(v) for v in a]
    if hasattr(a, "_obj"):
        return _struct(a._obj)
    return "ptr"


class ForwardingLibrary:
    """Stands in for the ctypes library: notes every call that is not a workspace query, then makes it."""

    def __init__(self, real):
        self._real, self._names, self.calls = real, _param_names(), []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if "workspace_bytes" in name or name == "gpde_last_error":
            return fn
        argtypes, names = _lib.SIGNATURES[name][1], self._names[name]
        assert len(argtypes) == len(names), name

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args))
            self.calls.append([name, ["~" if p in FREE_MEMORY_SCALARS else _argument(ct, a) for ct, p, a in zip(argtypes, names, args)]])
            return fn(*args)
        return call


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: seeded on the CPU, copied to the device
# ---------------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


def rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def mlp(dims, act=torch.nn.ReLU):
    layers = sum([[torch.nn.Linear(dims[i], dims[i + 1]), act()] for i in range(len(dims) - 1)], [])[:-1]
    return torch.nn.Sequential(*layers)


def conv(dims=SMALL, cin=64, cout=64, aggr="mean", cls=None, seed=1, frozen=False, on=None, act=torch.nn.ReLU, **kw):
    torch.manual_seed(seed)
    m = (cls or gp.NNConv_old)(cin, cout, mlp(dims, act), aggr=aggr, **kw)
    if frozen:
        m.requires_grad_(False)
    return m.to(dev() if on is None else on)


_graphs = {}


def graph(name):
    """(edge_index, edge_attr, n) on the CPU, built once: g16 / g10 the Darcy lattices (mean in-degree 18 / 56), `ring` 64 nodes with
    two in-edges each, `star` 8 nodes with 40 parallel edges into node 0 (ops.per_edge_association holds), `none` without edges."""
    if name not in _graphs:
        if name in ("g16", "g10"):
            _graphs[name] = synth.darcy_graph(16, 0.15) if name == "g16" else synth.darcy_graph(10, 0.6)
        elif name == "ring":
            i = torch.arange(64)
            _graphs[name] = (torch.stack([torch.cat([(i + 63) % 64, (i + 1) % 64]), torch.cat([i, i])]), rand(11, 128, 6), 64)
        elif name == "star":
            _graphs[name] = (torch.stack([torch.arange(40) % 8, torch.zeros(40, dtype=torch.int64)]), rand(12, 40, 6), 8)
        elif name == "none":
            _graphs[name] = (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, 6), 16)
        elif name == "two":                              # 50 sources -> 30 destinations, 300 edges
            g = torch.Generator().manual_seed(13)
            _graphs[name] = (torch.stack([torch.randint(0, 50, (300,), generator=g), torch.randint(0, 30, (300,), generator=g)]),
                             rand(14, 300, 6), (50, 30))
    return _graphs[name]


def on_dev(name, width=64, seed=2, to=None):
    """(x, edge_index, edge_attr) of a square graph where the scenario runs (fresh tensors: no cache key survives a scenario)."""
    ei, ea, n = graph(name)
    d = dev() if to is None else to
    return rand(seed, n, width).to(d), ei.clone().to(d), ea.clone().to(d)


def node_attr(requires_grad=False):
    """The g16 lattice's edge attributes as a node table (ops.NodeAttr.darcy)."""
    pos, a = synth.lattice_positions(16).float(), synth.darcy_coefficient(16)
    if not requires_grad:
        return ops.NodeAttr.darcy(pos.to(dev()), a.to(dev()))
    table = torch.cat([pos, a.reshape(-1, 1)], dim=1).to(dev()).requires_grad_(True)
    return ops.NodeAttr(table, [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (1, 2)])


def partial_budget(name, dims, nodes):
    """hidden_cache.BUDGET_BYTES under which H of the in-edges of `nodes` leading nodes fits and the whole H does not."""
    ei, _, n = graph(name)
    rp = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    assert int(rp[nodes - 1]) < int(rp[-1])
    return int(rp[nodes - 1]) * ops.hidden_width(dims) * 4


def backward(outs, *leaves):
    """Backward of sum(out * fixed weights) over `outs`; the gradients of `leaves` (tensors or modules), Nones dropped."""
    outs = outs if isinstance(outs, (list, tuple)) else [outs]
    loss = sum((o * rand(99 + k, *o.shape).to(o.device)).sum() for k, o in enumerate(outs))
    loss.backward()
    ts = []
    for l in leaves:
        ts.extend(p for _, p in sorted(l.named_parameters())) if isinstance(l, torch.nn.Module) else ts.append(l)
    return [t.grad for t in ts if t.grad is not None]


# ---------------------------------------------------------------------------------------------------------------------------
# the table: id -> (knob overrides, callable returning (outputs, further tensors to compare))
# ---------------------------------------------------------------------------------------------------------------------------
def scenarios():
    S = {}

    def add(sid, fn, **knobs):
        assert sid not in S, sid
        S[sid] = (knobs, fn)

    def plain(name, n_calls=1, grad=False, mode=None, glue=None, warm=0, **ckw):
        """`warm` plain calls, then `n_calls` calls (with `glue`) of one module on one graph; without a gradient unless `grad`."""
        def run():
            m = conv(**ckw)
            x, ei, ea = on_dev(name)
            kw = {} if glue is None else {k: (x if k == "residual" else v) for k, v in glue.items()}
            outs = []
            with (contextlib.nullcontext() if grad else (mode or torch.no_grad)()):
                for k in range(warm + n_calls):
                    outs.append(m(x, ei, ea, **(kw if k >= warm else {})))
            return outs, []
        return run

    GLUE = {"residual": {"residual": True}, "relu": {"activation": "relu"}, "both": {"residual": True, "activation": "relu"}}

    # ---- inference, 64 -> 64, Linear / ReLU chain
    add("inf.cold", plain("g16"))
    add("inf.repeat_builds_h_then_hit", plain("g10", n_calls=3))
    add("inf.partial_h_mixed", plain("g10", n_calls=3), MODE="on", BUDGET_BYTES=partial_budget("g10", SMALL, 70))
    add("inf.we_auto_ring", plain("ring", n_calls=4), WE_MODE="auto")
    add("inf.we_forced_by_max", plain("g16", n_calls=2, aggr="max"))
    add("refuse.max_over_budget", plain("g16", aggr="max"), WE_BUDGET_BYTES=1 << 20, BUDGET_BYTES=1 << 20)
    add("inf.max_edgeless", plain("none", aggr="max"))
    add("inf.per_edge_association", plain("star"), MODE="off")
    add("inf.hidden_cache_off", plain("g10", n_calls=2), MODE="off")
    add("refuse.float64", lambda: ([conv().double()(*[t.double() if t.is_floating_point() else t for t in on_dev("g16")])], []))
    for g, kw in GLUE.items():
        add(f"glue.{g}.direct", plain("g16", glue=kw), MODE="off")
        add(f"glue.{g}.full_h_hit", plain("g10", glue=kw, warm=1), MODE="on")
        add(f"glue.{g}.we", plain("ring", glue=kw, warm=2), MODE="on", WE_MODE="auto")
    add("glue.both.partial_h_only", plain("g10", glue=GLUE["both"], warm=1), MODE="on", BUDGET_BYTES=partial_budget("g10", SMALL, 70))
    add("glue.both.per_edge_association", plain("star", glue=GLUE["both"]), MODE="off")
    add("glue.both.max", plain("g16", glue=GLUE["both"], aggr="max"))
    add("glue.both.cpu", lambda: ([conv(on="cpu")(*(t := on_dev("g16", to="cpu")), residual=t[0], activation="relu")], []))

    def nodeattr(dims, grad=False, table_grad=False, **kw):
        def run():
            m = conv(dims)
            x, ei, _ = on_dev("g16")
            na = node_attr(table_grad)
            if not grad:
                with torch.no_grad():
                    return [m(x, ei, na, **({"residual": x} if kw.get("residual") else {}))], []
            x.requires_grad_(True)
            out = m(x, ei, na)
            return [out], backward(out, x, m, *([na.table] if table_grad else []))
        return run
    add("inf.nodeattr_3_linear", nodeattr(BIG))
    add("refuse.nodeattr_narrow_network", nodeattr(SMALL))
    add("inf.nodeattr_2_linear", nodeattr(TWO))
    add("inf.nodeattr_residual", nodeattr(BIG, residual=True))

    def prebuilt_csr(flip=False, flow="source_to_target"):
        def run():
            m = conv(flow=flow)
            x, ei, ea = on_dev("g16")
            with torch.no_grad():
                return [m(x, ops.csr_for(ei, x.size(0), flip=True) if flip else ops.build_csr(ei, x.size(0)), ea)], []
        return run
    add("inf.prebuilt_csr", prebuilt_csr())
    add("inf.flow_t2s_tensor", plain("g16", n_calls=2, flow="target_to_source"))
    add("inf.flow_t2s_flipped_csr", prebuilt_csr(flip=True, flow="target_to_source"))
    add("inf.cpu_staged", lambda: _no_grad(lambda: ([conv(on="cpu")(*on_dev("g16", to="cpu")) for _ in range(2)], [])))
    add("inf.cpu_staged_grad_mode", lambda: ([conv(on="cpu", frozen=True)(*on_dev("g16", to="cpu"))], []))
    add("inf.tanh_network", plain("g16", act=torch.nn.Tanh))
    add("inf.inference_mode", plain("g10", n_calls=3, mode=torch.inference_mode))

    # ---- training, 64 -> 64
    def train(name, depth=1, steps=1, ea_grad=False, glue=None, ckpt=False, **ckw):
        def run():
            m = conv(**ckw)
            x, ei, ea = on_dev(name)
            x.requires_grad_(True)
            ea.requires_grad_(ea_grad)
            outs, more = [], []
            for _ in range(steps):
                m.zero_grad(set_to_none=True)
                x.grad = None
                h = x
                for _ in range(depth):
                    if ckpt:
                        h = torch.utils.checkpoint.checkpoint(m, h, ei, ea, use_reentrant=False)
                    elif glue:
                        h = m(h, ei, ea, residual=h, activation="relu")
                    else:
                        h = m(h, ei, ea) if depth == 1 else torch.tanh(m(h, ei, ea))
                outs.append(h)
                more += [g.clone() for g in backward(h, x, m, *([ea] if ea_grad else []))]
            return outs, more
        return run
    add("train.direct_recompute", train("g10"), MODE="off")
    add("train.direct_low_in_degree", train("g16"), MODE="off")
    add("train.direct_h_kept", train("g10", dims=BIG), MODE="off", SAVE_H_BYTES=32 << 30, SAVE_H_MIN_EDGES=0)
    add("train.shared_h_x3", train("g10", depth=3), MODE="on")
    add("train.shared_h_auto_x3_two_steps", train("g10", depth=3, steps=2))
    add("train.we_node_x3", train("ring", depth=3, steps=2), MODE="on", WE_MODE="auto")
    add("train.partial_deferred_x3", train("g10", depth=3, steps=2, dims=BIG), BUDGET_BYTES=partial_budget("g10", BIG, 70))
    add("train.over_budget_narrow_network_x3", train("g10", depth=3, steps=2), BUDGET_BYTES=partial_budget("g10", SMALL, 70))
    add("train.deferred_off_x3", train("g10", depth=3, steps=2, dims=BIG), BUDGET_BYTES=partial_budget("g10", BIG, 70), DEFER_MODE="off")
    add("train.edge_attr_grad", train("g16", ea_grad=True), MODE="on")
    add("train.nodeattr", nodeattr(BIG, grad=True))
    add("train.nodeattr_narrow_network", nodeattr(SMALL, grad=True))
    add("train.nodeattr_2_linear", nodeattr(TWO, grad=True))
    add("train.nodeattr_table_grad", nodeattr(BIG, grad=True, table_grad=True))
    add("train.max", train("g16", aggr="max"))
    add("train.max_t2s", train("g16", aggr="max", flow="target_to_source"))
    add("train.glue_unfused", train("g16", glue=True), MODE="off")
    add("train.tanh_network", train("g16", act=torch.nn.Tanh))
    add("refuse.tanh_network_max_grad", train("ring", act=torch.nn.Tanh, aggr="max"))
    add("train.per_edge_association", train("star"), MODE="off")
    add("train.checkpoint", train("g10", depth=2, ckpt=True), MODE="on")
    add("train.cpu_staged", lambda: _cpu_train())

    def _cpu_train():
        m = conv(on="cpu")
        x, ei, ea = on_dev("g16", to="cpu")
        x.requires_grad_(True)
        out = m(x, ei, ea)
        return [out], backward(out, x, m)

    # ---- nnconv_group: one list that mixes every kind of call
    def group():
        a, b, c = conv(frozen=True), conv(frozen=True, seed=3), conv(seed=4)
        two, other = conv(frozen=True, cin=(64, 64), seed=5), conv(ANY, 24, 40, frozen=True, seed=6)
        xr, eir, ear = on_dev("ring")
        xg, eig, eag = on_dev("g16")
        (eit, eat, (ns, nd)) = graph("two")
        xs, xd = rand(21, ns, 64).to(dev()), rand(22, nd, 64).to(dev())
        xo = rand(23, 256, 24).to(dev())
        xc = xr.clone().requires_grad_(True)
        calls = [(a, xr, eir, ear), (b, xg, eig, eag), (a, xr, eir, ear, xr, "relu"), (b, xg, eig, eag, xg, "relu"),
                 (two, (xs, xd), eit.to(dev()), eat.to(dev())), (other, xo, eig, eag), (c, xc, eir, ear, xc)]
        outs = gp.nnconv_group(calls)
        return outs, backward(outs[-1], xc, c)
    add("group.mixed", group, WE_SMALL_EDGES=1000)
    add("group.mixed_no_grad", lambda: _no_grad(group_plain), WE_SMALL_EDGES=1000)

    def group_plain():
        a, b = conv(), conv(seed=3)
        xr, eir, ear = on_dev("ring")
        xg, eig, eag = on_dev("g16")
        return gp.nnconv_group([(a, xr, eir, ear), (b, xg, eig, eag, None, "relu"), (a, xr, eir, ear, xr), (b, xr, eir, ear)]), []

    def _no_grad(fn):
        with torch.no_grad():
            return fn()

    # ---- other widths and two node sets
    def any_width(route, grad, glue=False, aggr="mean", flow="source_to_target", act=torch.nn.ReLU):
        def run():
            m = conv(ANY, 24, 40, aggr=aggr, flow=flow, act=act)
            x, ei, ea = on_dev("g16", 24)
            kw = {"residual": rand(31, 256, 40).to(dev()), "activation": "relu"} if glue else {}
            if not grad:
                return _no_grad(lambda: ([m(x, ei, ea, **kw)], []))
            x.requires_grad_(True)
            out = m(x, ei, ea, **kw)
            return [out], backward(out, x, m)
        return run
    for route, knob in (("materialised", "off"), ("reassociated", "on"), ("streamed", "streamed")):
        add(f"any.{route}", any_width(route, False), ANY_REASSOC=knob)
        add(f"any.{route}.grad", any_width(route, True), ANY_REASSOC=knob)
        add(f"any.{route}.glue", any_width(route, False, glue=True), ANY_REASSOC=knob)
    add("any.glue.grad", any_width("materialised", True, glue=True))
    add("any.max", any_width("materialised", False, aggr="max"))
    add("any.max.grad", any_width("materialised", True, aggr="max"))
    add("any.max_t2s.grad", any_width("materialised", True, aggr="max", flow="target_to_source"))
    add("any.t2s", any_width("materialised", False, flow="target_to_source"))
    add("any.tanh_network.grad", any_width("materialised", True, act=torch.nn.Tanh), ANY_REASSOC="on")
    add("any.cpu", lambda: _no_grad(lambda: ([conv(ANY, 24, 40, on="cpu")(*on_dev("g16", 24, to="cpu"))], [])))

    def two_sets(cin=(64, 64), cout=64, dims=SMALL, grad=False, x_dst=True, flow="source_to_target", aggr="mean", cls=None, glue=False,
                 via_propagate=False):
        def run():
            m = conv(dims, cin, cout, aggr=aggr, flow=flow, cls=cls)
            ei, ea, (ns, nd) = graph("two")
            ei, ea = (ei.flip(0) if flow == "target_to_source" else ei).clone().to(dev()), ea.clone().to(dev())
            xs, xd = rand(21, ns, cin[0]).to(dev()), rand(22, nd, cin[1]).to(dev())
            kw = {"residual": rand(32, nd, cout).to(dev()), "activation": "relu"} if glue else {}
            call = (lambda x, **k: m.propagate(ei, x=x, pseudo=ea, **k)) if via_propagate else (lambda x, **k: m(x, ei, ea, **k, **kw))
            if not grad:
                return _no_grad(lambda: ([call((xs, xd)) if x_dst else call((xs, None), size=(ns, nd))], []))
            xs.requires_grad_(True), xd.requires_grad_(True)
            out = call((xs, xd))
            return [out], backward(out, xs, xd, m)
        return run
    add("two.64", two_sets())
    add("two.64.grad", two_sets(grad=True))
    add("two.24_40", two_sets((24, 16), 40, ANY))
    add("two.24_40.grad", two_sets((24, 16), 40, ANY, grad=True), ANY_REASSOC="on")
    add("two.x_dst_none", two_sets(x_dst=False))
    add("two.t2s", two_sets(flow="target_to_source", glue=True))
    add("two.max", two_sets(aggr="max"))
    add("two.propagate", two_sets(via_propagate=True))
    add("one.size_alone", lambda: _no_grad(lambda: ([conv()((t := on_dev("g16"))[0], t[1], t[2], size=(256, 256))], [])))
    add("one.pair_of_same_tensor", lambda: _no_grad(lambda: ([conv()(((t := on_dev("g16"))[0], t[0]), t[1], t[2])], [])))
    add("one.propagate", lambda: _no_grad(lambda: ([conv().propagate((t := on_dev("g10"))[1], x=t[0], pseudo=t[2]) for _ in range(2)], [])))
    add("one.propagate_t2s.grad", lambda: _propagate_grad())
    add("one.propagate_any", lambda: _no_grad(lambda: ([conv(ANY, 24, 40).propagate((t := on_dev("g16", 24))[1], x=t[0], pseudo=t[2],
                                                                                      size=(256, 256))], [])))
    add("one.propagate_1d_rows", lambda: _no_grad(lambda: ([conv([1, 16, 32, 4], 1, 4).propagate(
        (t := on_dev("g16", 1))[1], x=t[0][:, 0], pseudo=t[2][:, 0])], [])))

    def _propagate_grad():
        m = conv(flow="target_to_source")
        x, ei, ea = on_dev("g16")
        x.requires_grad_(True)
        out = m.propagate(ei, x=x, pseudo=ea)
        return [out], backward(out, x, m)

    # ---- message() and update()
    def parts(wide, grad, cpu):
        def run():
            d = "cpu" if cpu else dev()
            m = conv(SMALL if wide else ANY, 64 if wide else 24, 64 if wide else 40, on=d)
            cin, cout = (64, 64) if wide else (24, 40)
            xj, ps, ag, x = rand(41, 37, cin).to(d), rand(42, 37, 6).to(d), rand(43, 19, cout).to(d), rand(44, 19, cin).to(d)
            if not grad:
                return _no_grad(lambda: ([m.message(xj, ps), m.update(ag, x)], []))
            xj.requires_grad_(True), x.requires_grad_(True)
            outs = [m.message(xj, ps), m.update(ag, x)]
            return outs, backward(outs, xj, x, m)
        return run
    for wide in (True, False):
        for grad in (False, True):
            for cpu in (False, True):
                add(f"parts.{'64' if wide else '24_40'}.{'grad' if grad else 'no_grad'}.{'cpu' if cpu else 'device'}", parts(wide, grad, cpu))

    # ---- the diagonal modules (they share the front's pieces)
    def diag(name="g16", grad=False, aggr="mean", flow="source_to_target", glue=False, na=False, csr=False, cpu=False):
        def run():
            d = "cpu" if cpu else dev()
            m = conv([6, 16, 64], 64, 64, aggr=aggr, flow=flow, cls=gp.NNConvDiag, on=d)
            x, ei, ea = on_dev(name, to=d)
            if na:
                ea = node_attr()
            if csr:
                ei = ops.build_csr(ei, x.size(0))
            kw = {"residual": x, "activation": "relu"} if glue else {}
            if not grad:
                return _no_grad(lambda: ([m(x, ei, ea, **kw)], []))
            x.requires_grad_(True)
            out = m(x, ei, ea, **kw)
            return [out], backward(out, x, m)
        return run
    add("diag.inference", diag(glue=True))
    add("diag.grad", diag(grad=True, glue=True))
    add("diag.t2s.grad", diag(grad=True, flow="target_to_source"))
    add("diag.max.grad", diag(grad=True, aggr="max", glue=True))
    add("diag.max_t2s_csr.grad", lambda: _diag_max_csr())
    add("diag.nodeattr", diag(na=True))
    add("diag.nodeattr_csr", diag(na=True, csr=True))
    add("diag.cpu.grad", diag(grad=True, cpu=True))
    add("diag.two", two_sets((64, 16), 64, [6, 16, 64], cls=gp.NNConvDiag, glue=True))
    add("diag.two_t2s.grad", two_sets((64, 16), 64, [6, 16, 64], cls=gp.NNConvDiag, grad=True, flow="target_to_source"))
    add("diag.propagate", two_sets((64, 16), 64, [6, 16, 64], cls=gp.NNConvDiag, via_propagate=True))

    def _diag_max_csr():
        m = conv([6, 16, 64], 64, 64, aggr="max", flow="target_to_source", cls=gp.NNConvDiag)
        x, ei, ea = on_dev("g16")
        x.requires_grad_(True)
        out = m(x, ops.csr_for(ei, x.size(0), flip=True), ea)
        return [out], backward(out, x, m)

    # ---- refusals: the type and the full text
    def refuse(fn):
        return lambda: (fn(), [])
    sq = lambda **kw: (conv(**kw), *on_dev("g16", kw.get("cin", 64) if isinstance(kw.get("cin", 64), int) else 64))
    ei2 = lambda: graph("two")[0].clone().to(dev())
    ea2 = lambda: graph("two")[1].clone().to(dev())
    xs2 = lambda w=64: (rand(21, 50, w).to(dev()), rand(22, 30, w).to(dev()))
    add("refuse.nodeattr_two_sets", refuse(lambda: conv(cin=(64, 64))(xs2(), ei2(), node_attr())))
    add("refuse.nodeattr_two_sets_propagate", refuse(lambda: conv(cin=(64, 64)).propagate(ei2(), x=xs2(), pseudo=node_attr())))
    add("refuse.nodeattr_flipped", refuse(lambda: (lambda m, x, ei, ea: m(x, ei, node_attr()))(*sq(flow="target_to_source"))))
    add("refuse.nodeattr_flipped_propagate", refuse(lambda: (lambda m, x, ei, ea: m.propagate(ei, x=x, pseudo=node_attr()))(*sq(flow="target_to_source"))))
    add("refuse.unflipped_csr_t2s", refuse(lambda: (lambda m, x, ei, ea: m(x, ops.build_csr(ei, 256), ea))(*sq(flow="target_to_source"))))
    add("refuse.unflipped_csr_t2s_two_sets", refuse(lambda: conv(cin=(64, 64), flow="target_to_source")(
        xs2(), ops.build_csr(ei2(), 30, n_src=50), ea2())))
    add("refuse.activation", refuse(lambda: (lambda m, x, ei, ea: m(x, ei, ea, activation="gelu"))(*sq())))
    add("refuse.group_activation", refuse(lambda: (lambda m, x, ei, ea: gp.nnconv_group([(m, x, ei, ea, None, "gelu")]))(*sq())))
    add("refuse.propagate_keywords", refuse(lambda: (lambda m, x, ei, ea: m.propagate(ei, x=x, pseudo=ea, extra=1))(*sq())))
    add("refuse.float64_other_width", refuse(lambda: (lambda m, x, ei, ea: m(x.double(), ei, ea))(*sq(dims=ANY, cin=24, cout=40))))
    add("refuse.float64_two_sets", refuse(lambda: conv(cin=(64, 64))(tuple(t.double() for t in xs2()), ei2(), ea2())))
    add("refuse.residual_shape_two_sets", refuse(lambda: conv(cin=(64, 64))(xs2(), ei2(), ea2(), residual=xs2()[0])))
    add("refuse.edge_attr_rows", refuse(lambda: conv(cin=(64, 64))(xs2(), ei2(), ea2()[:-1])))
    add("refuse.max_grad_two_sets", refuse(lambda: conv(cin=(64, 64), aggr="max")(xs2(), ei2(), ea2())))
    add("refuse.width_above_256", refuse(lambda: (lambda m, x, ei, ea: m(rand(2, 256, 300).to(dev()), ei, ea))(
        *sq(dims=[6, 8, 300 * 300], cin=300, cout=300))))
    add("refuse.width_above_256_message", refuse(lambda: conv([6, 8, 300 * 300], 300, 300).message(rand(2, 5, 300).to(dev()), rand(3, 5, 6).to(dev()))))
    add("refuse.x_columns_other_width", refuse(lambda: (lambda m, x, ei, ea: m(x[:, :-1], ei, ea))(*sq(dims=ANY, cin=24, cout=40))))
    add("refuse.x_pair_of_three", refuse(lambda: (lambda m, x, ei, ea: m((x, x, x), ei, ea))(*sq())))
    add("refuse.size_unknown", refuse(lambda: conv(cin=(64, 64))((xs2()[0], None), ei2(), ea2())))
    add("refuse.max_float64", refuse(lambda: _no_grad(lambda: (lambda m, x, ei, ea: m.double()(x.double(), ei, ea.double()))(*sq(aggr="max")))))
    add("refuse.tanh_network_float64", refuse(lambda: (lambda m, x, ei, ea: m.double()(x.double(), ei, ea.double()))(*sq(act=torch.nn.Tanh))))
    add("refuse.constructor_flow", refuse(lambda: gp.NNConv_old(64, 64, mlp(SMALL), flow="sideways")))
    add("refuse.constructor_aggr", refuse(lambda: gp.NNConv_old(64, 64, mlp(SMALL), aggr="min")))
    add("refuse.constructor_keyword", refuse(lambda: gp.NNConv_old(64, 64, mlp(SMALL), node_dim=0)))
    add("refuse.constructor_in_channels", refuse(lambda: gp.NNConv_old((64, 64, 64), 64, mlp(SMALL))))
    add("refuse.diag.constructor_flow", refuse(lambda: gp.NNConvDiag(64, 64, mlp([6, 64]), flow="sideways")))
    add("refuse.diag.constructor_aggr", refuse(lambda: gp.NNConvDiag(64, 64, mlp([6, 64]), aggr="min")))
    add("refuse.diag.constructor_keyword", refuse(lambda: gp.NNConvDiag(64, 64, mlp([6, 64]), node_dim=0)))
    add("refuse.diag.constructor_in_channels", refuse(lambda: gp.NNConvDiag((64, 64, 64), 64, mlp([6, 64]))))
    add("refuse.diag.constructor_widths", refuse(lambda: gp.NNConvDiag(24, 40, mlp([6, 40]))))
    add("refuse.diag.nodeattr_two_sets", refuse(lambda: conv([6, 16, 64], (64, 16), 64, cls=gp.NNConvDiag)(
        (xs2()[0], rand(22, 30, 16).to(dev())), ei2(), node_attr())))
    add("refuse.diag.nodeattr_flipped", refuse(lambda: (lambda m, x, ei, ea: m(x, ei, node_attr()))(
        *sq(dims=[6, 16, 64], cls=gp.NNConvDiag, flow="target_to_source"))))
    add("refuse.diag.unflipped_csr_t2s", refuse(lambda: _no_grad(lambda: (lambda m, x, ei, ea: m(x, ops.build_csr(ei, 256), ea))(
        *sq(dims=[6, 16, 64], cls=gp.NNConvDiag, flow="target_to_source")))))
    add("refuse.diag.unflipped_csr_t2s_two_sets", refuse(lambda: conv([6, 16, 64], (64, 16), 64, cls=gp.NNConvDiag, flow="target_to_source")(
        (xs2()[0], rand(22, 30, 16).to(dev())), ops.build_csr(ei2(), 30, n_src=50), ea2())))
    add("refuse.diag.edge_attr_rows", refuse(lambda: (lambda m, x, ei, ea: m(x, ei, ea[:-1]))(*sq(dims=[6, 16, 64], cls=gp.NNConvDiag))))
    add("refuse.diag.max_grad_two_sets", refuse(lambda: conv([6, 16, 64], (64, 16), 64, cls=gp.NNConvDiag, aggr="max")(
        (xs2()[0], rand(22, 30, 16).to(dev())), ei2(), ea2())))
    add("refuse.diag.propagate_keywords", refuse(lambda: (lambda m, x, ei, ea: m.propagate(ei, x=x))(*sq(dims=[6, 16, 64], cls=gp.NNConvDiag))))
    return S


# ---------------------------------------------------------------------------------------------------------------------------
# running one scenario
# ---------------------------------------------------------------------------------------------------------------------------
def _counters():
    return dict(hidden_cache.stats, n_kept_hidden=ops.n_kept_hidden, n_grad_hidden_accumulated=ops.n_grad_hidden_accumulated)


def run(sid, table=None):
    """(record, tensors) of one scenario: from cleared caches, under KNOBS + its overrides, with the forwarding stand-in in place."""
    knobs, fn = (table or scenarios())[sid]
    hidden_cache.clear()
    ops.clear_caches()
    stub = ForwardingLibrary(_lib.lib())
    rec, tensors = {}, []
    with contextlib.ExitStack() as st:
        for (owner, name), v in KNOBS.items():
            st.enter_context(mock.patch.object(owner, name, knobs.get(name, v)))
        assert all(k in _OWNER for k in knobs), knobs
        st.enter_context(mock.patch.object(_lib, "lib", lambda: stub))
        before = _counters()
        try:
            outs, more = fn()
            torch.cuda.synchronize()
        except Exception as exc:                       # noqa: BLE001  (the refusal IS the record)
            rec["raises"] = [type(exc).__name__, str(exc)]
        else:
            outs = outs if isinstance(outs, (list, tuple)) else [outs]
            rec["grad_fn"] = [None if o.grad_fn is None else type(o.grad_fn).__name__ for o in outs]
            tensors = [t.detach().cpu() for t in list(outs) + list(more)]
        after = _counters()
    rec["calls"] = stub.calls
    rec["stats"] = {k: after[k] - before.get(k, 0) for k in sorted(after) if after[k] != before.get(k, 0)}
    hidden_cache.clear()
    ops.clear_caches()
    return rec, tensors


def record_all():
    table = scenarios()
    return {sid: run(sid, table)[0] for sid in table}


def scenario_tensors():
    table = scenarios()
    return {sid: run(sid, table)[1] for sid in table}
