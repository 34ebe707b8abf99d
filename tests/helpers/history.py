"""Test infrastructure: call HISTORIES of a module - the world, the alphabet of operations, the checker, the generator.

What a user calls is `conv(x, edge_index, edge_attr)`.  Which kernels then run, and on which cached tensors, is decided by a host-side
state machine from the call history: `hidden_cache._Entry` per module, the in-place sums and the (x, grad_out) stash of `autograd.py`,
the five address + version keyed caches of `ops.py`.  A wrong decision there launches correct kernels on stale operands.  This
module moves modules through histories and compares EVERY call with a reference that knows nothing of history.

World (`World`).  Two `gp.NNConv_old(64, 64, mlp)` with the kernel MLP [6, 256, 256, 4096] (keep-H, the deferred form and the W_e
forms all exist at these widths), aggregation `mean` on even seeds and `add` on odd ones, and three graphs (`GRAPHS`):
  dense  n = 256, e = 9216: more than hidden_cache.WE_SMALL_EDGES edges and at least 32 n of them - the shared-H route with the
         in-kernel dL/dH sum, a partial H, the deferred backward, ops.z_buffer / ops.keep_hidden (with SAVE_H_MIN_EDGES = 0);
  low    n = 1024, ~3000 edges, in-degree 0 .. 6: the W_e forms, the per-edge last layer;
  small  n = 200, e = 3000: W_e by size.
Every graph has duplicate edges, self-loops, nodes without in-edges and a shuffled edge order, as tests/helpers/magnitude_classes.
class_graph builds them (`history_graph` is that construction with the heavy node capped at n / 2 in-edges: class_graph's fixed
260 exceeds these node counts, and a maximal in-degree above n selects ops.per_edge_association, a route without any cache).  Each
graph has two edge_attr tensors; the second module shares graphs and attributes with the first.  Edges on a ReLU kink of the kernel
MLP (tests/helpers/kinks.py) are removed for BOTH modules and BOTH attribute tensors, again after every change of a hidden layer or
of an attribute tensor (`World.rethin`): when the surviving set changes, the graph's device tensors are replaced (a new graph is a
history like any other); when it does not, they stay the objects they were.  Hidden-layer writes of kind "scale" multiply W_i, b_i and
every later bias by 2 or 1/2 - exact in floating point, so every pre-activation keeps its ratio to its bound and the graph stays:
the cached H is then stale by the written values ALONE.

Reference.  The reference's op chain in float64 with stock torch ops (tests/helpers/composite_nnconv.py), on the world's device, on
the current values of x, edge_index, edge_attr and the parameters.
  * forward: each application is compared given the fp32 input that application actually received (no compounding over depth);
  * gradients: float64 autograd of the whole step.  Between applications stands a ReLU; the float64 chain applies the MASK of the
    run under test (an entry of a node feature within rounding of 0 may legitimately fall on either side; one flipped entry of
    [n, 64] moves a gradient by ~1 / sqrt(64 n), far above the bar, although no arithmetic is wrong - the same reasoning as kinks.py);
  * bars: forward max(1e-5, 4 e32), gradients max(2e-5, 4 e32), e32 = the distance of the SAME composite in float32 from float64
    on the same inputs (rule and factor of tests/test_gpu_regime_properties.py).  Nothing is taken from the library's output.
Outcome rule: a call meets the bars or raises an exception whose text names the cause (`named_cause`); never another number.

Operations (`Op`): small objects that repr() as Python literals; `walk(theme, seed, length)` draws a deterministic sequence with
random.Random, `Checker.run` executes one, `replay(literal)` a recorded prefix.  Every mutation moves the float64 answer by at least
`MIN_MOVE` = 2e-3 relative (100 x the backward bar: tests/test_history_host.py computes it), so a stale operand cannot hide."""
import ast
import collections
import contextlib
import gc
import random
import time

import torch
import torch.nn.functional as F
from torch.utils.checkpoint import CheckpointError, checkpoint

from graph_pde_amd import hidden_cache, ops
from tests.helpers import composite_nnconv
from tests.helpers.kinks import edges_off_the_kink

DIMS = [6, 256, 256, 4096]
GRAPHS = {"dense": dict(n=256, e=9216, shape="mixed"), "low": dict(n=1024, e=3000, shape="low"), "small": dict(n=200, e=3000, shape="mixed")}
C = 4                                   # disjoint components, node i in component i % C (magnitude_classes.class_graph)
TOL_FWD, TOL_BWD, FACTOR = 1e-5, 2e-5, 4.0
MIN_MOVE = 2e-3
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3", "root", "bias")
HIDDEN_PARAMS = ("w1", "b1", "w2", "b2")
THEMES = ("h_fits", "h_half", "h_none", "kept", "we", "shifting")
INJECTED = "history: injected out of memory in ops."


def history_graph(n: int, e: int, shape: str, g: torch.Generator):
    """(src, dst) int64: magnitude_classes.class_graph with the heavy node of each component capped at n / 2 in-edges."""
    assert n % C == 0
    m = n // C
    heavy = min(260, n // 2)
    if shape == "low":
        deg = torch.randint(0, 7, (n,), generator=g)
    else:
        empty = torch.randperm(m, generator=g)[:max(2, m // 16)]
        body = n - C - C * empty.numel()
        hi = max(9, 2 * (e - C * heavy) // body - 8)
        deg = torch.randint(8, hi + 1, (n,), generator=g)
        for c in range(C):
            deg[C * ((empty + c) % m) + c] = 0                      # nodes without in-edges, other rows in every component
            deg[C * ((m // 2 + 5 * c) % m) + c] = heavy + 7 * c     # one heavy node per component
    dst = torch.repeat_interleave(torch.arange(n), deg)
    cls = dst % C
    src = C * torch.randint(0, m, (dst.numel(),), generator=g) + cls
    for c in range(C):
        idx = (cls == c).nonzero().flatten()
        src[idx[1:6]], dst[idx[1:6]] = src[idx[0]].item(), dst[idx[0]].item()       # five copies of one edge
        src[idx[-6:]] = dst[idx[-6:]]                                                # self-loops
    perm = torch.randperm(dst.numel(), generator=g)                                  # unsorted edge order
    return src[perm], dst[perm]


def kernel_mlp(dims=DIMS):
    return torch.nn.Sequential(*sum([[torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.ReLU()] for i in range(len(dims) - 1)], [])[:-1])


class CompositeConv(torch.nn.Module):
    """A module with NNConv_old's parameters whose forward IS the composite in the dtype of its parameters: the stand-in the host
    tier walks (no library call anywhere), and what the checker's own teeth are tested on."""

    def __init__(self, aggr="mean", dims=DIMS):
        super().__init__()
        self.in_channels = self.out_channels = 64
        self.aggr = aggr
        self.nn = kernel_mlp(dims)
        self.root = torch.nn.Parameter(torch.empty(64, 64).uniform_(-0.125, 0.125))
        self.bias = torch.nn.Parameter(torch.empty(64).uniform_(-0.125, 0.125))

    def forward(self, x, edge_index, edge_attr):
        return composite_nnconv.composite_forward(self, x, edge_index, edge_attr)


def native_conv(aggr):
    import graph_pde_amd as gp
    return gp.NNConv_old(64, 64, kernel_mlp(), aggr=aggr)


def linears(conv):
    return [l for l in conv.nn if isinstance(l, torch.nn.Linear)]


def param_slot(conv, which):
    """(owner module, attribute name) of the parameter called `which`."""
    if which in ("root", "bias"):
        return conv, which
    return linears(conv)[int(which[1]) - 1], "weight" if which[0] == "w" else "bias"


def rel(a, b) -> float:
    a, b = a.detach().to(torch.float64), b.detach().to(torch.float64)
    nb = float(b.norm())
    return float((a - b).norm()) / nb if nb > 0 else float(a.norm())


class Op:
    """One operation of the alphabet: a name and arguments; repr() is the Python literal of the tuple (name, *args)."""
    __slots__ = ("name", "args")

    def __init__(self, name, *args):
        self.name, self.args = str(name), tuple(args)

    def __repr__(self):
        return repr((self.name,) + self.args)

    def __eq__(self, other):
        return isinstance(other, Op) and (self.name, self.args) == (other.name, other.args)

    def __hash__(self):
        return hash((self.name, self.args))


CALLS = ("infer", "train", "input_grads_only", "abandon", "twice", "infer_inside_train", "checkpointed", "inference_mode_call",
         "cpu_round_trip", "oom_once", "raise_in_forward", "between")
MUTATIONS = ("write_param", "write_param_data", "replace_param", "replace_mlp", "write_attr", "new_attr")
ALPHABET = CALLS + MUTATIONS + ("switch_graph", "switch_attr", "other_module", "release_all", "clear_caches", "set_budget", "set_mode", "regime")


def named_cause(ex: BaseException, op_name) -> bool:
    """The exceptions a call may end in instead of a number, each only from the operation that can legitimately produce it:
    `checkpointed` - torch's refusal of a segment whose recomputation took another route than its forward (CheckpointError), or
    the library's own refusal that says what to do (GPDE_ACCUMULATE_DLDH); `oom_once` - the out-of-memory error it injects.
    From any other operation every exception is a failure."""
    if op_name == "checkpointed":
        return isinstance(ex, CheckpointError) or "GPDE_ACCUMULATE_DLDH" in str(ex)
    if op_name == "oom_once":
        return INJECTED in str(ex)
    return False


class World:
    def __init__(self, seed: int, device="cpu", make_conv=None, graphs=tuple(GRAPHS), n_convs: int = 2, aggr=None):
        self.seed, self.device = int(seed), torch.device(device)
        self.aggr = aggr or ("mean" if seed % 2 == 0 else "add")
        self.gen = torch.Generator().manual_seed(7919 * self.seed + 13)       # every random amount of a history, on the host
        make_conv = make_conv or native_conv
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(1000 + self.seed)
            self.convs = [make_conv(self.aggr).to(self.device) for _ in range(n_convs)]
        self.raw, self.g = {}, {}
        self.extra_params = []          # further (weights, biases) sets whose kinks are removed too (a replacement planned ahead)
        self.flip = 1
        for name in graphs:
            spec = GRAPHS[name]
            src, dst = history_graph(spec["n"], spec["e"], spec["shape"], self.gen)
            n = spec["n"]
            self.raw[name] = dict(src=src, dst=dst, ea=[torch.rand(src.numel(), DIMS[0], generator=self.gen) for _ in range(2)])
            x = torch.randn(n, 64, generator=self.gen).to(self.device).requires_grad_(True)
            self.g[name] = dict(x=x, target=(0.3 * torch.randn(n, 64, generator=self.gen)).to(self.device), keep=None, ei=None, ea=[None, None],
                                generation=0)
        self.graph, self.attr, self.conv = graphs[0], 0, 0
        self.rethin()

    # -- kinks ------------------------------------------------------------------------------------------------------------
    def _param_sets(self):
        sets = []
        for conv in self.convs:
            lin = linears(conv)
            sets.append(([l.weight.detach().cpu() for l in lin], [l.bias.detach().cpu() for l in lin]))
        return sets + list(self.extra_params)

    def rethin(self, names=None):
        """Remove the edges on a ReLU kink under the CURRENT parameters of both modules, for both attribute tensors.  The device
        tensors of a graph are replaced only when its surviving edge set changed."""
        sets = self._param_sets()
        for name in (names or list(self.g)):
            raw, cur = self.raw[name], self.g[name]
            keep = torch.ones(raw["src"].numel(), dtype=torch.bool)
            for W, B in sets:
                for ea in raw["ea"]:
                    keep &= edges_off_the_kink(ea, W, B)
            if cur["keep"] is not None and torch.equal(keep, cur["keep"]):
                continue
            cur["keep"] = keep
            cur["ei"] = torch.stack([raw["src"][keep], raw["dst"][keep]]).to(self.device)
            cur["ea"] = [ea[keep].to(self.device) for ea in raw["ea"]]
            cur["generation"] += 1

    def current(self):
        return self.conv, self.graph, self.attr

    def full_h_bytes(self, name="dense") -> int:
        """Bytes of the whole H of a graph BEFORE the kink removal: an upper bound that every thinned version fits."""
        return int(self.raw[name]["src"].numel()) * ops.hidden_width(DIMS) * 4


class _Oracle(torch.nn.Module):
    forward = CompositeConv.forward


def oracle_of(conv, dtype, device, need_grad=False):
    """The composite on private copies of `conv`'s current parameter values in `dtype` on `device` (copies: nothing of the module
    under test stays referenced, so its memory can be freed and recycled)."""
    def own(p):
        return torch.nn.Parameter(p.detach().to(device=device, dtype=dtype, copy=True), requires_grad=need_grad)
    o = _Oracle()
    o.in_channels, o.out_channels, o.aggr = conv.in_channels, conv.out_channels, conv.aggr
    layers = []
    for l in conv.nn:
        if isinstance(l, torch.nn.Linear):
            nl = torch.nn.Linear(1, 1)
            nl.weight, nl.bias = own(l.weight), own(l.bias)
            layers.append(nl)
        else:
            layers.append(torch.nn.ReLU())
    o.nn = torch.nn.Sequential(*layers)
    o.root, o.bias = own(conv.root), own(conv.bias)
    return o


def _apply(plan, G, xs, call, masks=None):
    """The applications of `plan` = [(module index, graph name, attribute index)]: every graph carries its own running feature
    tensor from xs[graph], a ReLU stands between two applications on one graph, the loss is the sum over the graphs of the MSE of
    the last output to the graph's target.  Returns (loss, [(input, output, ReLU mask or None)])."""
    h = dict(xs)
    left = collections.Counter(g for _, g, _ in plan)
    rec, loss = [], None
    for i, (c, g, a) in enumerate(plan):
        xin = h[g]
        y = call(i, c, xin, g, a)
        left[g] -= 1
        m = None
        if left[g]:
            m = (y.detach() > 0) if masks is None else masks[i]
            if masks is not None and y.dtype == torch.float64:
                # the borrowed mask may differ from the float64 chain's own only at entries within rounding of 0: the run under
                # test is within TOL_FWD (relative L2) of float64 per application, so after i + 1 applications no entry of its
                # output is further than (i + 1) TOL_FWD |y|_2 from this one - an entry larger than that has ONE sign
                own = y.detach() > 0
                flipped = own != m.to(own.device)
                tol = (i + 1) * TOL_FWD * float(y.detach().norm())
                assert not bool(flipped.any()) or float(y.detach().abs()[flipped].max()) <= tol, \
                    f"the ReLU mask of application {i} differs from float64's at an entry of size " \
                    f"{float(y.detach().abs()[flipped].max()):.2e} (rounding allows {tol:.2e})"
            h[g] = torch.relu(y) if masks is None else y * m.to(device=y.device, dtype=y.dtype)
        else:
            term = F.mse_loss(y, G[g]["target"].to(device=y.device, dtype=y.dtype))
            loss = term if loss is None else loss + term
        rec.append((xin, y, m))
    return loss, rec


class Checker:
    """Executes operations on a world and holds every call to the bars.  `worst_fwd` / `worst_bwd`: the largest error seen (as a
    fraction of nothing - plain relative L2 against float64); `stale`: stale opportunities whose next call was checked; `raised`:
    calls that ended in a named cause instead of a number."""

    def __init__(self, world: World, theme: str = ""):
        self.w, self.theme = world, theme
        self.done = []
        self.worst_fwd = self.worst_bwd = 0.0
        self.n_calls = self.n_grads = self.stale = 0
        self.pending_stale = self.pending_pack = False
        self.stale_pack = 0
        self.raised, self.collisions = [], []
        self._stack = contextlib.ExitStack()
        self._oom = {}
        self.visited = collections.Counter()
        self.stats_before_clear = collections.Counter()
        self.regimes = [theme if theme in KNOBS and theme != "shifting" else "h_fits"]
        self.partial_hn_seen = 0

    # -- bookkeeping ------------------------------------------------------------------------------------------------------
    def literal(self) -> str:
        return repr({"theme": self.theme, "seed": self.w.seed, "ops": [(o.name,) + o.args for o in self.done]})

    def close(self):
        self._stack.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def run(self, op: Op):
        self.done.append(op)
        live = op.name in MUTATIONS and self.entry_live(self.w.convs[self.w.conv])
        packed = op.name in MUTATIONS and self.pack_live(self.w.convs[self.w.conv])
        try:
            getattr(self, "op_" + op.name)(*op.args)
        except AssertionError as ex:
            raise AssertionError(f"{ex}\n  theme {self.theme!r}, seed {self.w.seed}, operation {len(self.done) - 1}: {op!r}\n"
                                 f"  history.replay({self.literal()})") from None
        except Exception as ex:                 # an exception that names no cause: reported with the history that led to it
            raise AssertionError(f"{type(ex).__name__}: {ex}\n  theme {self.theme!r}, seed {self.w.seed}, operation {len(self.done) - 1}: {op!r}\n"
                                 f"  history.replay({self.literal()})") from ex
        if live:
            self.pending_stale = True
        if packed:
            self.pending_pack = True
        self.visited[op.name] += 1

    def run_all(self, operations):
        for op in operations:
            self.run(op)
        return self

    @staticmethod
    def entry_live(conv) -> bool:
        """The module's cache entry holds a live H, W_e, training W_e node or virtual-H node."""
        ent = hidden_cache._entries.get(conv)
        if ent is None:
            return False
        return (ent.hidden is not None and ent.token is not None and ent.token.valid) or ent.we is not None or \
            (ent.twe is not None and ent.twe_token is not None and ent.twe_token.valid) or \
            (ent.dvirtual is not None and ent.dtoken is not None and ent.dtoken.valid)

    @staticmethod
    def pack_live(conv) -> bool:
        """ops.pack_mlp holds a pack made from this module's kernel-MLP weights: the one cached operand of a module whose hidden
        cache is off (GPDE_HIDDEN_CACHE=off creates no entry at all)."""
        mine = {id(l.weight) for l in linears(conv)}
        return any(r() is not None and id(r()) in mine for refs, _ in ops._pack_cache.values() for r in refs)

    def _note_entry(self):
        ent = hidden_cache._entries.get(self.w.convs[self.w.conv])
        if ent is not None and ent.hidden is not None and ent.csr is not None and 0 < ent.hn < ent.csr.n_nodes:
            self.partial_hn_seen += 1

    # -- the checked step -------------------------------------------------------------------------------------------------
    def step(self, plan, grad="full", checkpoint_at=None, between=None, sgd=False, inputs=None):
        """Run `plan` on the modules under test and compare with float64.  grad: "none" (no_grad), "abandon" (forward with autograd,
        dropped), "inputs" (torch.autograd.grad(loss, x) only), "full" (loss.backward()), "twice" (backward(retain_graph=True), then
        backward(): twice the gradients).  Returns False when the call ended in a named cause."""
        w = self.w
        G = inputs or w.g
        graphs = list(dict.fromkeys(g for _, g, _ in plan))
        convs = list(dict.fromkeys(c for c, _, _ in plan))
        need_grad = grad != "none"
        xs = {g: G[g]["x"] for g in graphs}
        for g in graphs:
            xs[g].grad = None
        for c in convs:
            for p in w.convs[c].parameters():
                p.grad = None

        def lib_call(i, c, xin, g, a):
            conv, ei, ea = w.convs[c], G[g]["ei"], G[g]["ea"][a]
            if i == checkpoint_at:
                return checkpoint(lambda t: conv(t, ei, ea), xin, use_reentrant=False)
            return conv(xin, ei, ea)

        got = {}
        try:
            with (torch.enable_grad() if need_grad else torch.no_grad()):
                loss, rec = _apply(plan, G, xs, lib_call)
            if between is not None:
                between()
            if grad in ("full", "twice"):
                if grad == "twice":
                    loss.backward(retain_graph=True)
                loss.backward()
                for g in graphs:
                    got[f"x[{g}]"] = xs[g].grad
                for c in convs:
                    for k, p in w.convs[c].named_parameters():
                        got[f"conv{c}.{k}"] = p.grad
            elif grad == "inputs":
                gx = torch.autograd.grad(loss, [xs[g] for g in graphs])
                for g, t in zip(graphs, gx):
                    got[f"x[{g}]"] = t
        except (RuntimeError, CheckpointError) as ex:
            if not named_cause(ex, self.done[-1].name if self.done else None):
                raise
            self.raised.append((len(self.done) - 1, type(ex).__name__, str(ex).splitlines()[0][:160]))
            return False
        masks = [r[2] for r in rec]
        rec = [(a.detach(), b.detach(), m) for a, b, m in rec]
        del loss
        dev = w.device
        o64 = {c: oracle_of(w.convs[c], torch.float64, dev, bool(got)) for c in convs}
        o32 = {c: oracle_of(w.convs[c], torch.float32, dev, bool(got)) for c in convs}
        # forward: every application given the fp32 input it actually received
        with torch.no_grad():
            for i, (c, g, a) in enumerate(plan):
                xin, y, _ = rec[i]
                ei, ea = G[g]["ei"].to(dev), G[g]["ea"][a].to(dev)
                ref = o64[c](xin.to(dev).double(), ei, ea.double())
                e32 = rel(o32[c](xin.to(dev), ei, ea), ref)
                err = rel(y.to(dev), ref)
                self.worst_fwd = max(self.worst_fwd, err)
                self.n_calls += 1
                assert err <= max(TOL_FWD, FACTOR * e32), \
                    f"forward of application {i} of {plan} ({grad}): {err:.2e} from float64, the float32 composite {e32:.2e}"
        if got:
            want, e32s = {}, {}
            for o, dt, out in ((o64, torch.float64, want), (o32, torch.float32, e32s)):
                oxs = {g: G[g]["x"].detach().to(dev, dt).requires_grad_(True) for g in graphs}
                l, _ = _apply(plan, G, oxs, lambda i, c, xin, g, a: o[c](xin, G[g]["ei"].to(dev), G[g]["ea"][a].to(dev, dt)), masks=masks)
                l.backward()
                for g in graphs:
                    out[f"x[{g}]"] = oxs[g].grad
                if grad != "inputs":
                    for c in convs:
                        for k, p in o[c].named_parameters():
                            out[f"conv{c}.{k}"] = p.grad
            times = 2.0 if grad == "twice" else 1.0
            for k, ref in want.items():
                ref = ref * times
                e32 = rel(e32s[k] * times, ref)
                assert got.get(k) is not None, f"no gradient for {k} ({grad}, {plan})"
                err = rel(got[k].to(dev), ref)
                self.worst_bwd = max(self.worst_bwd, err)
                self.n_grads += 1
                assert err <= max(TOL_BWD, FACTOR * e32), \
                    f"gradient {k} of {plan} ({grad}): {err:.2e} from float64, the float32 composite {e32:.2e}"
        if self.pending_stale:
            self.stale, self.pending_stale = self.stale + 1, False
        if self.pending_pack:
            self.stale_pack, self.pending_pack = self.stale_pack + 1, False
        self._note_entry()
        if sgd and grad == "full":
            with torch.no_grad():
                for c in convs:
                    for p in w.convs[c].parameters():
                        if p.grad is not None and float(p.grad.norm()) > 0:
                            p.sub_(0.05 * float(p.norm()) / float(p.grad.norm()) * p.grad)      # every tensor moves by 5 % of its norm
            w.rethin()
        return True

    def _plan(self, depth):
        return [self.w.current()] * int(depth)

    # -- calls ------------------------------------------------------------------------------------------------------------
    def op_infer(self, depth):
        self.step(self._plan(depth), grad="none")

    def op_train(self, depth, sgd):
        self.step(self._plan(depth), grad="full", sgd=bool(sgd))

    def op_input_grads_only(self, depth):
        self.step(self._plan(depth), grad="inputs")

    def op_abandon(self, depth):
        self.step(self._plan(depth), grad="abandon")

    def op_twice(self, depth):
        self.step(self._plan(depth), grad="twice")

    def op_infer_inside_train(self, depth):
        self.step(self._plan(depth), grad="full", between=lambda: self._nested(self._plan(1)))

    def op_between(self, depth, what):
        """`what` = "release_all" | "clear_caches" between a training forward and its backward."""
        self.step(self._plan(depth), grad="full", between=getattr(self, "op_" + what))

    def _nested(self, plan):
        """A checked no_grad call between a forward and its backward (no gradient exists yet that its bookkeeping could drop)."""
        self.step(plan, grad="none")

    def op_checkpointed(self, depth, at):
        self.step(self._plan(depth), grad="full", checkpoint_at=int(at))

    def op_inference_mode_call(self):
        w = self.w
        c, g, a = w.current()
        raw, conv = w.raw[g], w.convs[c]
        lin = linears(conv)
        W, B = [l.weight.detach().cpu() for l in lin], [l.bias.detach().cpu() for l in lin]
        keep = w.g[g]["keep"] & edges_off_the_kink(raw["ea"][a] * 1.5, W, B)
        with torch.inference_mode():
            ei = torch.stack([raw["src"][keep], raw["dst"][keep]]).to(w.device)
            ea = raw["ea"][a][keep].to(w.device)
            local = {g: dict(ei=ei, ea=[ea, ea], x=w.g[g]["x"].detach().clone(), target=w.g[g]["target"])}
            self.step([(c, g, 0)] * 2, grad="none", inputs=local)
            ea.mul_(1.5)                        # an inference tensor: no version counter moves (ops._content_hash decides)
            self.step([(c, g, 0)] * 2, grad="none", inputs=local)

    def op_cpu_round_trip(self):
        w = self.w
        c, g, a = w.current()
        conv, cur = w.convs[c], w.g[g]
        conv.cpu()
        local = {g: dict(ei=cur["ei"].cpu(), ea=[t.cpu() for t in cur["ea"]], x=cur["x"].detach().cpu().requires_grad_(True), target=cur["target"].cpu())}
        try:
            self.step([(c, g, a)] * 2, grad="none", inputs=local)          # the staged path
            self.step([(c, g, a)], grad="full", inputs=local)
            with torch.no_grad():
                linears(conv)[-1].weight.mul_(1.5 if w.flip > 0 else 1 / 1.5)
                conv.root.mul_(1.5 if w.flip > 0 else 1 / 1.5)
            w.flip = -w.flip
            self.step([(c, g, a)] * 2, grad="none", inputs=local)
        finally:
            conv.to(w.device)

    def op_raise_in_forward(self):
        w = self.w
        c, g, a = w.current()
        conv, cur = w.convs[c], w.g[g]
        for ctx in (torch.no_grad(), torch.enable_grad()):
            self.step(self._plan(2), grad="none")                            # the entry holds something to damage
            try:
                with ctx:
                    conv(cur["x"][:, :32], cur["ei"], cur["ea"][a])
            except (ValueError, RuntimeError):
                pass
            else:
                raise AssertionError("a wrongly shaped x [n, 32] was accepted")
            self.step(self._plan(2), grad="full")

    def op_oom_once(self, where):
        """The next ops.<where> raises torch.OutOfMemoryError from Python (the device is never filled); the call either falls back
        and meets the bars or raises that very error; an ordinary call follows."""
        assert where in ("hidden_forward_raw", "edge_weights_raw")
        real, armed = getattr(ops, where), [True]

        def once(*a, **k):
            if armed[0]:
                armed[0] = False
                self._oom[where] = self._oom.get(where, 0) + 1
                raise torch.OutOfMemoryError(INJECTED + where)
            return real(*a, **k)
        setattr(ops, where, once)
        try:
            self.step(self._plan(2), grad="none")
            if armed[0]:
                self.step(self._plan(2), grad="full")
        finally:
            setattr(ops, where, real)
        self.step(self._plan(2), grad="full")

    # -- mutations --------------------------------------------------------------------------------------------------------
    def _amount(self):
        self.w.flip = -self.w.flip
        return self.w.flip

    def _noise(self, t):
        return (0.3 * float(t.detach().std()) * torch.randn(t.shape, generator=self.w.gen)).to(t.device)

    def op_write_param(self, which, kind):
        """A versioned in-place write under no_grad.  kind "scale": hidden layers - W_i, b_i and every later bias times 2 or
        1/2 (kink-neutral, see the module docstring), the others times 1.5 or 1/1.5; kind "noise": + 0.3 std randn."""
        conv = self.w.convs[self.w.conv]
        owner, name = param_slot(conv, which)
        p = getattr(owner, name)
        with torch.no_grad():
            if kind == "noise":
                p.add_(self._noise(p))
            elif which in HIDDEN_PARAMS:
                f = 2.0 if self._amount() > 0 else 0.5
                layer = linears(conv)[int(which[1]) - 1:]
                layer[0].weight.mul_(f)         # u_i -> f u_i exactly, and so every later pre-activation
                for l in layer:
                    l.bias.mul_(f)
            else:
                p.mul_(1.5 if self._amount() > 0 else 1 / 1.5)
        if which in HIDDEN_PARAMS:
            self.w.rethin()

    def op_write_param_data(self, which):
        """A `.data` write followed by ops.clear_caches(); hidden_cache.clear() - the documented contract."""
        conv = self.w.convs[self.w.conv]
        owner, name = param_slot(conv, which)
        p = getattr(owner, name)
        p.data.add_(self._noise(p))
        ops.clear_caches()
        self.clear_hidden_cache()
        if which in HIDDEN_PARAMS:
            self.w.rethin()

    def clear_hidden_cache(self):
        """hidden_cache.clear() zeroes its counters as well: what they had counted is carried in `stats_before_clear`."""
        for k, v in hidden_cache.stats.items():
            self.stats_before_clear[k] += v
        hidden_cache.clear()

    def recycle(self, ptr, shape, dtype, device, tries=256):
        """Same-size allocations, kept, until one returns `ptr` (the caching allocator hands a freed block to the next request of
        its size - possibly after a few others): (that tensor or None, the allocations held meanwhile)."""
        held = []
        for _ in range(tries):
            t = torch.empty(shape, dtype=dtype, device=device)
            if t.data_ptr() == ptr:
                return t, held
            held.append(t)
        return None, held

    def replace_tensor(self, old_ptr, values):
        """A NEW tensor object holding `values` (host) at version 0 - at `old_ptr` when the allocator can be made to agree."""
        gc.collect()
        dev = self.w.device
        t, held = self.recycle(old_ptr, values.shape, values.dtype, dev) if dev.type == "cuda" else (None, [])
        if t is None:
            t = torch.empty(values.shape, dtype=values.dtype, device=dev)
        del held
        t.data.copy_(values)                    # through .data: the new tensor's version counter stays 0
        return t

    def _replace_param(self, conv, which, values):
        owner, name = param_slot(conv, which)
        old = getattr(owner, name)
        ptr, ver = old.data_ptr(), old._version
        setattr(owner, name, None)
        del old
        t = self.replace_tensor(ptr, values)
        p = torch.nn.Parameter(t)
        with torch.no_grad():
            while p._version < ver:
                p.mul_(1.0)                     # versioned no-ops: the counter catches up with the replaced parameter's
        setattr(owner, name, p)
        hit = (p.data_ptr() == ptr, p._version == ver)
        self.collisions.append((which,) + hit)
        return all(hit)

    def op_replace_param(self, which):
        """A new Parameter object with other values; the old one is dropped and same-size allocations are made until one returns
        its address.  Whether data_ptr and _version collided is recorded in `collisions`."""
        conv = self.w.convs[self.w.conv]
        owner, name = param_slot(conv, which)
        old = getattr(owner, name).detach().cpu()
        values = old + 0.3 * float(old.std()) * torch.randn(old.shape, generator=self.w.gen)
        del owner
        self._replace_param(conv, which, values)
        if which in HIDDEN_PARAMS:
            self.w.rethin()

    def op_replace_mlp(self):
        conv = self.w.convs[self.w.conv]
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(torch.randint(0, 1 << 30, (1,), generator=self.w.gen)))
            new = kernel_mlp()
        conv.nn = None
        gc.collect()
        conv.nn = new.to(self.w.device)
        self.w.rethin()

    def op_write_attr(self):
        w = self.w
        _, g, a = w.current()
        f = 1.5 if self._amount() > 0 else 1 / 1.5
        w.raw[g]["ea"][a].mul_(f)
        w.g[g]["ea"][a].mul_(f)                 # versioned; the host master takes the same fp32 product
        w.rethin([g])

    def op_new_attr(self):
        """A new edge_attr tensor; the old one is dropped and its address recycled when the allocator agrees."""
        w = self.w
        _, g, a = w.current()
        cur = w.g[g]
        w.raw[g]["ea"][a] = torch.rand(w.raw[g]["src"].numel(), DIMS[0], generator=w.gen)
        ptr = cur["ea"][a].data_ptr()
        cur["ea"][a] = None
        cur["keep"] = None                      # the device tensors of this graph are rebuilt
        gc.collect()
        w.rethin([g])
        self.collisions.append(("edge_attr", cur["ea"][a].data_ptr() == ptr, True))

    # -- the rest ---------------------------------------------------------------------------------------------------------
    def op_switch_graph(self, name):
        if name in self.w.g:
            self.w.graph = name

    def op_switch_attr(self):
        self.w.attr = 1 - self.w.attr

    def op_other_module(self):
        self.w.conv = (self.w.conv + 1) % len(self.w.convs)

    def op_release_all(self):
        hidden_cache.release_all()

    def op_clear_caches(self):
        ops.clear_caches()

    def _set(self, mod, name, value):
        old = getattr(mod, name)
        self._stack.callback(setattr, mod, name, old)
        setattr(mod, name, value)

    def op_set_budget(self, how):
        full = self.w.full_h_bytes("dense") if "dense" in self.w.raw else 1 << 30
        self._set(hidden_cache, "BUDGET_BYTES", {"full": full, "half": full // 2, "none": 0}[how])

    def op_regime(self, theme):
        """The knobs of another theme and its first graph: theme "shifting" walks from regime to regime."""
        for op in KNOBS[theme]:
            getattr(self, "op_" + op.name)(*op.args)
        self.op_switch_graph(THEME_GRAPHS[theme][0])
        self.regimes.append(theme)

    def op_set_mode(self, name, value):
        mod = {"MODE": hidden_cache, "WE_MODE": hidden_cache, "DEFER_MODE": hidden_cache, "SAVE_H_MIN_EDGES": ops, "SAVE_H_BYTES": ops}[name]
        self._set(mod, name, value)


# ----------------------------------------------------------------------------------------------------------------------------
# generator
# ----------------------------------------------------------------------------------------------------------------------------
KNOBS = {
    "h_fits": [Op("set_mode", "MODE", "auto"), Op("set_mode", "WE_MODE", "off"), Op("set_mode", "DEFER_MODE", "auto"), Op("set_budget", "full")],
    "h_half": [Op("set_mode", "MODE", "auto"), Op("set_mode", "WE_MODE", "off"), Op("set_mode", "DEFER_MODE", "auto"), Op("set_budget", "half")],
    "h_none": [Op("set_mode", "MODE", "auto"), Op("set_mode", "WE_MODE", "off"), Op("set_mode", "DEFER_MODE", "auto"), Op("set_budget", "none")],
    "kept": [Op("set_mode", "MODE", "off"), Op("set_mode", "SAVE_H_MIN_EDGES", 0)],
    "we": [Op("set_mode", "MODE", "auto"), Op("set_mode", "WE_MODE", "auto"), Op("set_mode", "DEFER_MODE", "auto"), Op("set_budget", "full"),
           Op("switch_graph", "low")],
    "shifting": [Op("set_mode", "MODE", "auto"), Op("set_mode", "WE_MODE", "auto"), Op("set_mode", "DEFER_MODE", "auto"), Op("set_budget", "full")],
}
THEME_GRAPHS = {"h_fits": ("dense",), "h_half": ("dense",), "h_none": ("dense",), "kept": ("dense",), "we": ("low", "small"),
                "shifting": ("dense", "low", "small")}
# what leaves something LIVE in the entry (an inference H / W_e, an H node or a virtual-H node whose backward never ran) ...
_LEAVES_LIVE = (("infer", 3), ("abandon", 2), ("input_grads_only", 2))
_LEAVES_LIVE_THEME = {"h_none": (("abandon", 1), ("input_grads_only", 1))}       # (no H without a budget: only a virtual-H node can be live)
# ... for the mutation that follows; (name, weight)
_MUTATE = (("write_param", 5), ("replace_param", 2), ("write_param_data", 1), ("replace_mlp", 1), ("write_attr", 1), ("new_attr", 1))
_CALL = (("train", 7), ("infer", 3), ("twice", 1), ("infer_inside_train", 1), ("checkpointed", 1), ("between", 1), ("input_grads_only", 1),
         ("abandon", 1), ("inference_mode_call", 1), ("cpu_round_trip", 1), ("oom_once", 1), ("raise_in_forward", 1))
_MOVE_SHIFTING = (("switch_attr", 1), ("other_module", 1), ("switch_graph", 4), ("release_all", 1), ("clear_caches", 1))
_MOVE = (("switch_attr", 2), ("other_module", 2), ("switch_graph", 2), ("release_all", 1), ("clear_caches", 1))


def _pick(rng, table):
    names, weights = zip(*table)
    return rng.choices(names, weights)[0]


def _draw(rng, name, theme):
    depth = rng.choice((2, 2, 3, 3, 1))
    if name == "infer":
        return Op("infer", depth)
    if name == "train":
        return Op("train", max(depth, 2) if rng.random() < 0.8 else 1, rng.random() < 0.5)
    if name in ("input_grads_only", "abandon", "twice"):
        return Op(name, max(depth, 2))
    if name == "infer_inside_train":
        return Op(name, max(depth, 2))
    if name == "checkpointed":
        d = rng.choice((2, 3))
        return Op(name, d, rng.randrange(d))
    if name == "between":
        return Op(name, 2, rng.choice(("release_all", "clear_caches")))
    if name == "oom_once":
        return Op(name, rng.choice(("hidden_forward_raw", "edge_weights_raw")))
    if name == "write_param":
        which = rng.choice(PARAMS)
        return Op(name, which, "scale" if which in HIDDEN_PARAMS and rng.random() < 0.75 else rng.choice(("scale", "noise")))
    if name in ("write_param_data", "replace_param"):
        return Op(name, rng.choice(PARAMS))
    if name == "switch_graph":
        return Op(name, rng.choice(THEME_GRAPHS[theme]))
    return Op(name)


SHIFT_EVERY = 6


def walk(theme: str, seed: int, length: int = 40):
    """A deterministic sequence of about `length` operations for a theme: its knobs first, then groups drawn with
    random.Random((theme, seed)) - a plain call; or a call that leaves something live in the entry, a mutation and the call that must
    see it (a stale opportunity); or a move (other module / attributes / graph, a release).  "shifting" also takes on the knobs and
    the graph of another theme every few operations (`regime`)."""
    assert theme in THEMES
    rng = random.Random(f"{theme}/{seed}")
    out = list(KNOBS[theme])
    out += [Op("train", 3, False), Op("train", 2, True)]       # the policy learns that the module repeats its key
    shifting = theme == "shifting"
    # "shifting" starts under the knobs of h_fits and moves on every SHIFT_EVERY operations, through the other themes in an order
    # drawn once and then repeated: 40 operations visit every regime, whatever the seed
    tour, shifted = (rng.sample(THEMES[1:-1], len(THEMES) - 2) + ["h_fits"]) if shifting else [], len(out)
    while len(out) < length:
        if shifting and len(out) - shifted >= SHIFT_EVERY:
            out.append(Op("regime", tour[0]))
            tour, shifted = tour[1:] + tour[:1], len(out)
            continue
        r = rng.random() * 0.92
        if r < 0.40:
            out.append(_draw(rng, _pick(rng, _CALL), theme))
        elif r < 0.80:
            out.append(_draw(rng, _pick(rng, _LEAVES_LIVE_THEME.get(theme, _LEAVES_LIVE)), theme))
            out.append(_draw(rng, _pick(rng, _MUTATE), theme))
            out.append(_draw(rng, rng.choice(("infer", "train", "train")), theme))
        else:
            out.append(_draw(rng, _pick(rng, _MOVE_SHIFTING if shifting else _MOVE), theme))
    return out


def parse(literal):
    """A walk literal (the string a failure prints, or the dict it evaluates to) -> (theme, seed, [Op])."""
    d = ast.literal_eval(literal) if isinstance(literal, str) else literal
    return d["theme"], int(d["seed"]), [Op(*t) for t in d["ops"]]


def replay(literal, device=None, make_conv=None, graphs=None):
    """Execute a recorded history from a fresh world; returns the Checker (closed: the knobs are restored)."""
    theme, seed, operations = parse(literal)
    device = device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    hidden_cache.clear()
    ops.clear_caches()
    world = World(seed, device, make_conv=make_conv, graphs=graphs or THEME_GRAPHS.get(theme, tuple(GRAPHS)))
    with Checker(world, theme) as ck:
        t0 = time.perf_counter()
        ck.run_all(operations)
        ck.seconds = time.perf_counter() - t0
    return ck
