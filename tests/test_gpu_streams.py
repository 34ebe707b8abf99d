"""GPU tier of the stream contract (INTEGRATION.md "Streams", DESIGN.md "Streams").

1. A call issued on stream S launches all of its device work on S.
2. What the caller passes follows PyTorch's rules; what the library cached itself (packed weights, slot-ordered attributes,
   hidden activations H, per-edge weights W_e, source orders, CSRs, GCN coefficients) the library orders: a hit from another
   stream than the builder's is queued behind the build and keeps the buffer from being recycled under the reader.

Every case computes its serial baseline on the default stream, compares it ONCE with the float64 oracle at the project's bars
(forward 1e-5, gradients 2e-5) and then demands the bits of that baseline (torch.equal) from the call on other streams: the same
kernels with the same arguments in the same summation order.

SAFETY RULE OF THIS FILE.  The racing tests let a kernel read a buffer that may not have been written yet.  That is harmless only
for numbers:
  * indices are never raced.  Every CSR, every `csr.src_order`, the identity permutation of `attr_in_slot_order` and every GCN
    structure is built first and followed by torch.cuda.synchronize(); only float buffers are raced - packed weights,
    slot-ordered attributes, H, W_e, and the inputs x / grad_out / k;
  * the poison is zero bytes (helpers/streams.zeroed_pool), never NaN or a bit pattern: zero is a wrong number but a valid index,
    so even a mistake in a test cannot send a kernel out of bounds;
  * the graph builders are excluded (helpers/streams.EXCLUDED: radius_graph, radius_csr*, build_csr / csr_for, the selection of
    the neighbour cap, multilevel_radius_graphs, and with build_csr the reversed graph of gcn_norm): they run count, read-back and
    fill passes, the fill kernels write by the counts, and racing their producers could write out of bounds;
  * no test repeats a racing call to "catch" the race: each case issues its sequence once and compares.
Every racing test asserts that its window was still open (`not held.query()`) right after its last call was issued: a hidden
host synchronisation inside a call, or a hold that was too short, fails the case instead of passing it."""
import copy
import gc

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, hidden_cache, ops
from oracle.nnconv_oracle import nnconv_forward, nnconv_grads, rel_l2
from tests.helpers import diag_oracle, gcn_oracle
from tests.helpers.kinks import edges_off_the_kink
from tests.helpers.streams import (HOLD_EVICT_MS, HOLD_MS, ISSUE_EVICT_MS_MEASURED, ISSUE_MS_MEASURED, SIDE_STREAM_TABLE, IssueTimer, hold,
                                   stream_beside, stream_pair, zeroed_pool)
from tests.test_gpu_layouts import _any_oracle
from tests.test_host_logic import DenseNet

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
TOL_FWD, TOL_BWD = 1e-5, 2e-5
DIMS = [6, 64, 128, 4096]                # the 8-wave split-f16 kernel at n = 300, e = 6000
DIMS_DEFER = [6, 256, 256, 4096]         # the depth-deferred form (ops.deferred_supported) on the same graph
N64, E64 = 300, 6000
ONE = ops._ONE_SET


def _hits(cache):
    return ops.cross_stream_hits.get(cache, 0)


def _mlp_params(dims, g):
    W = [torch.empty(dims[i + 1], dims[i]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    B = [torch.empty(dims[i + 1]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    return W, B


def _graph(n, e, g):
    """[2, e] random edges: node n - 1 without in-edges, destination 3 with 40 in-edges."""
    src, dst = torch.randint(0, n, (e,), generator=g), torch.randint(0, n - 1, (e,), generator=g)
    dst[:40] = 3
    return torch.stack([src, dst])


def _bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _flat(res):
    out = []
    for r in (res if isinstance(res, (tuple, list)) else [res]):
        out.extend(_flat(r) if isinstance(r, (tuple, list)) else [r])
    return out


def _dist(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


_C64 = {}


def _case64(dims=DIMS):
    """Host tensors, device copies, CSR (built and synchronised) and pack of the 64-wide family: n = 300, exactly e = 6000 edges
    none of whose hidden pre-activations sits on the ReLU kink (helpers/kinks.py).  Built once, never modified."""
    key = tuple(dims)
    if key in _C64:
        return _C64[key]
    g = torch.Generator().manual_seed(4321 + dims[1])
    ei, ea = _graph(N64, E64 + 600, g), torch.randn(E64 + 600, dims[0], generator=g)
    W, B = _mlp_params(dims, g)
    keep = torch.nonzero(edges_off_the_kink(ea, W, B)).view(-1)[:E64]
    ei, ea = ei[:, keep].contiguous(), ea[keep].contiguous()
    assert ei.shape[1] == E64
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(dims=dims, ei=ei, ea=ea, W=W, B=B, x=r(N64, 64), x2=r(N64, 64), g=r(N64, 64), g2=r(N64, 64), res=r(N64, 64),
             root=torch.empty(64, 64).uniform_(-0.125, 0.125, generator=g), bias=torch.empty(64).uniform_(-0.125, 0.125, generator=g))
    c["d"] = {k: c[k].to(D) for k in ("ea", "x", "x2", "g", "g2", "res", "root", "bias")}
    c["Wd"], c["Bd"] = [w.to(D) for w in W], [b.to(D) for b in B]
    c["csr"] = ops.build_csr(ei.to(D), N64)
    c["csr"].src_order
    c["csr"].rowptr_host
    torch.cuda.synchronize()
    _C64[key] = c
    return c


def _fwd64(c, x, aggr="mean"):
    return nnconv_forward(x, c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], aggr=aggr, dtype=torch.float64, chunk_edges=4096)


# ---------------------------------------------------------------------------------------------------------------------------
# 1 + 2. float caches: a hit from another stream than the builder's; eviction under a queued reader
# ---------------------------------------------------------------------------------------------------------------------------
class _PackCase:
    """pack_mlp through ops.nnconv_forward_raw with a prebuilt CSR (the 8-wave kernel)."""
    cache, hidden_mode = "pack_mlp", False

    def __init__(self):
        c = self.c = _case64()
        self.x1, self.x2 = c["d"]["x"], c["d"]["x2"]
        pm = ops.pack_mlp(c["Wd"], c["Bd"])
        assert ops.fused_kernel_name(N64, E64, pm) == "gpde_fused_f16v3_kernel"
        self.numel = pm.packed.numel()
        zero = ops.PackedMlp(pm.dims, torch.zeros_like(pm.packed), pm.dims_c)
        d = c["d"]
        self.signatures = {"an all-zero pack": ops.nnconv_forward_raw(self.x2, c["csr"], d["ea"], zero, d["root"], d["bias"], "mean")}
        self.reference = _fwd64(c, c["x2"])

    def reset(self):
        ops.clear_caches()

    def first(self):
        self.call(self.x1)

    def call(self, x, W=None, B=None):
        c, d = self.c, self.c["d"]
        pm = ops.pack_mlp(c["Wd"] if W is None else W, c["Bd"] if B is None else B)
        return ops.nnconv_forward_raw(x, c["csr"], d["ea"], pm, d["root"], d["bias"], "mean")


class _AttrCase:
    """The slot-ordered attribute copy of attr_in_slot_order: e = 33,000 (just over _ATTR_SLOT_ORDER_MIN_EDGES) on n = 2000 nodes,
    the edge list in source-major order.  The identity probe of the first call synchronises by design: it is warmed with another
    attribute tensor in front of the hold, and the pack is built and synchronised on the default stream."""
    cache, hidden_mode = "attr_slot_order", False

    def __init__(self):
        n, e = 2000, 33000
        assert e >= ops._ATTR_SLOT_ORDER_MIN_EDGES > e - 1000 and ops.ATTR_SLOT_ORDER
        g = torch.Generator().manual_seed(99)
        src, _ = torch.sort(torch.randint(0, n, (e,), generator=g))
        self.ei = torch.stack([src, torch.randint(0, n, (e,), generator=g)])
        self.ea_host = torch.randn(e, DIMS[0], generator=g)
        self.W, self.B = _mlp_params(DIMS, g)
        self.Wd, self.Bd = [w.to(D) for w in self.W], [b.to(D) for b in self.B]
        self.root, self.bias = torch.empty(64, 64).uniform_(-0.125, 0.125, generator=g), torch.empty(64).uniform_(-0.125, 0.125, generator=g)
        self.rd, self.bd = self.root.to(D), self.bias.to(D)
        self.x1, x2 = torch.randn(n, 64, generator=g).to(D), torch.randn(n, 64, generator=g)
        self.x2 = x2.to(D)
        self.csr = ops.build_csr(self.ei.to(D), n)
        self.ea = self.ea_host.to(D)
        self.pm = ops.pack_mlp(self.Wd, self.Bd)
        ops.attr_in_slot_order(self.csr, torch.zeros(e, DIMS[0], device=D))      # the identity probe, in front of every hold
        torch.cuda.synchronize()
        assert self.csr._identity is not None and not self.csr._perm_is_identity
        self.numel = e * DIMS[0]
        self.signatures = {"all-zero attributes": ops.nnconv_forward_raw(self.x2, self.csr, torch.zeros(e, DIMS[0], device=D), self.pm,
                                                                         self.rd, self.bd, "mean")}
        self.reference = nnconv_forward(x2, self.ei, self.ea_host, self.W, self.B, self.root, self.bias, aggr="mean", dtype=torch.float64,
                                        chunk_edges=4096)

    def reset(self):
        self.csr._attr_sorted.clear()

    def first(self):
        self.call(self.x1)

    def call(self, x):
        return ops.nnconv_forward_raw(x, self.csr, self.ea, self.pm, self.rd, self.bd, "mean")


class _HiddenCase:
    """H (`what` = "hidden") and W_e ("edge_weights") of hidden_cache through gp.NNConv_old, the policy forced on with the switch
    tests/test_gpu_hidden.py uses (hidden_cache.MODE = "on") on its small graph.  Inference calls: the first builds H, the second
    hits H and builds W_e from it, the third hits W_e.  The pack and the CSR are built and synchronised on the default stream."""
    hidden_mode = True

    def __init__(self, what):
        from graph_pde_amd import synth
        self.cache, self.n_first = what, (1 if what == "hidden" else 2)
        torch.manual_seed(17)
        self.ei_host, self.ea_host, n = synth.darcy_graph(12, 0.2)
        self.conv = gp.NNConv_old(64, 64, DenseNet(DIMS, torch.nn.ReLU), aggr="mean").to(D)
        lin = ops.mlp_linears(self.conv.nn)
        self.W, self.B = [l.weight.detach().cpu() for l in lin], [l.bias.detach().cpu() for l in lin]
        self.ei, self.ea = self.ei_host.to(D), self.ea_host.to(D)
        g = torch.Generator().manual_seed(5)
        xs = [torch.randn(n, 64, generator=g) for _ in range(3)]
        self.x1, self.x1b, self.x2 = (t.to(D) for t in xs)
        self.reference = nnconv_forward(xs[2], self.ei_host, self.ea_host, self.W, self.B, self.conv.root.detach().cpu(),
                                        self.conv.bias.detach().cpu(), aggr="mean", dtype=torch.float64)
        # the serial sequence once, to read the entry's sizes and the zero signatures off it
        hidden_cache.clear()
        with torch.no_grad():
            for x in (self.x1, self.x1b):
                self.conv(x, self.ei, self.ea)
        ent = hidden_cache._entries[self.conv]
        assert ent.hidden is not None and ent.we is not None, "the policy did not build H and W_e on this graph"
        self.numel = ent.hidden.numel() if what == "hidden" else ent.we.numel()
        csr = ops.csr_for(self.ei, n)
        pm = ops.pack_mlp([l.weight for l in lin], [l.bias for l in lin])
        root, bias = self.conv.root.detach(), self.conv.bias.detach()
        we0 = ops.edge_weights_raw(torch.zeros_like(ent.hidden), pm, lin[-1].weight.detach(), lin[-1].bias.detach())
        self.signatures = {"W_e built from an all-zero H": ops.nnconv_forward_edgeweights_raw(self.x2, csr, we0, root, bias, "mean"),
                           "an all-zero W_e": ops.nnconv_forward_edgeweights_raw(self.x2, csr, torch.zeros_like(ent.we), root, bias, "mean")}
        torch.cuda.synchronize()

    def reset(self):
        hidden_cache.release_all()
        hidden_cache.clear()
        # the CSR (indices: never raced, and pinned here so that no eviction frees them under a queued kernel) and the pack are
        # built on the default stream and complete before any hold
        lin = ops.mlp_linears(self.conv.nn)
        self.pin = (ops.csr_for(self.ei, self.x1.size(0)), ops.pack_mlp([l.weight for l in lin], [l.bias for l in lin]))
        torch.cuda.synchronize()

    def first(self):
        for x in (self.x1, self.x1b)[:self.n_first]:
            self.call(x)

    def call(self, x):
        with torch.no_grad():
            return self.conv(x, self.ei, self.ea)


class _GcnCase:
    """The float coefficients of ops.gcn_norm on a prebuilt, synchronised CSR (`module` False), and the same normalisation pinned
    by gp.GCNConv(cached=True), which later calls take from the module without a look-up (`module` True)."""
    cache, hidden_mode = "gcn_norm", False

    def __init__(self, module):
        c = self.c = _case64()
        g = torch.Generator().manual_seed(23)
        x1, x2, ew = torch.randn(N64, 16, generator=g), torch.randn(N64, 16, generator=g), torch.rand(E64, generator=g) + 0.5
        self.x1, self.x2, self.ew, self.ei = x1.to(D), x2.to(D), ew.to(D), c["ei"].to(D)
        self.module = module
        torch.manual_seed(29)
        self.conv = gp.GCNConv(16, 24, cached=module).to(D)
        with torch.no_grad():
            self.conv.bias.uniform_(-0.5, 0.5)
        self.w, self.b = self.conv.weight.detach(), self.conv.bias.detach()
        self.reset()
        zero = ops.GcnNorm(self.csr, torch.zeros(E64, device=D), torch.zeros(N64, device=D), ops.gcn_flags())
        self.signatures = {"all-zero coefficients": ops.gcn_forward_raw(self.x2, zero, self.w, self.b)}
        self.reference = gcn_oracle.forward(x2, c["ei"], self.w.cpu(), self.b.cpu(), edge_weight=ew)

    def reset(self):
        self.conv._cached_device = None
        ops._gcn_norm_cache.clear()
        # the graph (indices: never raced, pinned here) is built and complete on the default stream before any hold
        self.csr = ops.csr_for(self.ei, N64) if self.module else self.c["csr"]
        torch.cuda.synchronize()

    def first(self):
        self.call(self.x1)

    def call(self, x):
        if self.module:
            with torch.no_grad():
                return self.conv(x, self.ei, self.ew)
        return ops.gcn_forward_raw(x, ops.gcn_norm(self.csr, self.ew), self.w, self.b)


_FLOAT_CASES = {}


def _float_case(name, monkeypatch):
    if name in ("hidden", "edge_weights"):
        monkeypatch.setattr(hidden_cache, "MODE", "on")
    if name not in _FLOAT_CASES:
        if name in ("gcn_norm", "gcn_cached"):
            case = _GcnCase(name == "gcn_cached")
        else:
            case = {"pack_mlp": _PackCase, "attr_slot_order": _AttrCase}[name]() if name in ("pack_mlp", "attr_slot_order") else _HiddenCase(name)
        # the serial baseline on the default stream, compared once with float64
        case.reset()
        torch.cuda.synchronize()
        case.first()
        case.baseline = case.call(case.x2)
        torch.cuda.synchronize()
        err = rel_l2(case.baseline.cpu(), case.reference)
        print(f"{name}: serial baseline vs float64 {err:.3e}")
        assert err <= TOL_FWD, err
        _FLOAT_CASES[name] = case
    return _FLOAT_CASES[name]


def _report(name, got, case):
    figs = {"baseline": _dist(got, case.baseline)}
    figs.update({k: _dist(got, v) for k, v in case.signatures.items()})
    print(f"{name}: relative distance of the second stream's result from " + ", ".join(f"{k}: {v:.3e}" for k, v in figs.items()))


@pytest.mark.parametrize("name", ["pack_mlp", "attr_slot_order", "hidden", "edge_weights", "gcn_norm", "gcn_cached"])
def test_cross_stream_hit_on_a_float_cache(name, monkeypatch):
    """Stream A builds the entry behind a hold; stream B, which has waited for nothing of A, hits it at once with another x.
    Without the library's ordering B reads the entry before A wrote it: the zero signature printed below."""
    case = _float_case(name, monkeypatch)
    case.reset()
    A, B = stream_pair()
    zeroed_pool(A, also=(B,))
    before = getattr(ops, "cross_stream_hits", {}).get(case.cache, 0)
    held = hold(A)
    with IssueTimer() as t:
        with torch.cuda.stream(A):
            case.first()
        with torch.cuda.stream(B):
            got = case.call(case.x2)
    window_open = not held.query()
    torch.cuda.synchronize()
    print(f"{name}: issuing the racing sequence took {t.ms:.2f} ms of host time (hold {HOLD_MS:.0f} ms)")
    _report(name, got, case)
    assert window_open, "the hold ended before the racing call was issued: a host synchronisation inside the call, or too short a hold"
    assert HOLD_MS >= 10 * ISSUE_MS_MEASURED
    assert _bits(got, case.baseline), "the second stream read the cached buffer before its builder had written it"
    assert _hits(case.cache) == before + 1, ops.cross_stream_hits
    with torch.cuda.stream(B):
        again = case.call(case.x2)
    torch.cuda.synchronize()
    assert _hits(case.cache) == before + 1, ops.cross_stream_hits  # a stream that has waited for an entry does not wait again
    assert _bits(again, case.baseline)


@pytest.mark.parametrize("name", ["pack_mlp", "pack_mlp_replaced", "hidden", "edge_weights"])
def test_eviction_under_a_queued_reader(name, monkeypatch):
    """The entry is built on A and complete.  B hits it and queues behind a hold; then every way of dropping it runs on A, whose
    allocator pool the block returns to, and A allocates and zeroes blocks of the entry's size.  Without `record_stream` on the
    hitting stream B's kernel reads the recycled, zeroed block.  `pack_mlp_replaced`: the entry is replaced by the pack of a second
    parameter set at the same addresses (new tensor objects over the same memory - not an in-place update of weights the queued
    call still owns, which would be the caller's own race)."""
    case = _float_case("pack_mlp" if name == "pack_mlp_replaced" else name, monkeypatch)
    case.reset()
    A, B = stream_pair()
    n_blocks = 4
    with torch.cuda.stream(A):
        case.first()
        # (A's allocator pool already holds n_blocks free blocks of the entry's size: with the entry's own block the n_blocks + 1
        # allocations under the hold are all served from the pool, none from the driver)
        warm = [torch.zeros(case.numel, dtype=torch.float32, device=D) for _ in range(n_blocks + (name == "pack_mlp_replaced"))]
        del warm
    with torch.cuda.stream(B):                                    # (B's pool too)
        warm = [torch.zeros(64 << 20, dtype=torch.uint8, device=D)] + [torch.zeros(256 << 10, dtype=torch.uint8, device=D) for _ in range(16)]
        del warm
    gc.collect()
    torch.cuda.synchronize()
    before = getattr(ops, "cross_stream_hits", {}).get(case.cache, 0)
    held = hold(B, HOLD_EVICT_MS)
    with IssueTimer() as t:
        with torch.cuda.stream(B):
            got = case.call(case.x2)
        with torch.cuda.stream(A):
            if name == "pack_mlp_replaced":
                W2, B2 = [w.detach() for w in case.c["Wd"]], [b.detach() for b in case.c["Bd"]]
                other = case.call(case.x1, W2, B2)
            else:
                ops.clear_caches()
                hidden_cache.release_all()
                hidden_cache.clear()
            gc.collect()
            blocks = [torch.zeros(case.numel, dtype=torch.float32, device=D) for _ in range(n_blocks + 1)]
    window_open = not held.query()
    torch.cuda.synchronize()
    print(f"{name}: issuing took {t.ms:.2f} ms of host time (hold {HOLD_EVICT_MS:.0f} ms)")
    _report(name, got, case)
    del blocks
    assert window_open, "the hold ended before the eviction was issued"
    assert HOLD_EVICT_MS >= 10 * ISSUE_EVICT_MS_MEASURED
    assert _bits(got, case.baseline), "the cached buffer was recycled while a queued kernel of another stream still read it"
    assert _hits(case.cache) == before + 1 or name != "pack_mlp_replaced", ops.cross_stream_hits     # (clear_caches() resets the counters)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. integer caches: bookkeeping only, never raced
# ---------------------------------------------------------------------------------------------------------------------------
def test_integer_caches_count_cross_stream_hits_and_are_never_raced():
    c = _case64()
    d = c["d"]
    A, B = torch.cuda.Stream(), torch.cuda.Stream()          # (nothing is raced here: any two streams)
    ops.clear_caches()

    # csr.src_order: built on A, complete, then read by a backward on B
    def bwd(csr):
        return _flat(ops.nnconv_backward_raw(d["x"], csr, d["ea"], c["Wd"], c["Bd"], d["root"], "mean", d["g"]))
    base = bwd(c["csr"])
    torch.cuda.synchronize()
    rx, rW, rb, rroot, rbias = nnconv_grads(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], "mean", c["g"], chunk_edges=4096)
    errs = {k: rel_l2(a.cpu(), b) for k, a, b in zip(["dx", "dW0", "dW1", "dW2", "db0", "db1", "db2", "droot", "dbias"], base,
                                                     [rx] + rW + rb + [rroot, rbias])}
    print("backward baseline vs float64", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= TOL_BWD for v in errs.values()), errs
    csr2 = ops.build_csr(c["ei"].to(D), N64)
    with torch.cuda.stream(A):
        csr2.src_order
    csr2.rowptr_host
    torch.cuda.synchronize()
    before = _hits("src_order")
    with torch.cuda.stream(B):
        got = bwd(csr2)
    torch.cuda.synchronize()
    assert _hits("src_order") == before + 1, ops.cross_stream_hits
    assert all(_bits(a, b) for a, b in zip(got, base))

    # the CSR cache: the entry's builder synchronises (it reads the bad-edge count back) - a hit is kept alive, not waited for
    ei_d = c["ei"].to(D)
    pm = ops.pack_mlp(c["Wd"], c["Bd"])
    y0 = ops.nnconv_forward_raw(d["x"], c["csr"], d["ea"], pm, d["root"], d["bias"], "mean")
    torch.cuda.synchronize()
    assert rel_l2(y0.cpu(), _fwd64(c, c["x"])) <= TOL_FWD
    with torch.cuda.stream(A):
        built = ops.csr_for(ei_d, N64)
    torch.cuda.synchronize()
    before = _hits("csr")
    with torch.cuda.stream(B):
        hit = ops.csr_for(ei_d, N64)
        y = ops.nnconv_forward_raw(d["x"], hit, d["ea"], ops.pack_mlp(c["Wd"], c["Bd"]), d["root"], d["bias"], "mean")
    torch.cuda.synchronize()
    assert hit is built and _hits("csr") == before + 1 and _bits(y, y0), ops.cross_stream_hits

    # the GCN normalisation and its reversed graph
    g = torch.Generator().manual_seed(8)
    x, w, ew = torch.randn(N64, 16, generator=g), torch.randn(16, 24, generator=g) / 4, torch.rand(E64, generator=g) + 0.5
    xd, wd, ewd = x.to(D), w.to(D), ew.to(D)
    norm0 = ops.gcn_norm(c["csr"], ewd)
    y0, r0 = ops.gcn_forward_raw(xd, norm0, wd), ops.gcn_forward_raw(xd, norm0, None, reverse=True)
    torch.cuda.synchronize()
    err = gcn_oracle.rel_l2(y0, gcn_oracle.forward(x, c["ei"], w, edge_weight=ew))
    assert err <= TOL_FWD, err
    ops.clear_caches()
    with torch.cuda.stream(A):
        norm = ops.gcn_norm(c["csr"], ewd)
        norm.reversed
    torch.cuda.synchronize()
    with torch.cuda.stream(B):
        hit = ops.gcn_norm(c["csr"], ewd)
        y, r = ops.gcn_forward_raw(xd, hit, wd), ops.gcn_forward_raw(xd, hit, None, reverse=True)
    torch.cuda.synchronize()
    assert hit is norm and _hits("gcn_norm") == 2, ops.cross_stream_hits          # the coefficients and the reversed pair
    assert _bits(y, y0) and _bits(r, r0)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. every entry point on a side stream
# ---------------------------------------------------------------------------------------------------------------------------
def _chain64(c):
    """The intermediate tensors of the 64-wide family that downstream entry points take as inputs (built once, default stream)."""
    if "chain" in c:
        return c["chain"]
    d, csr = c["d"], c["csr"]
    pm = ops.pack_mlp(c["Wd"], c["Bd"])
    hw, hb = c["Wd"][:-1] + [None], c["Bd"][:-1] + [None]
    H, hmax = ops.hidden_forward_raw(csr, d["ea"], pm, hw, hb)
    hn = 128
    Hp, hpmax = ops.hidden_forward_raw(csr, d["ea"], pm, hw, hb, n_nodes_limit=hn)
    H32, _ = ops.hidden_forward_raw(csr, d["ea"], pm, hw, hb, "f32")
    we = ops.edge_weights_raw(H32, pm, c["Wd"][-1], c["Bd"][-1])
    grad_h = ops.nnconv_backward_hidden_raw(d["x"], csr, H, c["dims"], c["Wd"][-1], c["Bd"][-1], d["root"], "mean", d["g"])[1]
    gwe = ops.nnconv_backward_edgeweights_raw(d["x"], csr, we, d["root"], "mean", d["g"])[1]
    table = torch.randn(N64, 3, generator=torch.Generator().manual_seed(3)).to(D)
    torch.cuda.synchronize()
    c["chain"] = dict(pm=pm, H=H, hmax=hmax, hn=hn, Hp=Hp, hpmax=hpmax, H32=H32, we=we, grad_h=grad_h, gwe=gwe, table=table)
    return c["chain"]


_ORACLE64 = {}


def _oracle64(dims=DIMS, forward=True):
    """float64 of the 64-wide family by output name (forward: y*, H; everything starting with d: a gradient)."""
    key = tuple(dims)
    if key in _ORACLE64:
        return _ORACLE64[key]
    c = _case64(dims)
    o = {}
    if forward:
        o = {"y": _fwd64(c, c["x"]), "y_add": _fwd64(c, c["x"], "add"), "y_max": _fwd64(c, c["x"], "max")}
        o["y_act"] = torch.relu(c["res"].double() + o["y"])
    rx, rW, rb, rroot, rbias = nnconv_grads(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], "mean", c["g"], chunk_edges=4096)
    o.update(dx=rx, droot=rroot, dbias=rbias, dW_last=rW[-1], db_last=rb[-1])
    _, rW2, rb2, _, _ = nnconv_grads(c["x2"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], "mean", c["g2"], chunk_edges=4096)
    for l in range(len(rW)):
        o[f"dW{l}"], o[f"db{l}"] = rW[l], rb[l]
        o[f"dW{l}_two"], o[f"db{l}_two"] = rW[l] + rW2[l], rb[l] + rb2[l]
    if forward:
        h = c["ea"].double()
        for l in range(len(c["W"]) - 1):
            h = torch.relu(torch.nn.functional.linear(h, c["W"][l].double(), c["B"][l].double()))
        o["H"] = h[c["csr"].perm.cpu().long()]
        o["hmax"] = o["H"].abs().max().reshape(1)
        # per CSR slot: W_e = H W_last^T + b_last; of sum(out * g) under 'mean': dL/dW_e = x_j (x) g_i / deg_i, dL/dH = dL/dW_e W_last
        w_last, b_last = c["W"][-1].double(), c["B"][-1].double()
        o["We"] = o["H"] @ w_last.t() + b_last
        src, dst = c["csr"].edge_index.cpu()
        deg = torch.bincount(dst, minlength=N64).clamp(min=1).double()
        gbar = c["g"].double()[dst] / deg[dst].unsqueeze(1)
        o["dWe"] = (c["x"].double()[src].unsqueeze(2) * gbar.unsqueeze(1)).reshape(E64, -1)
        # (the backward hands back dL/dU of the last hidden layer: dL/dH already masked by H > 0, as its wrappers state)
        o["dU"] = (o["dWe"] @ w_last) * (o["H"] > 0)
    _ORACLE64[key] = o
    return o


def _any(cin, cout, n_src=None, cind=None, k=24):
    """The any-width operands of tests/test_gpu_layouts._any_case, with a destination table of its own width (`cind`)."""
    n, e = 70, 300
    g = torch.Generator().manual_seed(cin * 1000 + cout + (n_src or 0))
    ns, cd = (n if n_src is None else n_src), (cin if cind is None else cind)
    src, dst = torch.randint(0, ns, (e,), generator=g), torch.randint(0, n - 1, (e,), generator=g)
    dst[:40] = 3
    csr = ops.build_csr(torch.stack([src, dst]).to(D), n, n_src=n_src)
    csr.src_order
    t = lambda *s: torch.randn(*s, generator=g)
    a = dict(n=n, ns=ns, e=e, cin=cin, cout=cout, csr=csr, ei=csr.edge_index.cpu(), x=t(ns, cin), xd=t(n, cd), we=t(e, cin * cout) / cin ** 0.5,
             root=t(cd, cout) / 4, bias=t(cout), res=t(n, cout), g=t(n, cout), hidden=torch.relu(t(e, k)), w_last=t(cin * cout, k) / k ** 0.5,
             b_last=t(cin * cout) / 4, k=t(e, cin) / 2)
    a["d"] = {key: v.to(D) for key, v in a.items() if torch.is_tensor(v) and v.dtype == torch.float32}
    torch.cuda.synchronize()
    return a


def _entries():
    """name -> (float inputs staged behind the side stream's hold, call(**inputs) -> {output name: tensor}, oracle {name: float64}).
    An output whose name the oracle holds is compared with it once, on the baseline (names starting with "d": gradients, 2e-5;
    the others 1e-5); every output is compared bit for bit with the baseline after the side-stream call."""
    c, cd = _case64(), _case64(DIMS_DEFER)
    d, csr, ch, o = c["d"], c["csr"], _chain64(c), _oracle64()
    pm, Wd, Bd, root, bias, dims = ch["pm"], c["Wd"], c["Bd"], d["root"], d["bias"], c["dims"]
    nl = len(Wd)
    T = {}

    def grads_full(r):
        gx, gW, gb, groot, gbias = r
        out = dict(dx=gx, droot=groot, dbias=gbias)
        out.update({f"dW{l}": w for l, w in enumerate(gW)})
        out.update({f"db{l}": b for l, b in enumerate(gb)})
        return out

    T["nnconv_forward_raw"] = (dict(x=d["x"], ea=d["ea"], res=d["res"]), lambda x, ea, res: dict(
        y=ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "mean"),
        y_act=ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "mean", residual=res, relu=True)), o)
    T["nnconv_forward_raw[f32]"] = (dict(x=d["x"], ea=d["ea"]), lambda x, ea: dict(
        y=ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "mean", precision="f32")), o)
    assert ops.fused_kernel_name(N64, E64, pm, "f32") == "gpde_fused_kernel"
    sel = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
    ea_na = ops.NodeAttr(ch["table"], sel).materialize(csr.edge_index).cpu()
    o_na = {"y": nnconv_forward(c["x"], csr.edge_index.cpu(), ea_na, c["W"], c["B"], c["root"], c["bias"], aggr="mean", dtype=torch.float64)}
    T["nnconv_forward_nodeattr_raw"] = (dict(x=d["x"], table=ch["table"]), lambda x, table: dict(
        y=ops.nnconv_forward_nodeattr_raw(x, csr, ops.NodeAttr(table, sel), pm, root, bias, "mean")), o_na)
    T["nnconv_forward_per_edge_raw"] = (dict(x=d["x"], ea=d["ea"]), lambda x, ea: dict(
        y=ops.nnconv_forward_per_edge_raw(x, csr, ea, pm, Wd, Bd, root, bias, "mean")), o)
    T["nnconv_backward_raw"] = (dict(x=d["x"], ea=d["ea"], g=d["g"]), lambda x, ea, g: grads_full(
        ops.nnconv_backward_raw(x, csr, ea, Wd, Bd, root, "mean", g)), o)
    # light + deferred backward of a depth-shared module: the deferred form needs its own kernel-MLP widths
    dd, csr_d, od = cd["d"], cd["csr"], _oracle64(DIMS_DEFER, forward=False)
    assert ops.deferred_supported(DIMS_DEFER)

    def light(x, ea, g):
        gx, gw, gb, groot, gbias = ops.nnconv_backward_light_raw(x, csr_d, ea, cd["Wd"], cd["Bd"], dd["root"], "mean", g)
        return dict(dx=gx, dW_last=gw, db_last=gb, droot=groot, dbias=gbias)

    def deferred(x, x2, ea, g, g2):
        r = _flat(ops.nnconv_backward_deferred_raw([x, x2], [g, g2], csr_d, ea, cd["Wd"], cd["Bd"], "mean"))
        out = {f"dW{l}_two": r[l] for l in range(nl - 1)}
        out.update({f"db{l}_two": r[nl - 1 + l] for l in range(nl - 1)})
        return out
    T["nnconv_backward_light_raw"] = (dict(x=dd["x"], ea=dd["ea"], g=dd["g"]), light, od)
    T["nnconv_backward_deferred_raw"] = (dict(x=dd["x"], x2=dd["x2"], ea=dd["ea"], g=dd["g"], g2=dd["g2"]), deferred, od)

    def hidden_fwd(ea):
        h, hmax = ops.hidden_forward_raw(csr, ea, pm, Wd[:-1] + [None], Bd[:-1] + [None])
        return dict(H=h[:, :dims[-2]], H_pad=h, hmax=hmax)
    T["hidden_forward_raw"] = (dict(ea=d["ea"]), hidden_fwd, o)
    T["nnconv_forward_hidden_raw"] = (dict(x=d["x"], hidden=ch["H"], res=d["res"]), lambda x, hidden, res: dict(
        y=ops.nnconv_forward_hidden_raw(x, csr, hidden, pm, root, bias, "mean", hmax=ch["hmax"]),
        y_act=ops.nnconv_forward_hidden_raw(x, csr, hidden, pm, root, bias, "mean", hmax=ch["hmax"], residual=res, relu=True)), o)
    T["nnconv_forward_mixed_raw"] = (dict(x=d["x"], ea=d["ea"], hidden=ch["Hp"]), lambda x, ea, hidden: dict(
        y=ops.nnconv_forward_mixed_raw(x, csr, ea, hidden, ch["hpmax"], ch["hn"], pm, root, bias, "mean")), o)
    T["edge_weights_raw"] = (dict(hidden=ch["H32"]), lambda hidden: dict(We=ops.edge_weights_raw(hidden, pm, Wd[-1], Bd[-1])), o)
    T["nnconv_forward_edgeweights_raw"] = (dict(x=d["x"], we=ch["we"]), lambda x, we: dict(
        y=ops.nnconv_forward_edgeweights_raw(x, csr, we, root, bias, "mean")), o)

    def group(x, we, res):
        r = ops.nnconv_forward_edgeweights_group([dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="add"),
                                                  dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="mean", residual=res, relu=True),
                                                  dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="max")])
        return dict(y_add=r[0], y_act=r[1], y_max=r[2])
    T["nnconv_forward_edgeweights_group"] = (dict(x=d["x"], we=ch["we"], res=d["res"]), group, o)

    def bwd_we(x, we, g):
        gx, gwe, groot, gbias = ops.nnconv_backward_edgeweights_raw(x, csr, we, root, "mean", g)[:4]
        return dict(dx=gx, dWe=gwe, droot=groot, dbias=gbias)
    T["nnconv_backward_edgeweights_raw"] = (dict(x=d["x"], we=ch["we"], g=d["g"]), bwd_we, o)

    def we_bwd(grad_we, hidden):
        gh, gw, gb = ops.edge_weights_backward_raw(grad_we, hidden, dims, Wd[-1])
        return dict(dU=gh[:, :dims[-2]], dU_pad=gh, dW_last=gw, db_last=gb)
    T["edge_weights_backward_raw"] = (dict(grad_we=ch["gwe"], hidden=ch["H32"]), we_bwd, o)

    def bwd_h(x, hidden, g):
        gx, gh, gw, gb, groot, gbias = ops.nnconv_backward_hidden_raw(x, csr, hidden, dims, Wd[-1], Bd[-1], root, "mean", g)
        return dict(dx=gx, dU=gh[:, :dims[-2]], dU_pad=gh, dW_last=gw, db_last=gb, droot=groot, dbias=gbias)
    T["nnconv_backward_hidden_raw"] = (dict(x=d["x"], hidden=ch["H"], g=d["g"]), bwd_h, o)

    def h_bwd(ea, grad_hidden):
        r = _flat(ops.hidden_backward_raw(csr, ea, dims, Wd[:-1], Bd[:-1], grad_hidden))
        out = {f"dW{l}": r[l] for l in range(nl - 1)}
        out.update({f"db{l}": r[nl - 1 + l] for l in range(nl - 1)})
        return out
    T["hidden_backward_raw"] = (dict(ea=d["ea"], grad_hidden=ch["grad_h"]), h_bwd, o)
    T["gather_rows"] = (dict(rows=d["ea"]), lambda rows: dict(rows=ops.gather_rows(rows, csr.perm)),
                        {"rows": c["ea"][csr.perm.cpu().long()].double()})

    # any width 24 -> 40 (materialised per-edge weights, re-associated), bipartite 12 / 5 -> 12
    a = _any(24, 40)
    ad, acsr = a["d"], a["csr"]
    y_any = _any_oracle(a, "mean", we=a["we"])
    _, r_any = _any_oracle(a, "mean", we=a["we"], grads=True)
    o_any = dict(y=y_any, y_max=torch.relu(a["res"].double() + _any_oracle(a, "max", we=a["we"])), dx=r_any["x"], dwe=r_any["leaves"][0],
                 droot=r_any["root"], dbias=r_any["bias"])
    _, r_h = _any_oracle(a, "mean", grads=True)
    o_anyh = dict(y=_any_oracle(a, "mean"), dx=r_h["x"], dh=r_h["leaves"][0], dw_last=r_h["leaves"][1], db_last=r_h["leaves"][2],
                  droot=r_h["root"], dbias=r_h["bias"])
    T["nnconv_forward_edgeweights_any_raw"] = (dict(x=ad["x"], we=ad["we"], res=ad["res"]), lambda x, we, res: dict(
        y=ops.nnconv_forward_edgeweights_any_raw(x, acsr, we, ad["root"], ad["bias"], "mean"),
        y_max=ops.nnconv_forward_edgeweights_any_raw(x, acsr, we, ad["root"], ad["bias"], "max", residual=res, relu=True)), o_any)
    T["nnconv_backward_edgeweights_any_raw"] = (dict(x=ad["x"], we=ad["we"], g=ad["g"]), lambda x, we, g: dict(zip(
        ("dx", "dwe", "droot", "dbias"), ops.nnconv_backward_edgeweights_any_raw(x, acsr, we, ad["root"], "mean", g))), o_any)
    T["nnconv_forward_hidden_any_raw"] = (dict(x=ad["x"], hidden=ad["hidden"]), lambda x, hidden: dict(
        y=ops.nnconv_forward_hidden_any_raw(x, acsr, hidden, ad["w_last"], ad["b_last"], ad["root"], ad["bias"], "mean")), o_anyh)
    T["nnconv_backward_hidden_any_raw"] = (dict(x=ad["x"], hidden=ad["hidden"], g=ad["g"]), lambda x, hidden, g: dict(zip(
        ("dx", "dh", "dw_last", "db_last", "droot", "dbias"),
        ops.nnconv_backward_hidden_any_raw(x, acsr, hidden, ad["w_last"], ad["b_last"], ad["root"], "mean", g))), o_anyh)

    b = _any(12, 12, n_src=45, cind=5)
    bd, bcsr = b["d"], b["csr"]
    _, r_b = _any_oracle(b, "mean", we=b["we"], xd=b["xd"], grads=True)
    _, r_bh = _any_oracle(b, "mean", xd=b["xd"], grads=True)
    o_b = dict(y=_any_oracle(b, "mean", we=b["we"], xd=b["xd"]), dx_src=r_b["x"], dx_dst=r_b["xd"], dwe=r_b["leaves"][0], droot=r_b["root"],
               dbias=r_b["bias"])
    o_bh = dict(y=_any_oracle(b, "add", xd=b["xd"]), dx_src=r_bh["x"], dx_dst=r_bh["xd"], dh=r_bh["leaves"][0], dw_last=r_bh["leaves"][1],
                db_last=r_bh["leaves"][2], droot=r_bh["root"], dbias=r_bh["bias"])
    T["nnconv_forward_edgeweights_bip_raw"] = (dict(x=bd["x"], xd=bd["xd"], we=bd["we"]), lambda x, xd, we: dict(
        y=ops.nnconv_forward_edgeweights_bip_raw(x, xd, bcsr, we, bd["root"], bd["bias"], "mean")), o_b)
    T["nnconv_backward_edgeweights_bip_raw"] = (dict(x=bd["x"], xd=bd["xd"], we=bd["we"], g=bd["g"]), lambda x, xd, we, g: dict(zip(
        ("dx_src", "dx_dst", "dwe", "droot", "dbias"), ops.nnconv_backward_edgeweights_bip_raw(x, xd, bcsr, we, bd["root"], "mean", g))), o_b)
    T["nnconv_forward_hidden_bip_raw"] = (dict(x=bd["x"], xd=bd["xd"], hidden=bd["hidden"]), lambda x, xd, hidden: dict(
        y=ops.nnconv_forward_hidden_bip_raw(x, xd, bcsr, hidden, bd["w_last"], bd["b_last"], bd["root"], bd["bias"], "add")), o_bh)
    T["nnconv_backward_hidden_bip_raw"] = (dict(x=bd["x"], xd=bd["xd"], hidden=bd["hidden"], g=bd["g"]), lambda x, xd, hidden, g: dict(zip(
        ("dx_src", "dx_dst", "dh", "dw_last", "db_last", "droot", "dbias"),
        ops.nnconv_backward_hidden_bip_raw(x, xd, bcsr, hidden, bd["w_last"], bd["b_last"], bd["root"], "mean", g))), o_bh)

    # the diagonal operator at w = 24: add / mean / max
    q = _any(24, 24)
    qd, qcsr = q["d"], q["csr"]
    f64 = lambda t: t.double().requires_grad_(True)
    o_q = {}
    for aggr in ("add", "mean", "max"):
        x64, k64, r64, b64 = f64(q["x"]), f64(q["k"]), f64(q["root"]), f64(q["bias"])
        ref = diag_oracle.diag_reference(x64, x64, q["ei"], k64, r64, b64, aggr)
        o_q["y_" + aggr] = ref.detach()
        if aggr != "max":
            (ref * q["g"].double()).sum().backward()
            o_q.update({f"dx_{aggr}": x64.grad, f"dk_{aggr}": k64.grad, f"droot_{aggr}": r64.grad, f"dbias_{aggr}": b64.grad})
    T["diagconv_forward_raw"] = (dict(x=qd["x"], k=qd["k"]), lambda x, k: {
        "y_" + aggr: ops.diagconv_forward_raw(x, ONE, qcsr, k, qd["root"], qd["bias"], aggr) for aggr in ("add", "mean", "max")}, o_q)

    def diag_bwd(x, k, g):
        out = {}
        for aggr in ("add", "mean"):
            gx, _, gk, groot, gbias = ops.diagconv_backward_raw(x, ONE, qcsr, k, qd["root"], aggr, g)
            out.update({f"dx_{aggr}": gx, f"dk_{aggr}": gk, f"droot_{aggr}": groot, f"dbias_{aggr}": gbias})
        return out
    T["diagconv_backward_raw"] = (dict(x=qd["x"], k=qd["k"], g=qd["g"]), diag_bwd, o_q)

    # GCN 16 -> 24 on the 64-wide family's graph: the default route, the fused kernel, the transposed operator of the backward
    gg = torch.Generator().manual_seed(8)
    xg, wg, bg = torch.randn(N64, 16, generator=gg), torch.randn(16, 24, generator=gg) / 4, torch.randn(24, generator=gg)
    norm = ops.gcn_norm(csr)
    norm.reversed
    wgd, bgd = wg.to(D), bg.to(D)
    o_g = dict(y=gcn_oracle.forward(xg, c["ei"], wg, bg), y_fused=gcn_oracle.forward(xg, c["ei"], wg, bg, relu=True))
    coef64, self64 = (torch.from_numpy(t) for t in gcn_oracle.coefficients(c["ei"], N64))
    o_g["y_rev"] = torch.zeros(N64, 16, dtype=torch.float64).index_add(0, c["ei"][0], xg.double()[c["ei"][1]] * coef64.view(-1, 1)) + \
        self64.view(-1, 1) * xg.double()                     # the transposed operator: every edge carries its coefficient back
    T["gcn_forward_raw"] = (dict(x=xg.to(D)), lambda x: dict(
        y=ops.gcn_forward_raw(x, norm, wgd, bgd), y_fused=ops.gcn_forward_raw(x, norm, wgd, bgd, relu=True, route="aggregate_first"),
        y_rev=ops.gcn_forward_raw(x, norm, None, reverse=True)), o_g)
    # the float part of the GCN normalisation on the prebuilt CSR (its reversed graph goes through build_csr and stays out)
    ewg = torch.rand(E64, generator=gg) + 0.5
    cw, sw = (torch.from_numpy(t) for t in gcn_oracle.coefficients(c["ei"], N64, ewg))

    def norm_of(ew):
        ops._gcn_norm_cache.clear()
        nm = ops.gcn_norm(csr, ew)
        return dict(coef=nm.coef, self_coef=nm.self_coef)
    T["gcn_norm"] = (dict(ew=ewg.to(D)), norm_of, dict(coef=cw[csr.perm.cpu().long()], self_coef=sw))
    # the keys of the neighbour cap: single element-wise launches, bit for bit the host's arithmetic (helpers/neighbor_cap.py)
    from tests.helpers import neighbor_cap as nc
    pos = torch.rand(N64, 2, generator=gg, dtype=torch.float64)
    src_np, dst_np = csr.src.cpu().numpy(), csr.dst.cpu().numpy()
    T["edge_sqdist_keys"] = (dict(pos=pos.to(D)), lambda pos: dict(keys=ops.edge_sqdist_keys(csr, pos)),
                             dict(keys=torch.from_numpy(nc.d2_bits(nc.d2_open(pos.numpy(), None, src_np, dst_np)))))
    T["edge_hash_keys"] = (dict(src_ids=csr.src.clone(), dst_ids=csr.dst.clone()), lambda src_ids, dst_ids: dict(
        keys=ops.edge_hash_keys(src_ids, dst_ids, 5)), dict(keys=torch.from_numpy(nc.hash_keys(src_np, dst_np, 5))))
    torch.cuda.synchronize()
    return T


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        _TABLE = _entries()
        base = {}
        for name, (inputs, call, oracle) in _TABLE.items():
            base[name] = call(**inputs)                    # the serial baseline; it also warms every cache and host-side plan
        torch.cuda.synchronize()
        for name, (inputs, call, oracle) in _TABLE.items():
            _TABLE[name] = (inputs, call, oracle, base[name])
    return _TABLE


def test_the_table_names_what_the_host_tier_lists():
    assert {n.split("[")[0] for n in _table()} == set(SIDE_STREAM_TABLE)


@pytest.mark.parametrize("name", sorted(SIDE_STREAM_TABLE) + ["nnconv_forward_raw[f32]"])
def test_entry_point_on_a_side_stream(name):
    """The default stream and a side stream S are both held (S twice as long).  On S the float inputs are produced by device
    copies queued behind S's hold into buffers that hold zeros, then the call is issued on S with no host synchronisation.  A
    launch, zero-fill or copy that slipped onto the null stream would run before the inputs exist (or, held by the default
    stream's hold, still before S's); a call that synchronised the host would find a window closed."""
    inputs, call, oracle, base = _table()[name]
    figs = {}
    for k, v in base.items():
        if k in oracle and v is not None:
            if v.dtype == torch.int64:                       # keys: the host's bits exactly
                figs[k] = (0.0 if torch.equal(v.cpu(), oracle[k]) else float("inf"), 0.0)
            else:
                figs[k] = (rel_l2(v.cpu(), oracle[k].cpu()), TOL_BWD if k.startswith("d") else TOL_FWD)
    print(name, "baseline vs float64", {k: f"{v[0]:.2e}" for k, v in figs.items()})
    assert all(err <= bar for err, bar in figs.values()), figs
    assert figs, "no output of this entry is compared with its reference"
    default = torch.cuda.current_stream()
    S = stream_beside(default)
    staged = {k: torch.zeros_like(v) for k, v in inputs.items()}
    with torch.cuda.stream(S):              # once without a hold: S's allocator pool then holds every block the call needs
        first = call(**inputs)
    torch.cuda.synchronize()
    bad = [k for k in base if not _bits(first[k], base[k])]
    assert not bad, f"outputs of the first side-stream call that differ from the default-stream baseline: {bad}"
    del first
    held0, held_s = hold(default, HOLD_MS), hold(S, 2 * HOLD_MS)
    with IssueTimer() as t, torch.cuda.stream(S):
        for k, v in inputs.items():
            staged[k].copy_(v)
        got = call(**staged)
    open0, open_s = not held0.query(), not held_s.query()
    torch.cuda.synchronize()
    print(f"{name}: issued in {t.ms:.2f} ms of host time; windows open: default {open0}, side {open_s}")
    assert open0 and open_s, "a hold ended before the call was issued: the call synchronised the host"
    bad = [k for k in base if not _bits(got[k], base[k])]
    assert not bad, f"outputs that differ from the default-stream baseline: {bad}"


# ---------------------------------------------------------------------------------------------------------------------------
# 5 + 6. modules with autograd on a side stream; two streams at once
# ---------------------------------------------------------------------------------------------------------------------------
def _module_case(kind):
    """(make() -> module, x, forward(model, x_leaf) -> y, grad_out, oracle(model) -> {name: float64}) of one module family."""
    g = torch.Generator().manual_seed(31)
    if kind == "NNConv_old":
        c = _case64()
        ei, ea = c["ei"].to(D), c["d"]["ea"]
        make = lambda: gp.NNConv_old(64, 64, DenseNet(DIMS, torch.nn.ReLU), aggr="mean").to(D)
        x, gout, cin, cout, ei_h, ea_h = c["x"], c["g"], 64, 64, c["ei"], c["ea"]
    elif kind == "NNConv":
        n, e, cin, cout = 70, 300, 24, 40
        ei_h, ea_h = _graph(n, e, g), torch.randn(e, 6, generator=g)
        ei, ea = ei_h.to(D), ea_h.to(D)
        make = lambda: gp.NNConv(cin, cout, DenseNet([6, 16, cin * cout], torch.nn.ReLU), aggr="mean").to(D)
        x, gout = torch.randn(n, cin, generator=g), torch.randn(n, cout, generator=g)
    elif kind == "NNConvDiag":
        n, e, w = 70, 300, 24
        ei_h, ea_h = _graph(n, e, g), torch.randn(e, 3, generator=g)
        ei, ea = ei_h.to(D), ea_h.to(D)
        make = lambda: gp.NNConvDiag(w, w, torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, w)), aggr="mean").to(D)
        x, gout = torch.randn(n, w, generator=g), torch.randn(n, w, generator=g)
    else:
        c = _case64()
        ei_h, ei = c["ei"], c["ei"].to(D)
        make = lambda: gp.GCNConv(16, 24).to(D)
        x, gout = torch.randn(N64, 16, generator=g), torch.randn(N64, 24, generator=g)
        ea = None
    fwd = (lambda m, xl: m(xl, ei)) if kind == "GCNConv" else (lambda m, xl: m(xl, ei, ea))

    def oracle(m):
        if kind in ("NNConv_old", "NNConv"):
            lin = ops.mlp_linears(m.nn)
            W, B = [l.weight.detach().cpu() for l in lin], [l.bias.detach().cpu() for l in lin]
            root, bias = m.root.detach().cpu(), m.bias.detach().cpu()
            y = nnconv_forward(x, ei_h, ea_h, W, B, root, bias, aggr="mean", in_channels=cin, out_channels=cout, dtype=torch.float64)
            rx, rW, rb, rroot, rbias = nnconv_grads(x, ei_h, ea_h, W, B, root, bias, "mean", gout)
            out = {"y": y, "dx": rx, "root": rroot, "bias": rbias}
            for l, layer in enumerate(lin):
                for nm, p in m.named_parameters():
                    if p is layer.weight:
                        out[nm] = rW[l]
                    elif p is layer.bias:
                        out[nm] = rb[l]
            return out
        if kind == "NNConvDiag":
            m64 = copy.deepcopy(m).double()
            x64 = x.to(D).double().requires_grad_(True)
            ref = diag_oracle.diag_reference(x64, x64, ei, m64.nn(ea.double()), m64.root, m64.bias, "mean")
            (ref * gout.to(D).double()).sum().backward()
            out = {"y": ref.detach(), "dx": x64.grad}
            out.update({nm: p.grad for nm, p in m64.named_parameters()})
            return out
        y, gx, gw, gb = gcn_oracle.gradients(x, ei_h, m.weight, m.bias, gout)
        return {"y": y, "dx": gx, "weight": gw, "bias": gb}
    return make, x.to(D), fwd, gout.to(D), oracle


def _step(model, x, fwd, gout):
    """One training step on the current stream: {name: tensor} of the output, the input gradient and every parameter gradient."""
    leaf = x.clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    y = fwd(model, leaf)
    (y * gout).sum().backward()
    out = {"y": y.detach(), "dx": leaf.grad}
    out.update({nm: p.grad for nm, p in model.named_parameters()})
    return out


def _twin_baseline(kind):
    make, x, fwd, gout, oracle = _module_case(kind)
    torch.manual_seed(13)
    conv, twin = make(), make()
    twin.load_state_dict(conv.state_dict())
    base = _step(twin, x, fwd, gout)                     # the serial baseline on the default stream
    torch.cuda.synchronize()
    ref = oracle(twin)
    figs = {k: rel_l2(v.cpu(), ref[k].cpu()) for k, v in base.items() if k in ref and v is not None}
    print(kind, "default-stream step vs float64", {k: f"{v:.2e}" for k, v in figs.items()})
    assert "y" in figs and "dx" in figs and all(v <= (TOL_FWD if k == "y" else TOL_BWD) for k, v in figs.items()), figs
    return conv, x, fwd, gout, base


@pytest.mark.parametrize("kind", ["NNConv_old", "NNConv", "NNConvDiag", "GCNConv"])
def test_module_training_step_on_a_side_stream(kind):
    """forward, backward() and the gradients read after S.synchronize(), all under torch.cuda.stream(S): the bits of the
    default-stream step of a twin with the same weights."""
    conv, x, fwd, gout, base = _twin_baseline(kind)
    S = stream_beside(torch.cuda.current_stream())
    calls = _lib.n_native_calls
    held = hold(S)
    with torch.cuda.stream(S):
        got = _step(conv, x, fwd, gout)
    window_open = not held.query()
    S.synchronize()
    assert window_open, "the hold ended before the step was issued: the module path synchronised the host"
    assert _lib.n_native_calls > calls
    bad = [k for k in base if not _bits(got[k], base[k])]
    assert not bad, f"tensors that differ from the default-stream step of the twin: {bad}"


def test_two_streams_at_once():
    """Two modules of different families that share no cache entry, each behind a hold on its own stream, released together: the
    library keeps no global state between calls (its only device globals are the timing arrays)."""
    conv1, x1, fwd1, g1, base1 = _twin_baseline("NNConv")
    conv2, x2, fwd2, g2, base2 = _twin_baseline("GCNConv")
    S1, S2 = stream_pair()
    h1, h2 = hold(S1), hold(S2)
    with torch.cuda.stream(S1):
        got1 = _step(conv1, x1, fwd1, g1)
    with torch.cuda.stream(S2):
        got2 = _step(conv2, x2, fwd2, g2)
    open1, open2 = not h1.query(), not h2.query()
    torch.cuda.synchronize()
    assert open1 and open2, "a hold ended before both steps were issued: the two modules ran one after the other"
    bad = [("NNConv", k) for k in base1 if not _bits(got1[k], base1[k])] + [("GCNConv", k) for k in base2 if not _bits(got2[k], base2[k])]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# 7. what a cross-stream hit keeps, a snapshot pins
# ---------------------------------------------------------------------------------------------------------------------------
def _tensor_ptrs(obj, out, seen):
    """data_ptr of every tensor reachable from `obj` through tuples, lists, dicts and the package's own objects (Csr, PackedMlp,
    GcnNorm, the cache records)."""
    if obj is None or id(obj) in seen:
        return out
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        out.add(obj.data_ptr())
    elif isinstance(obj, dict):
        _tensor_ptrs(list(obj.values()), out, seen)
    elif isinstance(obj, (tuple, list, set)):
        for o in obj:
            _tensor_ptrs(o, out, seen)
    elif type(obj).__module__.startswith("graph_pde_amd"):
        names = [s for c in type(obj).__mro__ for s in getattr(c, "__slots__", ())] + list(getattr(obj, "__dict__", {}))
        for nm in names:
            _tensor_ptrs(getattr(obj, nm, None), out, seen)
    return out


def test_a_snapshot_pins_what_a_cross_stream_hit_keeps(monkeypatch):
    """Bookkeeping only - nothing is raced, no stream is held.  Every cache is filled on the default stream: a 64 -> 64 NNConv with
    the kernel MLP [3, 32, 32, 4096] on 256 nodes / 32,768 random edges (attr_in_slot_order engages) and a second instance of it on
    512 nodes / 1,024 edges (the inference W_e form qualifies; one instance per graph, since a module caches one H), and a GCNConv
    on the small graph - one training step, then two calls without gradient each.  Then the snapshots are taken and the same calls
    run once on a side stream: every tensor a cross-stream hit hands to ops._keep_for must be reachable from the snapshots (a
    recorded graph that pinned them reads nothing the caches could free), and every cache name but "deferred" must have counted."""
    monkeypatch.setattr(hidden_cache, "MODE", "on")
    ops.clear_caches()
    hidden_cache.clear()
    g = torch.Generator().manual_seed(71)
    torch.manual_seed(71)
    dims = [3, 32, 32, 4096]
    assert 32768 >= ops._ATTR_SLOT_ORDER_MIN_EDGES and ops.ATTR_SLOT_ORDER
    cases = []
    for n, e in ((256, 32768), (512, 1024)):
        ei, ea = _graph(n, e, g).to(D), torch.randn(e, dims[0], generator=g).to(D)
        conv = gp.NNConv(64, 64, DenseNet(dims, torch.nn.ReLU), aggr="mean").to(D)
        cases.append((conv, torch.randn(n, 64, generator=g).to(D), (lambda m, xl, ei=ei, ea=ea: m(xl, ei, ea)), torch.randn(n, 64, generator=g).to(D)))
    ei_small = ei
    cases.append((gp.GCNConv(16, 24).to(D), torch.randn(512, 16, generator=g).to(D), (lambda m, xl: m(xl, ei_small)),
                  torch.randn(512, 24, generator=g).to(D)))

    def calls(no_grad_calls):
        for model, x, fwd, gout in cases:
            _step(model, x, fwd, gout)
        for model, x, fwd, gout in cases:
            with torch.no_grad():
                for _ in range(no_grad_calls):
                    fwd(model, x)
    calls(2)
    torch.cuda.synchronize()
    assert ops.cross_stream_hits == {}
    ent_big, ent_small = hidden_cache._entries[cases[0][0]], hidden_cache._entries[cases[1][0]]
    assert ent_big.hidden is not None and ent_small.hidden is not None, "the policy built no H"
    pinned = _tensor_ptrs([ops.cache_snapshot(), hidden_cache.snapshot()], set(), set())
    kept, real_keep = [], ops._keep_for
    monkeypatch.setattr(ops, "_keep_for", lambda t, stream: (kept.append(t), real_keep(t, stream)))
    S = stream_beside(torch.cuda.current_stream())
    with torch.cuda.stream(S):
        # (without gradient first: H and W_e of the default stream are still the entries; the training step then rebuilds H from
        # the slot-ordered attributes and runs the backward over the source order and the reversed GCN graph)
        for model, x, fwd, gout in cases:
            with torch.no_grad():
                fwd(model, x)
        for model, x, fwd, gout in cases:
            _step(model, x, fwd, gout)
    S.synchronize()
    torch.cuda.synchronize()
    print("cross-stream hits:", dict(ops.cross_stream_hits), "tensors kept:", len(kept))
    loose = [(tuple(t.shape), t.dtype) for t in kept if t.data_ptr() not in pinned]
    print("kept by a hit but not pinned by the snapshots:", loose)
    assert kept and not loose, loose
    names = {"csr", "pack_mlp", "attr_slot_order", "attr_identity", "src_order", "gcn_norm", "hidden", "edge_weights"}
    assert names <= set(ops.cross_stream_hits), sorted(names - set(ops.cross_stream_hits))
    ops.clear_caches()
    hidden_cache.clear()
