"""GPU tier: property-based random graphs in EVERY forward regime (tests/test_gpu_hypothesis.py draws graphs that all land on
the 8-wave kernel with fp32 aggregation).  A regime is chosen first, then a structure sized so that the library must take
it - and the test asserts that it did, through the host-side route queries (ops.forward_route, ops.fused_kernel_name,
ops.launch_plan) and the per-kind launch counts of _lib.profile_begin / profile_end:

  v3       8-wave kernel, fp32 aggregation          e < 32768, 3 Linear layers
  v6       one wave per SIMD, split-f16 aggregation  32768 <= e <= 48000, 3 Linear layers with k1 >= 225
  edge     per-edge last layer (low in-degree)      e >= 4096, e <= 4 n, k2 >= 256, in-degrees <= 64
  generic  fp32 MFMA kernel                         2 or 4 - 5 Linear layers, or precision="f32"
  chunked  node-chunked plan                        a workspace that holds part of the nodes (n_chunks >= 2)
  per_edge the reference's association              a node with more in-edges than the graph has nodes (ops.per_edge_association)
  max      aggr="max"                               inference (per-edge weights) and the differentiable PyG chain

In every regime the structure carries duplicate edges, self-loops, nodes without in-edges (destinations limited to the first
n_dst nodes), the three edge_index layouts, root / bias on or off, add / mean, and optionally one destination with >= 8,192
in-edges (not in 'edge', where it would leave the regime, nor in 'chunked' and 'max': see there).  The node count bounds what a skewed graph can be: the re-associated regimes need in-degrees up to the node count
(above it the call takes the reference's association, the per_edge regime), so their skewed graphs have > 8,192 nodes.
Forward and every gradient are compared with the float64 oracle: forward <= max(1e-6, 4 x e32) and <= 1e-5 outright when the
fp32 oracle is within 2.5e-6 (e32: the fp32 oracle's own distance from float64), gradients <= 2e-5.  Weights are drawn from the
example's seed after the constructor; edges on the ReLU kink (tests/helpers/kinks.py) and, for 'max', edges tied for a
maximum (tests/helpers/max_ties.py) are removed.  GPDE_HYP_EXAMPLES examples per regime (default 3)."""
import collections
import os

import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops, synth
from oracle.nnconv_oracle import densenet_forward, nnconv_forward, nnconv_grads, rel_l2
from tests.helpers.kinks import edges_off_the_kink
from tests.helpers.max_ties import edges_off_the_max_ties

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD, FWD_FACTOR = 1e-6, 2e-5, 4
NORTH_STAR, E32_WELL = 1e-5, 2.5e-6
N_EXAMPLES = int(os.environ.get("GPDE_HYP_EXAMPLES", "3"))
REGIMES = ["v3", "v6", "edge", "generic", "chunked", "per_edge", "max"]
SKEW = 8192
SKEW_EDGES = SKEW + 400      # into the skewed node: >= SKEW of them survive the kink removal
TAKEN = collections.Counter()


def _kernel(dims, e, precision=None):
    return _lib.lib().gpde_nnconv_fwd_kernel(e, len(dims) - 1, _lib.dims_array(dims),
                                             ops._PRECISION[precision or ops.DEFAULT_PRECISION]).decode()


# hidden widths each fused kernel is built for (its own support predicate, asked at a size where it is the default)
V3_K1 = [k for k in range(16, 321) if _kernel([6, k, 64, 4096], 1000) == "gpde_fused_f16v3_kernel"]
V6_K1 = [k for k in range(16, 321) if _kernel([6, k, 64, 4096], 1 << 20) == "gpde_fused_f16v6_kernel"]


@st.composite
def structures(draw, regime):
    skew = draw(st.booleans())
    dims_mid = None
    precision = None
    aggr = draw(st.sampled_from(["mean", "add"]))
    k0 = draw(st.integers(1, 7))
    if regime == "v3":
        # (a skewed graph - > 8192 nodes, < 32768 edges - has e <= 4 n: its in-degree keeps it off the per-edge last layer)
        dims_mid = [draw(st.sampled_from(V3_K1)), draw(st.integers(16, 320))]
        e = draw(st.integers(SKEW_EDGES + 64, 32767)) if skew else draw(st.integers(1, 20000))
        n = draw(st.integers(SKEW_EDGES + 100, SKEW_EDGES + 800)) if skew else draw(st.integers(2, 400))
    elif regime == "v6":
        dims_mid = [draw(st.sampled_from(V6_K1)), draw(st.integers(16, 320))]
        if skew:            # > 8192 nodes for the skewed node, e > 4 n for the re-associated path
            e = draw(st.integers(40000, 48000))
            n = draw(st.integers(SKEW_EDGES + 100, int(0.9 * e) // 4))
        else:
            e = draw(st.integers(37000, 48000))     # (>= 32768 after the kink removal, which thins a few per cent)
            n = draw(st.integers(320, 4000))
    elif regime == "edge":
        dims_mid = [draw(st.sampled_from(V6_K1 + V3_K1)), draw(st.integers(256, 320))]
        e = draw(st.integers(4600, 12000))
        n = draw(st.integers(e // 4 + 1, 3 * e))
        # a node with more than ops.EDGE_PATH_MAX_IN_DEGREE in-edges takes the re-associated path (the v3 / v6 regimes draw those
        # skewed graphs): the split-f16 per-edge weights measure 4 - 5.6 x the reference's error on such sums (ops.py)
        skew = False
    elif regime == "generic":
        n_lin = draw(st.sampled_from([2, 3, 4, 5]))
        dims_mid = [draw(st.integers(16, 300)) for _ in range(n_lin - 1)]
        precision = "f32" if n_lin == 3 else None
        e = draw(st.integers(SKEW_EDGES + 64, 30000)) if skew else draw(st.integers(1, 20000))
        n = draw(st.integers(SKEW_EDGES + 100, SKEW_EDGES + 800)) if skew else draw(st.integers(2, 400))
    elif regime == "chunked":
        dims_mid = [draw(st.sampled_from(V6_K1 + V3_K1)), draw(st.integers(16, 320))]
        e = draw(st.integers(1, 40000))
        n = draw(st.integers(160, 600))
        skew = False        # (a node chunk holds >= 64 nodes: a skewed graph of > 8192 nodes would need a 128+-node chunk - not small)
    elif regime == "per_edge":
        n_lin = draw(st.integers(2, 5))
        dims_mid = [draw(st.integers(16, 300)) for _ in range(n_lin - 1)]
        n = draw(st.integers(2, 64))
        e = draw(st.integers(SKEW_EDGES + 64, 20000)) if skew else draw(st.integers(4 * n, 20000))
    else:   # max: the gradient runs PyG's chain on [E, 4096] tensors, the oracle differentiates them in float64
        n_lin = draw(st.integers(2, 4))
        dims_mid = [draw(st.integers(16, 256)) for _ in range(n_lin - 1)]
        n = draw(st.integers(2, 300))
        e = draw(st.integers(0, 3000))
        skew = False        # (8,192 in-edges of [E, 4096] float64 autograd: ~1 GB per example)
    n_dst = draw(st.integers(1, n))
    if regime == "per_edge":
        n_dst = min(n_dst, max(1, e // (2 * n)))              # a mean in-degree above the node count
    else:
        if not skew:
            e = min(e, n * n // 2)                            # in-degrees within the node count (_graph enforces it)
        n_dst = max(n_dst, min(n - 1 if skew else n, -(-2 * e // n)))
        if skew:
            n_dst = min(n_dst, n - 1)                         # node n - 1 is the skewed one
    if regime == "edge":
        n_dst = max(n_dst, min(n, -(-e // 24)))               # in-degrees within ops.EDGE_PATH_MAX_IN_DEGREE (_graph enforces it)
    if regime == "max":
        aggr = "max"
    dup = draw(st.integers(0, 64))
    if regime != "per_edge":
        dup = min(dup, n // 4)                                # `dup` copies of one edge stay within the node count too
    if regime == "edge":
        dup = min(dup, 16)
    return {
        "regime": regime, "n": n, "e": e, "k0": k0, "mid": dims_mid, "precision": precision, "aggr": aggr,
        "root": draw(st.booleans()), "bias": draw(st.booleans()), "skew": skew,
        "dup": dup, "loops": draw(st.integers(0, 64)), "n_dst": n_dst,
        "layout": draw(st.sampled_from(["contiguous", "every_other_column", "transposed_storage"])),
        "seed": draw(st.integers(0, 2 ** 31 - 1)),
    }


def _graph(c, g):
    n, e = c["n"], c["e"]
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, c["n_dst"], (e,), generator=g)
    cap = ops.EDGE_PATH_MAX_IN_DEGREE if c["regime"] == "edge" else n
    if c["regime"] != "per_edge" and e and int(torch.bincount(dst).max()) > cap - c["dup"]:
        # the re-associated regimes: every in-degree within the node count (ops.per_edge_association), here balanced
        dst = (torch.arange(e) % c["n_dst"])[torch.randperm(e, generator=g)]
    if c["skew"]:
        dst[:SKEW_EDGES] = n - 1                                                 # one destination with >= 8192 in-edges
    dup, loops = min(c["dup"], e // 4), min(c["loops"], e // 4)
    if dup:
        src[SKEW_EDGES if c["skew"] else 0:][:dup] = src[-1].item()
        dst[SKEW_EDGES if c["skew"] else 0:][:dup] = dst[-1].item()                # `dup` copies of one edge
    if loops:
        src[e - loops:] = dst[e - loops:]                                  # self-loops
    perm = torch.randperm(e, generator=g)                                  # unsorted edge order
    return src[perm], dst[perm]


def _module(c, g):
    dims = [c["k0"]] + c["mid"] + [4096]
    mlp = torch.nn.Sequential(*sum([[torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.ReLU()] for i in range(len(dims) - 1)], [])[:-1])
    conv = gp.NNConv_old(64, 64, mlp, aggr=c["aggr"], root_weight=c["root"], bias=c["bias"])
    with torch.no_grad():     # from the example's seed, AFTER the constructor (NNConv_old.__init__ resets nn: nn_conv.py:258)
        for p_ in conv.nn.parameters():
            p_.copy_(torch.empty_like(p_).uniform_(-1, 1, generator=g) / (p_.shape[-1] ** 0.5))
        for p_ in (conv.root, conv.bias):
            if p_ is not None:
                p_.copy_(torch.empty_like(p_).uniform_(-0.125, 0.125, generator=g))
    return conv


def _layout(ei, layout, d):
    if layout == "every_other_column":
        big = torch.zeros(2, 2 * ei.shape[1], dtype=torch.int64, device=d)
        big[:, ::2] = ei.to(d)
        return big[:, ::2]
    if layout == "transposed_storage":
        return ei.t().contiguous().to(d).t()
    return ei.to(d)


def _assert_forward(err, e32, what):
    if e32 <= E32_WELL:
        assert err <= NORTH_STAR, (what, err, "fp32 oracle vs float64:", e32)
    assert err <= max(TOL_FWD, FWD_FACTOR * e32), (what, err, "fp32 oracle vs float64:", e32)


def _assert_regime(c, csr, pm, x_d, ea_d, root, bias):
    """The regime the example was drawn for is the one the library takes; returns the forward of the checked call."""
    r, aggr = c["regime"], c["aggr"]
    route = ops.forward_route(csr, pm, aggr, precision=c["precision"])
    if r == "per_edge":
        assert route == {"association": "per_edge"}, (c, route)
        return None
    assert route["association"] == "node", (c, route, csr.max_in_degree)
    ws = None
    if r == "chunked":
        full = ops.workspace_bytes(csr.n_nodes, csr.n_edges, pm)
        zrow = 64 * ops.hidden_width(pm.dims) * 4                          # Z bytes per node, the bulk of the workspace
        ws_bytes = full - (csr.n_nodes - csr.n_nodes * 2 // 5) * zrow      # room for ~2/5 of the nodes' Z
        plan = ops.launch_plan(csr.n_nodes, csr.n_edges, pm, ws_bytes)
        assert plan["n_chunks"] >= 2, (c, plan, full, ws_bytes)
        assert ops.forward_route(csr, pm, aggr, ws_bytes=ws_bytes)["n_chunks"] == plan["n_chunks"]
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x_d.device)
    elif r in ("v3", "generic"):
        want = "gpde_fused_f16v3_kernel" if r == "v3" else "gpde_fused_kernel"
        assert route["kernel"] == want and not route["edge_path"] and route["n_chunks"] == 1, (c, route)
    elif r == "v6":
        assert route["kernel"] == "gpde_fused_f16v6_kernel" and not route["edge_path"], (c, route)
    elif r == "edge":
        assert route["edge_path"], (c, route)
    _lib.profile_begin()
    y = ops.nnconv_forward_raw(x_d, csr, ea_d, pm, root, bias, aggr, ws=ws, precision=c["precision"])
    torch.cuda.synchronize()
    prof = _lib.profile_end()
    assert prof["fused"][1] >= 1, (c, prof)
    if r == "v6":
        assert prof["prep"][1] > 0, (c, prof)              # the split-f16 aggregation's pre-passes ran
    if r == "chunked":
        assert prof["epilogue"][1] == plan["n_chunks"], (c, prof, plan)
    return y


def _run_example(c):
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(c["seed"])
    src, dst = _graph(c, g)
    conv = _module(c, g)
    e = src.numel()
    ea = torch.randn(e, c["k0"], generator=g)
    x, gout = torch.randn(c["n"], 64, generator=g), torch.randn(c["n"], 64, generator=g)
    lin = ops.mlp_linears(conv.nn)
    W, B = [l.weight.detach().clone() for l in lin], [l.bias.detach().clone() for l in lin]
    keep = edges_off_the_kink(ea, W, B) if e else torch.ones(0, dtype=torch.bool)
    if c["regime"] == "max":
        keep &= edges_off_the_max_ties(x, torch.stack([src, dst]), ea, W, B)
    src, dst, ea = src[keep], dst[keep], ea[keep].contiguous()
    ei = torch.stack([src, dst])
    if c["skew"]:
        assert int(torch.bincount(dst).max()) >= SKEW, c
    root = None if conv.root is None else conv.root.detach().clone()
    bias = None if conv.bias is None else conv.bias.detach().clone()
    aggr = c["aggr"]
    ref = nnconv_forward(x, ei, ea, W, B, root, bias, aggr=aggr, dtype=torch.float64, chunk_edges=4096)
    e32 = rel_l2(nnconv_forward(x, ei, ea, W, B, root, bias, aggr=aggr, dtype=torch.float32, chunk_edges=4096), ref)

    conv = conv.to(d)
    ei_d = _layout(ei, c["layout"], d)
    if c["regime"] != "max":
        csr = ops.csr_for(ei_d, c["n"])
        pm = ops.pack_mlp([l.weight for l in ops.mlp_linears(conv.nn)], [l.bias for l in ops.mlp_linears(conv.nn)])
        y = _assert_regime(c, csr, pm, x.to(d), ea.to(d), conv.root, conv.bias)
        if y is not None:
            _assert_forward(rel_l2(y.cpu(), ref), e32, ("regime forward", c))
        rx, rW, rb, rroot, rbias = nnconv_grads(x, ei, ea, W, B, root, bias, aggr, gout, chunk_edges=4096)
    else:
        with torch.no_grad():
            y = conv(x.to(d), ei_d, ea.to(d))
        _assert_forward(rel_l2(y.cpu(), ref), e32, ("max inference", c))
        rx, rW, rb, rroot, rbias = _max_grads(x, ei, ea, W, B, root, bias, gout)
    xin = x.to(d).requires_grad_(True)
    out = conv(xin, ei_d, ea.to(d))
    (out * gout.to(d)).sum().backward()
    torch.cuda.synchronize()
    _assert_forward(rel_l2(out.detach().cpu(), ref), e32, ("module forward", c))
    errs = {"dx": rel_l2(xin.grad.cpu(), rx)}
    for l, layer in enumerate(ops.mlp_linears(conv.nn)):
        errs[f"dW{l + 1}"] = rel_l2(layer.weight.grad.cpu(), rW[l])
        errs[f"db{l + 1}"] = rel_l2(layer.bias.grad.cpu(), rb[l])
    if conv.root is not None:
        errs["droot"] = rel_l2(conv.root.grad.cpu(), rroot)
    if conv.bias is not None:
        errs["dbias"] = rel_l2(conv.bias.grad.cpu(), rbias)
    bad = {k: v for k, v in errs.items() if not v <= TOL_BWD}
    assert not bad, (c, bad)
    TAKEN[c["regime"]] += 1


def _max_grads(x, ei, ea, W, B, root, bias, gout):
    """float64 autograd through the oracle's 'max' forward (segment max of the reference-order messages)."""
    leaves = [t.double().requires_grad_(True) for t in [x] + W + B + [t for t in (root, bias) if t is not None]]
    xs, Ws, Bs = leaves[0], leaves[1:1 + len(W)], leaves[1 + len(W):1 + 2 * len(W)]
    rest = leaves[1 + 2 * len(W):]
    r = rest.pop(0) if root is not None else None
    bb = rest.pop(0) if bias is not None else None
    # the oracle's forward (nnconv_forward) detaches its inputs: its messages, segment max and update restated on the leaves
    src, dst = ei[0], ei[1]
    m = torch.matmul(xs[src].unsqueeze(1), densenet_forward(ea.double(), Ws, Bs).view(-1, 64, 64)).squeeze(1)
    agg = torch.full((xs.shape[0], 64), float("-inf"), dtype=torch.float64).scatter_reduce(
        0, dst.unsqueeze(1).expand_as(m), m, reduce="amax", include_self=True)
    agg = torch.where(torch.bincount(dst, minlength=xs.shape[0]).unsqueeze(1) > 0, agg, torch.zeros_like(agg))
    if r is not None:
        agg = agg + xs @ r
    if bb is not None:
        agg = agg + bb
    (agg * gout.double()).sum().backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return z(xs), [z(w) for w in Ws], [z(b) for b in Bs], None if r is None else z(r), None if bb is None else z(bb)


@pytest.mark.parametrize("regime", REGIMES)
@settings(max_examples=N_EXAMPLES, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
@given(data=st.data())
def test_regime_forward_and_gradients_vs_float64(regime, data):
    _run_example(data.draw(structures(regime)))


def test_every_regime_drew_its_examples():
    """Each regime ran at least min(3, GPDE_HYP_EXAMPLES) examples to the end (a regime that quietly stops being taken
    fails its own test above; this one fails if a regime's examples stopped being drawn at all)."""
    if not TAKEN:
        pytest.skip("no regime example ran in this process")
    short = {r: TAKEN[r] for r in REGIMES if TAKEN[r] < min(3, N_EXAMPLES)}
    assert not short, short


def test_headline_and_benchmark_graphs_stay_on_the_fused_f16_kernels():
    """The per-edge association of ill-conditioned sums never takes the reference's radius graphs: G241 (the headline) and
    every bench.py configuration route to the split-f16 fused kernels, G241 to gpde_fused_f16v6_kernel."""
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    lin = [torch.nn.Linear(6, 1024), torch.nn.Linear(1024, 1024), torch.nn.Linear(1024, 4096)]
    pm = ops.pack_mlp([l.weight.to(d) for l in lin], [l.bias.to(d) for l in lin])
    for s, r in [(241, 0.10), (121, 0.10), (61, 0.10), (16, 0.15)]:
        r2 = synth.lattice_r2(s, r)
        rad = int(r2 ** 0.5) + 1
        offs = [(a, b) for a in range(-rad, rad + 1) for b in range(-rad, rad + 1) if a * a + b * b <= r2]
        e = sum((s - abs(a)) * (s - abs(b)) for a, b in offs)          # edges of lattice_radius_graph(s, r)
        csr = ops.Csr(s * s, e, *(torch.zeros(0, dtype=torch.int32),) * 4, _max_in_degree=len(offs))
        assert not ops.per_edge_association(csr, pm.dims, "mean"), (s, r)
        if s == 241:
            assert (e, len(offs)) == (95539625, 1793)
            assert ops.fused_kernel_name(s * s, e, pm) == "gpde_fused_f16v6_kernel"
        else:
            assert ops.fused_kernel_name(s * s, e, pm) in ("gpde_fused_f16v6_kernel", "gpde_fused_f16v3_kernel"), (s, r)
