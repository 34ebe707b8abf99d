"""GPU tier: a frozen input of an any-width / two-node-set NNConv call gets no gradient and changes nothing else.

The autograd Functions of this family (autograd.WeConvAnyFunction, autograd.HiddenAnyFunction) read `ctx.needs_input_grad` by
position and return one gradient per input by position, for a call on one node set and for a call between two.  A slot that is
off by one shows as a gradient that lands on the wrong input, a gradient that is dropped, or one that is computed from the wrong
`need_*` flag.  The `need_*` flags of the native backward only drop outputs (`full` against `part` in
tests/test_gpu_reassoc_any.py), so the bar is bit-equality: with ONE differentiable input frozen, that input's `.grad` is None and
the output and every other gradient are `torch.equal` to the run with every input on.

Cells: {one node set, two sets with in_dst != in_src, two sets with x_dst=None} x {materialised, re-associated} x {add, mean}, at
24 -> 40 (16-byte column accesses) and 7 -> 5 (dword accesses) / (24, 12) -> 40 and (7, 3) -> 5, on the 37 -> 53 graph of
tests/test_gpu_bipartite.py (a 300-edge hub, three destinations without in-edges, three sources without out-edges)."""
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from tests.test_gpu_bipartite import K0, bip_graph, dev
from tests.test_gpu_widths import DenseNet, _linears

pytestmark = pytest.mark.gpu
N_SRC, N_DST = 37, 53
ENTRY_POINTS = [f"nnconv_{d}_{op}_{sets}_raw" for d in ("forward", "backward") for op in ("edgeweights", "hidden") for sets in ("any", "bip")]


@pytest.fixture
def native_trace(monkeypatch):
    """Names of the any-width / two-node-set entry points a test's calls went through, in order."""
    trace = []
    for name in ENTRY_POINTS:
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            trace.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return trace


def run(conv, leaves, frozen, call, g):
    """One forward and backward with the input named `frozen` (or none) not requiring a gradient.  Returns (out, {name: .grad})."""
    for name, t in leaves.items():
        t.grad = None
        t.requires_grad_(name != frozen)
    out = call(conv)
    (out * g).sum().backward()
    return out.detach(), {name: t.grad for name, t in leaves.items()}


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("route", ["materialised", "reassociated"])
@pytest.mark.parametrize("sets,cin,cout", [("one", 24, 40), ("one", 7, 5), ("two", (24, 12), 40), ("two", (7, 3), 5),
                                           ("two_no_dst", (24, 12), 40), ("two_no_dst", (7, 3), 5)])
def test_one_frozen_input_drops_its_gradient_and_nothing_else(sets, cin, cout, route, aggr, monkeypatch, native_trace):
    if route == "reassociated":
        monkeypatch.setattr(ops, "ANY_REASSOC", "on")
    one = sets == "one"
    cs, cd = (cin, cin) if one else cin
    n_src = N_DST if one else N_SRC
    ei, _ = bip_graph(n_src, N_DST, seed=cs + cout)
    gen = torch.Generator().manual_seed(cs * 100 + cout)
    torch.manual_seed(cs * 7 + cout)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, 33, cs * cout]), aggr=aggr).to(dev())
    x_src = torch.randn(n_src, cs, generator=gen).to(dev())
    x_dst = None if sets != "two" else torch.randn(N_DST, cd, generator=gen).to(dev())
    ea = torch.rand(ei.shape[1], K0, generator=gen).to(dev())
    g = torch.randn(N_DST, cout, generator=gen).to(dev())
    last = _linears(conv.nn)[-1]
    leaves = {"x_src": x_src, "edge_attr": ea, "w_last": last.weight, "b_last": last.bias, "bias": conv.bias}
    if x_dst is not None:
        leaves["x_dst"] = x_dst
    if sets != "two_no_dst":
        leaves["root"] = conv.root                  # (x_dst=None: no root term, the parameter is not part of the call)
    others = {n: p for n, p in conv.named_parameters() if p is not conv.root and all(p is not t for t in leaves.values())}
    if one:
        call = lambda c: c(x_src, ei, ea)
    else:
        call = lambda c: c((x_src, x_dst), ei, ea, size=(n_src, N_DST))

    def grads_of(frozen):
        conv.zero_grad()
        del native_trace[:]
        out, gr = run(conv, leaves, frozen, call, g)
        op, kind = ("hidden" if route == "reassociated" else "edgeweights"), ("any" if one else "bip")
        assert native_trace == [f"nnconv_forward_{op}_{kind}_raw", f"nnconv_backward_{op}_{kind}_raw"], native_trace
        gr.update({n: p.grad for n, p in others.items()})
        return out, {n: (None if t is None else t.clone()) for n, t in gr.items()}

    out0, g0 = grads_of(None)
    assert all(g0[n] is not None and bool(torch.isfinite(g0[n]).all()) and float(g0[n].abs().max()) > 0 for n in g0), \
        [n for n in g0 if g0[n] is None]
    if sets == "two_no_dst":
        assert conv.root.grad is None
    for frozen in leaves:
        out, gr = grads_of(frozen)
        assert gr[frozen] is None, frozen
        assert torch.equal(out, out0), frozen
        bad = [n for n in g0 if n != frozen and (gr[n] is None or not torch.equal(gr[n], g0[n]))]
        print(f"[frozen] {sets} {cin}->{cout} {route} {aggr}: {frozen} frozen, differing gradients {bad}")
        assert not bad, (frozen, bad)
