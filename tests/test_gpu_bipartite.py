"""GPU tier: NNConv BETWEEN TWO NODE SETS (gpde_nnconv_*_edgeweights_bip, gpde_nnconv_*_hidden_bip, gpde_csr_from_coo2) and
flow='target_to_source'.

    out_i = aggr_{e: j -> i} x_src[j] . W_e  (+ x_dst[i] . root when x_dst is given and the module has a root)  + bias

The float64 oracle is the composite below (`oracle_out`): gather x_src by row 0, per-edge product, index_add_ over row 1 into n_dst
rows, / clamp(count, 1) for mean, + x_dst @ root + bias; its gradients come from float64 autograd.  Bars: the project's own
(tests/test_gpu_widths.py, tests/test_gpu_reassoc_any.py) - relative L2 <= 1e-5 forward, <= 2e-5 every gradient, worst destination
row with in-degree >= 1 <= 1e-5.  Every test prints the figures it asserts on (-s shows them)."""
import copy

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from tests.helpers.any_tilings import worst_row
from tests.test_gpu_widths import DenseNet, _rel

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD, TOL_ROW = 1e-5, 2e-5, 1e-5
SHAPES = [(37, 53), (53, 37)]
WIDTHS = [((1, 1), 8), ((24, 24), 40), ((40, 40), 24), ((64, 64), 64), ((24, 7), 40), ((7, 24), 5), ((132, 132), 256)]
K0 = 6


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def route_on(monkeypatch):
    monkeypatch.setattr(ops, "ANY_REASSOC", "on")


class Tap(torch.nn.Module):
    """A kernel network that is NOT a Linear / ReLU chain to the module (always the materialised route) and keeps the gradient of
    the per-edge weights it returned (rows in the order it was called with: CSR slot order)."""

    def __init__(self, dims):
        super().__init__()
        self.net = DenseNet(dims)
        self.grads = []

    def forward(self, p):
        w = self.net(p)
        if w.requires_grad:
            w.register_hook(self.grads.append)
        return w


def bip_graph(n_src, n_dst, seed, hub=300, e_rest=300):
    """(edge_index: a strided, non-contiguous int64 [2, E] view, in-degree per destination).  Destination 1 has `hub` in-edges,
    the last three destinations none, the last three sources no out-edge; 20 copies of one edge; no sorted order."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n_src - 3, (hub + e_rest,), generator=g)
    dst = torch.cat([torch.full((hub,), 1, dtype=torch.int64), torch.randint(0, n_dst - 3, (e_rest,), generator=g)])
    src[hub:hub + 20], dst[hub:hub + 20] = 2, 4
    perm = torch.randperm(hub + e_rest, generator=g)
    big = torch.zeros(2, 2 * (hub + e_rest), dtype=torch.int64, device=dev())
    ei = big[:, 1::2]
    ei.copy_(torch.stack([src[perm], dst[perm]]))
    assert not ei.is_contiguous()
    deg = torch.bincount(dst, minlength=n_dst)
    assert int((deg == 0).sum()) >= 3 and int(torch.bincount(src, minlength=n_src)[-3:].sum()) == 0
    return ei, deg.to(dev())


def oracle_out(xs, xd, ei, w, root, bias, aggr, n_dst):
    """The float64 composite of the module docstring; `w` [E, in_src * out] in the order of `ei`."""
    cin = xs.shape[1]
    cout = w.shape[1] // cin
    m = torch.bmm(xs[ei[0]].unsqueeze(1), w.view(-1, cin, cout)).squeeze(1)
    if aggr == "max":
        out = torch.full((n_dst, cout), float("-inf"), dtype=xs.dtype, device=xs.device)
        out = out.scatter_reduce(0, ei[1].unsqueeze(1).expand_as(m), m, "amax", include_self=True)
        out = torch.where(torch.isinf(out), torch.zeros_like(out), out)
    else:
        out = torch.zeros(n_dst, cout, dtype=xs.dtype, device=xs.device).index_add_(0, ei[1], m)
        if aggr == "mean":
            out = out / torch.bincount(ei[1], minlength=n_dst).clamp(min=1).to(xs.dtype).unsqueeze(1)
    if xd is not None and root is not None:
        out = out + xd @ root
    if bias is not None:
        out = out + bias
    return out


def inputs(n_src, n_dst, cs, cd, cout, e, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(dev())
    return r(n_src, cs), r(n_dst, cd), torch.rand(e, K0, generator=g).to(dev()), r(n_dst, cout)


def step(conv, xs, xd, ei, ea, n_dst, g, deg, tag):
    """One training step of `conv` on the rectangular call against the float64 oracle: every bar.  Returns (out, grads dict)."""
    conv.zero_grad()
    conv64 = copy.deepcopy(conv).double()
    xs32, xd32 = xs.clone().requires_grad_(True), None if xd is None else xd.clone().requires_grad_(True)
    out = conv((xs32, xd32), ei, ea, size=(xs.shape[0], n_dst))
    (out * g).sum().backward()
    xs64, xd64 = xs.double().requires_grad_(True), None if xd is None else xd.double().requires_grad_(True)
    w64 = conv64.nn(ea.double())
    w64.retain_grad()
    ref = oracle_out(xs64, xd64, ei, w64, conv64.root, conv64.bias, conv.aggr, n_dst)
    (ref * g.double()).sum().backward()
    errs = {"out": _rel(out.detach(), ref.detach()), "row": worst_row(out.detach()[deg >= 1], ref.detach()[deg >= 1]),
            "gx_src": _rel(xs32.grad, xs64.grad)}
    grads = {"gx_src": xs32.grad}
    if xd is not None:
        errs["gx_dst"] = _rel(xd32.grad, xd64.grad if xd64.grad is not None else torch.zeros_like(xd64))
        grads["gx_dst"] = xd32.grad
    if isinstance(conv.nn, Tap):
        perm = ops.csr_for(ei, n_dst, n_src=xs.shape[0]).perm.long()
        errs["gW_e"] = _rel(conv.nn.grads[-1], w64.grad[perm])
        grads["gW_e"] = conv.nn.grads[-1]
    for (name, p), (_, p64) in zip(conv.named_parameters(), conv64.named_parameters()):
        if xd is None and name == "root":
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
            continue
        errs["g_" + name], grads["g_" + name] = _rel(p.grad, p64.grad), p.grad
    print(f"[bipartite] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert out.shape == (n_dst, conv.out_channels)
    assert errs["out"] <= TOL_FWD and errs["row"] <= TOL_ROW, errs
    assert all(v <= TOL_BWD for k, v in errs.items() if k not in ("out", "row")), errs
    return out.detach(), grads


# ---- 1. both directions of rectangularity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("cin,cout", WIDTHS)
@pytest.mark.parametrize("n_src,n_dst", SHAPES)
def test_materialised_route_vs_float64_oracle(n_src, n_dst, cin, cout, aggr):
    ei, deg = bip_graph(n_src, n_dst, seed=n_src + cout)
    xs, xd, ea, g = inputs(n_src, n_dst, cin[0], cin[1], cout, ei.shape[1], seed=cout)
    torch.manual_seed(cin[0] * 7 + cout)
    # (equal widths: given as an int in one direction and as a pair in the other - both spellings run the same call)
    conv = gp.NNConv(cin[0] if cin[0] == cin[1] and n_src < n_dst else cin, cout, Tap([K0, 16, cin[0] * cout]), aggr=aggr).to(dev())
    calls0 = _lib.n_native_calls
    step(conv, xs, xd, ei, ea, n_dst, g, deg, f"materialised {n_src}->{n_dst} {cin}->{cout} {aggr}")
    assert _lib.n_native_calls - calls0 == 2            # one native forward, one native backward (the CSR is not counted)


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("cin,cout", WIDTHS)
@pytest.mark.parametrize("n_src,n_dst", SHAPES)
def test_reassociated_route_vs_float64_oracle(n_src, n_dst, cin, cout, aggr, route_on, monkeypatch):
    seen = []
    for name in ("nnconv_forward_hidden_bip_raw", "nnconv_backward_hidden_bip_raw"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            seen.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    ei, deg = bip_graph(n_src, n_dst, seed=n_src + cout + 1)
    xs, xd, ea, g = inputs(n_src, n_dst, cin[0], cin[1], cout, ei.shape[1], seed=cout + 1)
    torch.manual_seed(cin[0] * 7 + cout + 1)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, 33, cin[0] * cout]), aggr=aggr).to(dev())
    step(conv, xs, xd, ei, ea, n_dst, g, deg, f"reassociated {n_src}->{n_dst} {cin}->{cout} {aggr}")
    assert seen == ["nnconv_forward_hidden_bip_raw", "nnconv_backward_hidden_bip_raw"], seen


@pytest.mark.parametrize("cin,cout", WIDTHS)
@pytest.mark.parametrize("n_src,n_dst", SHAPES)
def test_max_inference_vs_float64_oracle(n_src, n_dst, cin, cout):
    ei, deg = bip_graph(n_src, n_dst, seed=n_src + cout + 2)
    xs, xd, ea, _ = inputs(n_src, n_dst, cin[0], cin[1], cout, ei.shape[1], seed=cout + 2)
    torch.manual_seed(cout + 2)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, cin[0] * cout]), aggr="max").to(dev())
    with torch.no_grad():
        out = conv((xs, xd), ei, ea)
        ref = oracle_out(xs.double(), xd.double(), ei, copy.deepcopy(conv.nn).double()(ea.double()), conv.root.double(), conv.bias.double(), "max", n_dst)
    e, row = _rel(out, ref), worst_row(out[deg >= 1], ref[deg >= 1])
    print(f"[bipartite] max {n_src}->{n_dst} {cin}->{cout}: out={e:.2e} row={row:.2e}")
    assert e <= TOL_FWD and row <= TOL_ROW
    with pytest.raises(NotImplementedError, match="aggr='max' with a gradient"):
        conv((xs.clone().requires_grad_(True), xd), ei, ea)


# ---- 2. identity with the square operator ------------------------------------------------------------------------------------
def _square_embedding(conv, xs, xd, ei, ea, g):
    """Today's square module on one index space of n_src + n_dst nodes (sources first), the loss on the destination rows only."""
    n_src = xs.shape[0]
    x = torch.cat([xs, xd]).requires_grad_(True)
    ei_sq = torch.stack([ei[0], ei[1] + n_src])
    out = conv(x, ei_sq, ea)
    (out * torch.cat([torch.zeros(n_src, g.shape[1], device=g.device), g])).sum().backward()
    return out.detach()[n_src:], x.grad[:n_src], x.grad[n_src:]


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("cin,cout", [(24, 40), (40, 24), (7, 5)])
@pytest.mark.parametrize("n_src,n_dst", SHAPES)
def test_materialised_route_is_bit_identical_to_the_square_embedding(n_src, n_dst, cin, cout, aggr):
    ei, _ = bip_graph(n_src, n_dst, seed=cin)
    xs, xd, ea, g = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=cin)
    torch.manual_seed(cin)
    conv = gp.NNConv(cin, cout, Tap([K0, 16, cin * cout]), aggr=aggr).to(dev())
    xs32, xd32 = xs.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    out = conv((xs32, xd32), ei, ea)
    (out * g).sum().backward()
    gwe = conv.nn.grads[-1]
    groot, gbias = conv.root.grad.clone(), conv.bias.grad.clone()
    conv.zero_grad()
    out_sq, gxs_sq, gxd_sq = _square_embedding(conv, xs, xd, ei, ea, g)
    same = {"out": torch.equal(out.detach(), out_sq), "gW_e": torch.equal(gwe, conv.nn.grads[-1]), "gx_src": torch.equal(xs32.grad, gxs_sq),
            "gx_dst": torch.equal(xd32.grad, gxd_sq), "gbias": torch.equal(gbias, conv.bias.grad)}
    print(f"[bipartite] square identity (materialised) {n_src}->{n_dst} {cin}->{cout} {aggr}: {same} "
          f"groot rel={_rel(groot, conv.root.grad):.2e}")
    assert all(same[k] for k in ("out", "gW_e", "gx_src", "gx_dst")), same
    assert _rel(groot, conv.root.grad) <= 1e-6          # (x^T g over n_src + n_dst rows, the source rows adding zeros, in other strips)


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("cin,cout", [(24, 40), (40, 24)])
@pytest.mark.parametrize("n_src,n_dst", SHAPES)
def test_reassociated_route_equals_the_square_embedding(n_src, n_dst, cin, cout, aggr, route_on, monkeypatch):
    ei, _ = bip_graph(n_src, n_dst, seed=cin + 1)
    xs, xd, ea, g = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=cin + 1)
    torch.manual_seed(cin + 1)
    net = DenseNet([K0, 16, 33, cin * cout])
    conv = gp.NNConv(cin, cout, net, aggr=aggr).to(dev())
    taps = []                                           # dL/dH as the two native backwards return it (rows in CSR slot order)
    for name, k in (("nnconv_backward_hidden_bip_raw", 2), ("nnconv_backward_hidden_any_raw", 1)):
        def spy(*a, _f=getattr(ops, name), _k=k, **kw):
            r = _f(*a, **kw)
            taps.append(r[_k])
            return r
        monkeypatch.setattr(ops, name, spy)
    xs32, xd32 = xs.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    out = conv((xs32, xd32), ei, ea)
    (out * g).sum().backward()
    gh = taps[-1]
    conv.zero_grad()
    out_sq, gxs_sq, gxd_sq = _square_embedding(conv, xs, xd, ei, ea, g)
    errs = {"out": _rel(out.detach(), out_sq), "gx_src": _rel(xs32.grad, gxs_sq), "gx_dst": _rel(xd32.grad, gxd_sq), "gH": _rel(gh, taps[-1])}
    bits = {"out": torch.equal(out.detach(), out_sq), "gx_src": torch.equal(xs32.grad, gxs_sq), "gx_dst": torch.equal(xd32.grad, gxd_sq),
            "gH": torch.equal(gh, taps[-1])}
    print(f"[bipartite] square identity (re-associated) {n_src}->{n_dst} {cin}->{cout} {aggr}: {errs} bit-equal: {bits}")
    assert all(v <= 1e-6 for v in errs.values()), errs


# ---- 3. x_dst = None -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["materialised", "reassociated"])
def test_without_destination_features_there_is_no_root_term(route, monkeypatch):
    if route == "reassociated":
        monkeypatch.setattr(ops, "ANY_REASSOC", "on")
    n_src, n_dst, cin, cout = 37, 53, 24, 40
    ei, deg = bip_graph(n_src, n_dst, seed=3)
    xs, _, ea, g = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=3)
    torch.manual_seed(3)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, cin * cout]), aggr="mean").to(dev())
    assert conv.root is not None
    step(conv, xs, None, ei, ea, n_dst, g, deg, f"x_dst=None {route}")
    with pytest.raises(ValueError, match="number of destination nodes is unknown"):
        conv((xs, None), ei, ea)


# ---- 4. flow='target_to_source' ------------------------------------------------------------------------------------------------
def _train(conv, x, ei, ea, g, size=None):
    conv.zero_grad()
    xin = tuple(t.clone().requires_grad_(True) for t in x) if isinstance(x, tuple) else x.clone().requires_grad_(True)
    out = conv(xin, ei, ea, size=size)
    (out * g).sum().backward()
    xg = [t.grad for t in xin] if isinstance(xin, tuple) else [xin.grad]
    return [out.detach()] + xg + [p.grad.clone() for p in conv.parameters()]


@pytest.mark.parametrize("cin,cout", [(64, 64), (24, 40)])
def test_target_to_source_equals_the_swapped_edge_index_square(cin, cout):
    n = 41
    g0 = torch.Generator().manual_seed(cin)
    ei = torch.randint(0, n, (2, 500), generator=g0).to(dev())
    x, ea, g = torch.randn(n, cin, generator=g0).to(dev()), torch.rand(500, K0, generator=g0).to(dev()), torch.randn(n, cout, generator=g0).to(dev())
    torch.manual_seed(cin)
    a = gp.NNConv(cin, cout, DenseNet([K0, 16, cin * cout]), aggr="mean", flow="target_to_source").to(dev())
    b = gp.NNConv(cin, cout, copy.deepcopy(a.nn), aggr="mean").to(dev())
    b.load_state_dict(a.state_dict())
    ra, rb = _train(a, x, ei, ea, g), _train(b, x, ei.flip(0), ea, g)
    same = [torch.equal(u, v) for u, v in zip(ra, rb)]
    print(f"[bipartite] flow {cin}->{cout}: bit-equal (out, gx, parameters...) = {same}")
    assert len(ra) == len(rb) and all(same), same
    with torch.no_grad():
        assert torch.equal(a(x, ei, ea), b(x, ei.flip(0), ea))


def test_target_to_source_equals_the_swapped_edge_index_rectangular():
    n_src, n_dst, cin, cout = 37, 53, 24, 40
    ei, _ = bip_graph(n_src, n_dst, seed=4)
    xs, xd, ea, g = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=4)
    torch.manual_seed(4)
    a = gp.NNConv(cin, cout, DenseNet([K0, 16, cin * cout]), aggr="add", flow="target_to_source").to(dev())
    b = gp.NNConv(cin, cout, copy.deepcopy(a.nn), aggr="add").to(dev())
    b.load_state_dict(a.state_dict())
    ra, rb = _train(a, (xs, xd), ei.flip(0), ea, g), _train(b, (xs, xd), ei, ea, g)
    same = [torch.equal(u, v) for u, v in zip(ra, rb)]
    print(f"[bipartite] flow rectangular: bit-equal = {same}")
    assert len(ra) == len(rb) and all(same), same


# ---- 5. graph builders ---------------------------------------------------------------------------------------------------------
def test_radius_csr_between_two_point_sets():
    g = torch.Generator().manual_seed(5)
    pos, q = torch.rand(40, 2, generator=g, dtype=torch.float64).to(dev()), torch.rand(12, 2, generator=g, dtype=torch.float64).to(dev())
    csr = ops.radius_csr(pos, 0.3, pos_dst=q)
    ref = ops.csr_for(ops.radius_graph(pos, 0.3, pos_dst=q), 12, n_src=40)
    assert csr.n_nodes == 12 and csr.n_src == 40 and csr.n_edges == ref.n_edges > 0
    for name in ("rowptr", "src", "dst"):
        assert torch.equal(getattr(csr, name), getattr(ref, name)), name
    assert torch.equal(csr.perm, torch.arange(csr.n_edges, dtype=torch.int32, device=dev()))


def test_down_graph_of_two_levels_with_level_local_ids():
    g = torch.Generator().manual_seed(6)
    levels = [torch.rand(40, 2, generator=g, dtype=torch.float64).to(dev()), torch.rand(12, 2, generator=g, dtype=torch.float64).to(dev())]
    down = ops.multilevel_radius_graphs(levels, [0.2, 0.4], [0.3])["down"][0]
    cin, cout, e = 24, 40, down.shape[1]
    assert e > 0 and int(down[0].max()) < 40 and int(down[1].max()) < 12
    xs, xd, ea, _ = inputs(40, 12, cin, cin, cout, e, seed=6)
    torch.manual_seed(6)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, cin * cout]), aggr="mean").to(dev())
    with torch.no_grad():
        out = conv((xs, xd), down, ea)
        shared = conv(torch.cat([xs, xd]), torch.stack([down[0], down[1] + 40]), ea)[40:]
        via_csr = conv((xs, xd), ops.radius_csr(levels[0], 0.3, reference_ties=True, pos_dst=levels[1]),
                       ea[ops.csr_for(down, 12, n_src=40).perm.long()])
    print(f"[bipartite] down graph: {e} edges, rel = {_rel(out, shared):.2e}")
    assert out.shape == (12, cout) and torch.equal(out, shared) and torch.equal(out, via_csr)


# ---- 6. degenerate calls -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["materialised", "reassociated"])
def test_no_edges_no_sources_no_destinations(route, monkeypatch):
    if route == "reassociated":
        monkeypatch.setattr(ops, "ANY_REASSOC", "on")
    cin, cout = 24, 40
    torch.manual_seed(7)
    conv = gp.NNConv((cin, 7), cout, DenseNet([K0, 16, cin * cout]), aggr="mean").to(dev())
    none = torch.zeros(2, 0, dtype=torch.int64, device=dev())
    ea0 = torch.zeros(0, K0, device=dev())
    for n_src, n_dst in ((5, 9), (0, 9), (5, 0)):
        xs, xd = torch.randn(n_src, cin, device=dev(), requires_grad=True), torch.randn(n_dst, 7, device=dev(), requires_grad=True)
        conv.zero_grad()
        out = conv((xs, xd), none, ea0)
        ref = xd.detach().double() @ conv.root.detach().double() + conv.bias.detach().double()
        assert out.shape == (n_dst, cout) and (n_dst == 0 or _rel(out.detach(), ref) <= TOL_FWD)
        out.sum().backward()
        assert xs.grad is None or float(xs.grad.abs().sum()) == 0.0
        if n_dst:
            assert _rel(xd.grad, conv.root.detach().double().sum(1).expand(n_dst, 7)) <= TOL_BWD
            assert _rel(conv.root.grad, xd.detach().double().sum(0).unsqueeze(1).expand(7, cout)) <= TOL_BWD
            assert _rel(conv.bias.grad, torch.full((cout,), float(n_dst))) <= TOL_BWD
        print(f"[bipartite] degenerate {route} ({n_src}, {n_dst}): ok")


@pytest.mark.parametrize("root_weight,bias", [(False, True), (True, False), (False, False)])
def test_without_root_or_bias(root_weight, bias):
    n_src, n_dst, cin, cout = 53, 37, 24, 40
    ei, deg = bip_graph(n_src, n_dst, seed=8)
    xs, xd, ea, g = inputs(n_src, n_dst, cin, 7, cout, ei.shape[1], seed=8)
    torch.manual_seed(8)
    conv = gp.NNConv((cin, 7), cout, Tap([K0, 16, cin * cout]), aggr="add", root_weight=root_weight, bias=bias).to(dev())
    _, grads = step(conv, xs, xd, ei, ea, n_dst, g, deg, f"root={root_weight} bias={bias}")
    if not root_weight:
        assert float(grads["gx_dst"].abs().max()) == 0.0


def test_misaligned_views_take_the_dword_tiling():
    """x_dst / residual / W_e handed over at addresses that are not 16-byte aligned: the V = 1 fallback, the same result."""
    n_src, n_dst, cin, cout = 37, 53, 24, 40
    ei, deg = bip_graph(n_src, n_dst, seed=9)
    xs, xd, ea, _ = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=9)
    csr = ops.csr_for(ei, n_dst, n_src=n_src)
    g0 = torch.Generator().manual_seed(9)
    we = torch.randn(csr.n_edges * cin * cout + 1, generator=g0).to(dev())
    root, res = torch.randn(cin * cout + 1, generator=g0).to(dev()), torch.randn(n_dst * cout + 1, generator=g0).to(dev())
    xdm = torch.empty(n_dst * cin + 1, device=dev())[1:].view(n_dst, cin).copy_(xd)
    we_m, root_m, res_m = we[1:].view(-1, cin * cout), root[1:].view(cin, cout), res[1:].view(n_dst, cout)
    assert we_m.data_ptr() % 16 == 4 and xdm.data_ptr() % 16 == 4
    out_m = ops.nnconv_forward_edgeweights_bip_raw(xs, xdm, csr, we_m, root_m, None, "add", residual=res_m, relu=True)
    out_a = ops.nnconv_forward_edgeweights_bip_raw(xs, xd, csr, we_m.clone(), root_m.clone(), None, "add", residual=res_m.clone(), relu=True)
    slot_ei = csr.edge_index
    ref = torch.relu(oracle_out(xs.double(), xd.double(), slot_ei, we_m.double(), root_m.double(), None, "add", n_dst) + res_m.double())
    print(f"[bipartite] misaligned: V=1 {_rel(out_m, ref):.2e} V=4 {_rel(out_a, ref):.2e}")
    assert _rel(out_m, ref) <= TOL_FWD and _rel(out_a, ref) <= TOL_FWD
    gm = ops.nnconv_backward_edgeweights_bip_raw(xs, xdm, csr, we_m, root_m, "add", res_m)
    ga = ops.nnconv_backward_edgeweights_bip_raw(xs, xd, csr, we_m.clone(), root_m.clone(), "add", res_m.clone())
    for u, v in zip(gm, ga):
        assert _rel(u, v.double()) <= TOL_BWD


def test_cpu_tensors_are_staged_and_returned_on_the_cpu():
    n_src, n_dst, cin, cout = 37, 53, 24, 40
    ei, _ = bip_graph(n_src, n_dst, seed=10)
    xs, xd, ea, g = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=10)
    torch.manual_seed(10)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, cin * cout]), aggr="mean")
    xs_c, xd_c = xs.cpu().requires_grad_(True), xd.cpu().requires_grad_(True)
    out_c = conv((xs_c, xd_c), ei.cpu(), ea.cpu())
    assert out_c.device.type == "cpu"
    (out_c * g.cpu()).sum().backward()
    conv_d = copy.deepcopy(conv).to(dev())
    conv_d.zero_grad()
    res = _train(conv_d, (xs, xd), ei, ea, g)
    # (the kernel network ran on the CPU in one call and on the device in the other: the same operator on W_e that agree to fp32 rounding)
    errs = [_rel(out_c, res[0]), _rel(xs_c.grad, res[1]), _rel(xd_c.grad, res[2]), _rel(conv.root.grad, conv_d.root.grad)]
    print(f"[bipartite] CPU tensors staged: out / gx_src / gx_dst / groot vs the device module = {errs}")
    assert errs[0] <= TOL_FWD and all(v <= TOL_BWD for v in errs[1:])
    assert xs_c.grad.device.type == "cpu" and conv.root.grad.device.type == "cpu"


def test_residual_and_relu():
    n_src, n_dst, cin, cout = 37, 53, 24, 40
    ei, _ = bip_graph(n_src, n_dst, seed=11)
    xs, xd, ea, res = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=11)
    torch.manual_seed(11)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, cin * cout]), aggr="mean").to(dev())
    with torch.no_grad():
        plain = conv((xs, xd), ei, ea)
        fused = conv((xs, xd), ei, ea, residual=res, activation="relu")
    want = torch.relu(res + plain)
    print(f"[bipartite] residual + relu fused: rel = {_rel(fused, want):.2e}")
    assert _rel(fused, want) <= 1e-6
    composed = conv((xs.clone().requires_grad_(True), xd), ei, ea, residual=res, activation="relu")
    assert composed.requires_grad and _rel(composed.detach(), want) <= 1e-6


@pytest.mark.parametrize("route", ["materialised", "reassociated"])
def test_two_identical_calls_give_identical_bits(route, monkeypatch):
    if route == "reassociated":
        monkeypatch.setattr(ops, "ANY_REASSOC", "on")
    n_src, n_dst, cin, cout = 53, 37, 40, 24
    ei, _ = bip_graph(n_src, n_dst, seed=12)
    xs, xd, ea, g = inputs(n_src, n_dst, cin, cin, cout, ei.shape[1], seed=12)
    torch.manual_seed(12)
    conv = gp.NNConv(cin, cout, DenseNet([K0, 16, cin * cout]), aggr="add").to(dev())
    a, b = _train(conv, (xs, xd), ei, ea, g), _train(conv, (xs, xd), ei, ea, g)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---- 7. C ABI ------------------------------------------------------------------------------------------------------------------
def test_csr_from_coo2_counts_either_side_and_python_names_it():
    lib = _lib.lib()
    n_src, n_dst = 5, 9
    for bad_row, side in ((0, "source"), (1, "destination")):
        ei = torch.tensor([[0, 1, 2, 4], [0, 3, 8, 8]], dtype=torch.int64, device=dev())
        ei[bad_row, 2] = (n_src, n_dst)[bad_row]         # in range for the OTHER side when n_src < n_dst (row 0), out of range for its own
        e = ei.shape[1]
        rowptr = torch.empty(n_dst + 1, dtype=torch.int32, device=dev())
        src, dst, perm = (torch.empty(e, dtype=torch.int32, device=dev()) for _ in range(3))
        n_bad = torch.full((1,), -1, dtype=torch.int32, device=dev())
        nbytes = int(lib.gpde_csr_workspace_bytes(e, max(n_src, n_dst)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
        rc = lib.gpde_csr_from_coo2(ei.data_ptr(), ei.stride(0), ei.stride(1), e, n_src, n_dst, rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                    perm.data_ptr(), n_bad.data_ptr(), ws.data_ptr(), nbytes, ops._stream_ptr(dev()))
        assert rc == 0 and int(n_bad) == 1, (rc, int(n_bad))
        with pytest.raises(IndexError, match=side) as ei_err:
            ops.build_csr(ei, n_dst, n_src=n_src)
        assert ("destination" if side == "source" else "source") not in str(ei_err.value)
    # a square call gives the arrays of gpde_csr_from_coo bit for bit
    sq = torch.randint(0, 9, (2, 200), generator=torch.Generator().manual_seed(0)).to(dev())
    a, b = ops.build_csr(sq, 9), ops.build_csr(sq, 9, n_src=9)
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("rowptr", "src", "dst", "perm"))


def test_native_argument_errors():
    lib = _lib.lib()
    n_src, n_dst, cin, cout, e = 4, 6, 8, 8, 3
    d = dev()
    xs, xd, we = torch.randn(n_src, cin, device=d), torch.randn(n_dst, cin, device=d), torch.randn(e, cin * cout, device=d)
    root, out, g = torch.randn(cin, cout, device=d), torch.empty(n_dst, cout, device=d), torch.randn(n_dst, cout, device=d)
    csr = ops.build_csr(torch.tensor([[0, 1, 3], [5, 0, 0]], device=d), n_dst, n_src=n_src)
    st = ops._stream_ptr(d)
    fwd = lambda x_dst, in_dst: lib.gpde_nnconv_fwd_edgeweights_bip(xs.data_ptr(), n_src, x_dst, n_dst, we.data_ptr(), e, csr.rowptr.data_ptr(),
                                                                   csr.src.data_ptr(), root.data_ptr(), None, None, 0, _lib.GPDE_AGGR_ADD,
                                                                   cin, in_dst, cout, out.data_ptr(), st)
    assert fwd(None, cin) == -1 and b"x_dst" in lib.gpde_last_error()                 # GPDE_EINVAL: root without x_dst
    assert fwd(xd.data_ptr(), 257) == -2                                               # GPDE_EUNSUPPORTED: in_dst outside 1 .. 256
    assert fwd(xd.data_ptr(), cin) == 0
    nbytes = int(lib.gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(n_src, n_dst, e, cin, cin, cout))
    ws, gwe = torch.empty(nbytes, dtype=torch.uint8, device=d), torch.empty_like(we)
    bwd = lambda aggr: lib.gpde_nnconv_bwd_edgeweights_bip(xs.data_ptr(), n_src, xd.data_ptr(), n_dst, we.data_ptr(), e, csr.rowptr.data_ptr(),
                                                           csr.src.data_ptr(), None, None, root.data_ptr(), aggr, cin, cin, cout, g.data_ptr(),
                                                           None, None, gwe.data_ptr(), None, None, ws.data_ptr(), nbytes, st)
    assert bwd(_lib.GPDE_AGGR_MAX) == -2                                               # GPDE_EUNSUPPORTED
    assert bwd(_lib.GPDE_AGGR_ADD) == 0
    hid, wl = torch.randn(e, 5, device=d), torch.randn(cin * cout, 5, device=d)
    hb = int(lib.gpde_nnconv_fwd_hidden_bip_workspace_bytes(n_dst, e, cin, cout, 5))
    hws = torch.empty(hb, dtype=torch.uint8, device=d)
    hfwd = lambda x_dst, in_dst, aggr: lib.gpde_nnconv_fwd_hidden_bip(xs.data_ptr(), n_src, x_dst, n_dst, hid.data_ptr(), e, 5, csr.rowptr.data_ptr(),
                                                                      csr.src.data_ptr(), wl.data_ptr(), None, root.data_ptr(), None, aggr, cin,
                                                                      in_dst, cout, out.data_ptr(), hws.data_ptr(), hb, st)
    assert hfwd(None, cin, _lib.GPDE_AGGR_ADD) == -1 and hfwd(xd.data_ptr(), 257, _lib.GPDE_AGGR_ADD) == -2
    assert hfwd(xd.data_ptr(), cin, _lib.GPDE_AGGR_MAX) == -2 and hfwd(xd.data_ptr(), cin, _lib.GPDE_AGGR_ADD) == 0
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError):
        ops.nnconv_backward_edgeweights_bip_raw(xs, xd, csr, we, root, "max", g)
