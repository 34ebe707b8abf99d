"""GPU tier of GCNConv: ops.gcn_norm, ops.gcn_forward_raw (both routes), the autograd function and the module against the
float64 checker of tests/helpers/gcn_oracle.py.

Bars (the project's): forward 1e-5 relative L2 against float64 and the same bar row by row (|err_row| <= bar * max(|ref_row|, rms
row norm), the rule of tests/test_gpu_width_tilings.py); gradients 2e-5, a reduction over N (grad_W, grad_bias) that misses it is
held to max(2e-5, 4 * e32), e32 = the float32 torch chain's own distance from float64 on the same input.  Coefficients: 1e-6
relative unweighted (an exact integer degree and four roundings: <= 2.4e-7), (row length + 4) * 2^-24 weighted (the worst case of
a positive fp32 sum).  The float32 torch chain sits at 1e-7 .. 2.5e-7 row-wise on the ladder and at 5e-7 .. 1.6e-6 on the hub row:
the bars test addressing and tails, not luck."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from tests.helpers import gcn_oracle as go
from tests.helpers import layouts
from tests.test_gcn_host import plan_classes

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(REPO, "graph-pde_amd", "shims")
FWD_BAR, GRAD_BAR = 1e-5, 2e-5
WIDTHS = [(1, 1), (3, 5), (33, 65), (64, 64), (128, 128), (256, 130), (130, 256)]
NORM_OPTS = [dict(), dict(improved=True), dict(add_self_loops=False), dict(normalize=False)]


def dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def graph(name):
    ei, n = getattr(go, name)()
    return ei, n, go.weights_for(ei)


def native_norm(name, weighted=False, **kw):
    ei, n, ew = graph(name)
    csr = ops.csr_for(_dev_tensor(name, "ei"), n)
    return ops.gcn_norm(csr, _dev_tensor(name, "ew") if weighted else None, **kw)


@functools.lru_cache(maxsize=None)
def _dev_tensor(name, which):
    ei, n, ew = graph(name)
    return (ei if which == "ei" else ew).to(dev())


def _check_fwd(out, ref, tag):
    e, r = go.rel_l2(out, ref), go.row_excess(out, ref)
    print(f"{tag}: rel-L2 {e:.3e}, worst row {r:.3e}")
    assert e <= FWD_BAR and r <= FWD_BAR, (tag, e, r)


# ---- coefficients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "selfloops", "hub"])
@pytest.mark.parametrize("kw", NORM_OPTS, ids=str)
@pytest.mark.parametrize("weighted", [False, True])
def test_coefficients(name, kw, weighted):
    ei, n, ew = graph(name)
    ops._gcn_norm_cache.clear()
    norm = native_norm(name, weighted, **kw)
    csr = norm.csr
    perm = csr.perm.long().cpu()
    coef_ref, self_ref = go.coefficients(ei, n, ew if weighted else None, **kw)
    coef_ref, self_ref = torch.from_numpy(coef_ref)[perm], torch.from_numpy(self_ref)
    coef, selfc = norm.coef.double().cpu(), norm.self_coef.double().cpu()
    rp = csr.rowptr.long().cpu()
    rowlen = (rp[1:] - rp[:-1]).double()
    if weighted:
        tol_e, tol_n = (rowlen[csr.dst.long().cpu()] + 4) * 2.0 ** -24, (rowlen + 4) * 2.0 ** -24
    else:
        tol_e, tol_n = torch.full_like(coef_ref, 1e-6), torch.full_like(self_ref, 1e-6)
    worst = float(((coef - coef_ref).abs() / coef_ref.abs().clamp_min(1e-300)).max()) if coef.numel() else 0.0
    print(f"{name} {kw} weighted={weighted}: worst relative coefficient error {worst:.3e}")
    assert bool(((coef - coef_ref).abs() <= tol_e * coef_ref.abs()).all())
    assert bool(((selfc - self_ref).abs() <= tol_n * self_ref.abs()).all())
    if kw.get("normalize", True) and kw.get("add_self_loops", True):
        loops = (csr.src == csr.dst).cpu()
        assert bool((norm.coef.cpu()[loops] == 0).all()) and (name != "selfloops" or int(loops.sum()) > 90)
    if not kw.get("normalize", True) and weighted:
        assert torch.equal(norm.coef.cpu(), ew[perm])
    # two builds: the same bits
    ops._gcn_norm_cache.clear()
    again = native_norm(name, weighted, **kw)
    assert again is not norm and torch.equal(again.coef, norm.coef) and torch.equal(again.self_coef, norm.self_coef)


def test_norm_cache():
    ei, n, ew = graph("ladder")
    ei_d, ew_d = ei.to(dev()), ew.to(dev())
    csr = ops.csr_for(ei_d, n)
    a = ops.gcn_norm(csr, ew_d)
    calls = _lib.n_native_calls
    assert ops.gcn_norm(ops.csr_for(ei_d, n), ew_d) is a and _lib.n_native_calls == calls          # same tensors: a hit, no native call
    assert ops.gcn_norm(csr, ew_d, improved=True) is not a and _lib.n_native_calls == calls + 1    # the flags are part of the key
    ew_d.mul_(2.0)                                                                                  # an in-place edit: a miss
    b = ops.gcn_norm(csr, ew_d)
    assert b is not a and _lib.n_native_calls == calls + 2 and not torch.equal(b.coef, a.coef)
    rect = ops.csr_for(ei_d, n, n_src=n + 1)
    with pytest.raises(ValueError, match="one node set"):
        ops.gcn_norm(rect)


# ---- forward --------------------------------------------------------------------------------------------------------------------
def _fwd_case(name, cin, cout, route, bias=True, relu=False, weighted=False, seed=0, **kw):
    ei, n, ew = graph(name)
    g = torch.Generator().manual_seed(1000 * cin + cout + seed)
    x = torch.randn(n, cin, generator=g)
    w = torch.randn(cin, cout, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g) if bias else None
    norm = native_norm(name, weighted, **kw)
    out = ops.gcn_forward_raw(x.to(dev()), norm, w.to(dev()), None if b is None else b.to(dev()), relu=relu, route=route)
    ref = go.forward(x, ei, w, b, edge_weight=ew if weighted else None, relu=relu, **kw)
    return out, ref, x, w, b, norm


@pytest.mark.parametrize("name", ["ladder", "selfloops"])
@pytest.mark.parametrize("route", ops.GCN_ROUTES)
@pytest.mark.parametrize("cin,cout", WIDTHS)
def test_forward_widths(name, route, cin, cout):
    out, ref, *_ = _fwd_case(name, cin, cout, route)
    _check_fwd(out, ref, f"{name} {cin}->{cout} {route}")


@pytest.mark.parametrize("route", ops.GCN_ROUTES)
@pytest.mark.parametrize("cls", sorted(plan_classes().items()), ids=lambda c: "p{}w{}k{}c{}_{}x{}".format(*c[0], *c[1]))
def test_forward_every_plan_class(route, cls):
    """One width pair per tiling class gpde_gcn_plan reports (channel passes, column blocks per wave, K tail, column tail)."""
    (cin, cout) = cls[1]
    p = ops.gcn_plan(cin, cout)
    assert (p["passes"], p["col_blocks_per_wave"], p["k_tail"], p["col_tail"]) == cls[0]
    out, ref, *_ = _fwd_case("selfloops", cin, cout, route, weighted=True)
    _check_fwd(out, ref, f"class {cls[0]} {cin}->{cout} {route}")


@pytest.mark.parametrize("route", ops.GCN_ROUTES)
@pytest.mark.parametrize("opt", [dict(bias=False), dict(relu=True), dict(weighted=True), dict(bias=False, relu=True, weighted=True),
                                 dict(improved=True), dict(add_self_loops=False, weighted=True), dict(normalize=False, weighted=True)], ids=str)
@pytest.mark.parametrize("cin,cout", [(33, 65), (128, 128)])
def test_forward_options(route, opt, cin, cout):
    out, ref, *_ = _fwd_case("selfloops", cin, cout, route, **opt)
    _check_fwd(out, ref, f"{opt} {cin}->{cout} {route}")
    if opt.get("relu"):
        assert float(out.min()) == 0.0


@pytest.mark.parametrize("c", [1, 3, 64, 65, 130, 256])
def test_pure_aggregation(c):
    """W = NULL: out = A x (+ bias, ReLU) at width c."""
    ei, n, ew = graph("selfloops")
    g = torch.Generator().manual_seed(c)
    x, b = torch.randn(n, c, generator=g), torch.randn(c, generator=g)
    norm = native_norm("selfloops", True)
    out = ops.gcn_forward_raw(x.to(dev()), norm, None, b.to(dev()), relu=True)
    _check_fwd(out, go.forward(x, ei, None, b, edge_weight=ew, relu=True), f"aggregation at {c}")
    out2 = ops.gcn_forward_raw(x.to(dev()), norm, None)
    _check_fwd(out2, go.forward(x, ei, None, None, edge_weight=ew), f"aggregation at {c}, no bias")
    with pytest.raises(ValueError, match="route"):
        ops.gcn_forward_raw(x.to(dev()), norm, None, route="fused")


@pytest.mark.parametrize("route", ops.GCN_ROUTES)
def test_rows_without_in_edges(route):
    ei, n, _ = graph("ladder")
    empty = [i for i in range(n) if i % 70 == 0]
    out, ref, x, w, b, norm = _fwd_case("ladder", 33, 65, route)
    selfc = torch.from_numpy(go.coefficients(ei, n)[1])
    want = (selfc[empty].view(-1, 1) * x[empty].double()) @ w.double() + b.double()             # self_coef x W + b
    assert go.rel_l2(out[empty], want) <= FWD_BAR
    out0, ref0, x, w, b, _ = _fwd_case("ladder", 33, 65, route, add_self_loops=False)
    assert torch.equal(out0[empty].cpu(), b.expand(len(empty), -1))                              # no self loop: exactly the bias
    _check_fwd(out0, ref0, f"ladder without self loops {route}")


def test_two_forward_calls_give_the_same_bits_and_routes_agree():
    a, ref, x, w, b, norm = _fwd_case("selfloops", 128, 128, "aggregate_first")
    again = ops.gcn_forward_raw(x.to(dev()), norm, w.to(dev()), b.to(dev()), route="aggregate_first")
    assert torch.equal(a, again)
    for other in ("aggregate_mm", "transform_first"):
        t = ops.gcn_forward_raw(x.to(dev()), norm, w.to(dev()), b.to(dev()), route=other)
        assert go.rel_l2(t, a) <= 2 * FWD_BAR
        assert torch.equal(t, ops.gcn_forward_raw(x.to(dev()), norm, w.to(dev()), b.to(dev()), route=other))
    for r in ("aggregate_first", "aggregate_mm"):
        out, agg = ops.gcn_forward_raw(x.to(dev()), norm, w.to(dev()), b.to(dev()), route=r, agg_out=True)
        assert torch.equal(agg, ops.gcn_forward_raw(x.to(dev()), norm, None)) and (r != "aggregate_first" or torch.equal(out, a))
    with pytest.raises(ValueError, match="agg_out"):
        ops.gcn_forward_raw(x.to(dev()), norm, w.to(dev()), route="transform_first", agg_out=True)
    with pytest.raises(ValueError):
        ops.gcn_forward_raw(x.to(dev())[:, :100], norm, w.to(dev()))                              # weight of another width
    with pytest.raises(ValueError):
        ops.gcn_forward_raw(x.double().to(dev()), norm, w.to(dev()))


# ---- gradients ------------------------------------------------------------------------------------------------------------------
def _grad_case(name, cin, cout, route, weighted=False, **kw):
    ei, n, ew = graph(name)
    g = torch.Generator().manual_seed(77 * cin + cout)
    x = torch.randn(n, cin, generator=g)
    w = torch.randn(cin, cout, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    go_ = torch.randn(n, cout, generator=g)
    xd, wd, bd = (t.to(dev()).requires_grad_(True) for t in (x, w, b))
    norm = native_norm(name, weighted, **kw)
    out = gp.autograd.GCNFunction.apply(xd, wd, bd, norm, route)
    out.backward(go_.to(dev()))
    okw = dict(edge_weight=ew if weighted else None, **kw)
    ref = go.gradients(x, ei, w, b, go_, **okw)
    return (out, xd.grad, wd.grad, bd.grad), ref, (x, ei, w, b, go_, okw)


def _check_grads(got, ref, inputs, tag):
    out, gx, gw, gb = got
    rout, rgx, rgw, rgb = ref
    _check_fwd(out, rout, tag)
    ex, rx = go.rel_l2(gx, rgx), go.row_excess(gx, rgx)
    ew_, eb = go.rel_l2(gw, rgw), go.rel_l2(gb, rgb)
    print(f"{tag}: grad_x {ex:.3e} (worst row {rx:.3e}), grad_W {ew_:.3e}, grad_bias {eb:.3e}")
    assert ex <= GRAD_BAR and rx <= GRAD_BAR, (tag, ex, rx)
    bar_w = bar_b = GRAD_BAR
    if ew_ > GRAD_BAR or eb > GRAD_BAR:                   # a reduction over N: the float32 chain's own distance is the yardstick
        x, ei, w, b, go_, okw = inputs
        _, _, c32w, c32b = go.chain32(x, ei, w, b, go_, **okw)
        if ew_ > GRAD_BAR:                                # (only the gradient that missed gets the wider bar)
            bar_w = max(GRAD_BAR, 4 * go.rel_l2(c32w, rgw))
        if eb > GRAD_BAR:
            bar_b = max(GRAD_BAR, 4 * go.rel_l2(c32b, rgb))
        print(f"{tag}: e32 bars grad_W {bar_w:.3e}, grad_bias {bar_b:.3e}")
    assert ew_ <= bar_w and eb <= bar_b, (tag, ew_, bar_w, eb, bar_b)


@pytest.mark.parametrize("name", ["ladder", "selfloops", "directed"])
@pytest.mark.parametrize("route", ops.GCN_ROUTES)
@pytest.mark.parametrize("cin,cout", [(3, 5), (33, 65), (64, 64), (130, 33)])
def test_backward(name, route, cin, cout):
    """`directed` has no reverse edges: a backward that aggregated over the forward CSR would pass on the symmetric graphs and
    fails here."""
    got, ref, inputs = _grad_case(name, cin, cout, route, weighted=(name == "selfloops"))
    _check_grads(got, ref, inputs, f"{name} {cin}->{cout} {route}")


def test_directed_graph_is_not_its_own_transpose():
    """The check above has teeth: on `directed`, aggregating grad_out over the FORWARD graph is far from grad_x."""
    ei, n, _ = graph("directed")
    x, w = torch.randn(n, 8), torch.randn(8, 8)
    g = torch.randn(n, 8)
    _, rgx, _, _ = go.gradients(x, ei, w, None, g)
    wrong = go.forward(g, ei, w.t().contiguous())
    assert go.rel_l2(wrong, rgx) > 0.1


@pytest.mark.parametrize("cin,cout", [(3, 5), (33, 65), (128, 128)])
def test_hub(cin, cout):
    """A destination row of 8,192 in-edges (node 3) and, for the backward, a source with 8,192 out-edges (node 5)."""
    for route in ops.GCN_ROUTES:
        got, ref, inputs = _grad_case("hub", cin, cout, route)
        _check_grads(got, ref, inputs, f"hub {cin}->{cout} {route}")
        assert float(((got[0][3].detach().double().cpu() - ref[0][3]).norm() / ref[0][3].norm())) <= FWD_BAR        # the hub row itself


@pytest.mark.parametrize("route", [None, "aggregate_first"])
def test_needs_input_grad_and_reproducibility(route):
    ei, n, _ = graph("directed")
    norm = native_norm("directed")
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(n, 33, generator=g).to(dev()), torch.randn(33, 65, generator=g).to(dev()), torch.randn(65, generator=g).to(dev())
    go_ = torch.randn(n, 65, generator=g).to(dev())
    norm.reversed                                           # (built here: the counts below are those of the backward alone)

    def run(rx, rw, rb):
        xs, ws, bs = x.clone().requires_grad_(rx), w.clone().requires_grad_(rw), b.clone().requires_grad_(rb)
        out = gp.autograd.GCNFunction.apply(xs, ws, bs, norm, route)
        calls = _lib.n_native_calls
        out.backward(go_)
        return xs.grad, ws.grad, bs.grad, _lib.n_native_calls - calls
    full = run(True, True, True)
    assert full[3] == 1                                     # ONE native launch, A^T g, under every route
    again = run(True, True, True)
    assert all(torch.equal(a, b_) for a, b_ in zip(full[:3], again[:3]))
    gx, gw, gb, calls = run(True, False, False)
    assert torch.equal(gx, full[0]) and gw is None and gb is None and calls == 1
    gx, gw, gb, calls = run(False, True, False)
    assert gx is None and gb is None and calls == 1 and go.rel_l2(gw, full[1]) <= 1e-6
    gx, gw, gb, calls = run(False, False, True)
    assert gx is None and gw is None and calls == 0 and torch.equal(gb, full[2])       # the kernel is skipped
    conv = gp.GCNConv(33, 65).to(dev())
    with pytest.raises(NotImplementedError, match="edge_weight"):
        conv(x, ei.to(dev()), torch.ones(ei.size(1), device=dev(), requires_grad=True))


# ---- module ---------------------------------------------------------------------------------------------------------------------
class TwoLayer(torch.nn.Module):
    def __init__(self, cin=6, hid=33, cout=4, **kw):
        super().__init__()
        self.c1, self.c2 = gp.GCNConv(cin, hid, **kw), gp.GCNConv(hid, cout, **kw)

    def forward(self, x, ei, ew=None):
        return self.c2(F.relu(self.c1(x, ei, ew)), ei, ew)


def test_two_layer_net_on_the_strided_grid_equals_the_host_path():
    torch.manual_seed(3)
    ei, n = go.grid()
    net = TwoLayer()
    with torch.no_grad():
        net.c1.bias.uniform_(-1, 1)
        net.c2.bias.uniform_(-1, 1)
    x, y = torch.randn(n, 6), torch.randn(n, 4)
    loss_h = F.mse_loss(net(x, ei), y)
    loss_h.backward()
    host = [p.grad.clone() for p in net.parameters()]
    net.zero_grad()
    net_d = net.to(dev())
    ei_d = ei.contiguous().to(dev()).t().contiguous().t()   # [2, E] with strides (1, 2) on the device
    assert not ei_d.is_contiguous()
    calls = _lib.n_native_calls
    loss_d = F.mse_loss(net_d(x.to(dev()), ei_d), y.to(dev()))
    loss_d.backward()
    assert _lib.n_native_calls > calls
    assert abs(float(loss_d) - float(loss_h)) <= 1e-5 * abs(float(loss_h))
    for p, h in zip(net_d.parameters(), host):
        assert go.rel_l2(p.grad, h) <= 1e-5
    net.cpu()


@pytest.fixture(scope="module")
def shim_data():
    sys.path.insert(0, SHIMS)
    from torch_geometric.data import Data, DataLoader
    from torch_geometric.nn import GCNConv
    yield Data, DataLoader, GCNConv
    sys.path.remove(SHIMS)


def test_a_batch_of_two_graphs_equals_the_two_graphs(shim_data):
    Data, DataLoader, GCNConv = shim_data
    assert GCNConv is gp.GCNConv
    torch.manual_seed(4)
    (e1, n1), (e2, n2) = go.grid(), go.directed()
    x1, x2 = torch.randn(n1, 6), torch.randn(n2, 6)
    net = TwoLayer().to(dev())
    batch = next(iter(DataLoader([Data(x=x1, edge_index=e1.contiguous()), Data(x=x2, edge_index=e2)], batch_size=2, shuffle=False))).to(dev())
    with torch.no_grad():
        both = net(batch.x, batch.edge_index)
        a, b = net(x1.to(dev()), e1.to(dev())), net(x2.to(dev()), e2.to(dev()))
    assert both.shape == (n1 + n2, 4) and go.rel_l2(both, torch.cat([a, b])) <= 1e-6


def test_cached_flow_and_csr_inputs():
    torch.manual_seed(5)
    (e1, n1), (e2, _) = go.directed(), go.directed(seed=9)
    e1, e2 = e1.to(dev()), e2.to(dev())
    x = torch.randn(n1, 6, device=dev())
    plain, cached, t2s = gp.GCNConv(6, 9).to(dev()), gp.GCNConv(6, 9, cached=True).to(dev()), gp.GCNConv(6, 9, flow="target_to_source").to(dev())
    cached.load_state_dict(plain.state_dict())
    t2s.load_state_dict(plain.state_dict())
    with torch.no_grad():
        first = cached(x, e1)
        assert torch.equal(first, plain(x, e1))
        assert torch.equal(cached(x, e2), first) and not torch.equal(plain(x, e2), first)       # pinned / not pinned
        assert torch.equal(t2s(x, e1), plain(x, e1.flip(0)))
        assert go.rel_l2(t2s(x, e1), go.forward(x.cpu(), e1.cpu().flip(0), plain.weight.cpu(), plain.bias.cpu())) <= FWD_BAR
        assert torch.equal(plain(x, ops.csr_for(e1, n1)), plain(x, e1))                         # an ops.Csr as the graph
        assert torch.equal(t2s(x, ops.csr_for(e1, n1, flip=True)), t2s(x, e1))                  # ... built for the module's flow
        with pytest.raises(ValueError, match="flip=True"):
            t2s(x, ops.csr_for(e1, n1))
        moved = cached.cpu()                                                                    # a cached module moved to the host and back
        assert go.rel_l2(moved(x.cpu(), e1.cpu()), first) <= FWD_BAR
        assert torch.equal(moved.to(dev())(x, e2), first)
        with pytest.raises(ValueError, match="weight"):
            ops.gcn_forward_raw(x, ops.gcn_norm(ops.csr_for(e1, n1)), torch.zeros(6, device=dev()))
        xv = torch.randn(n1, device=dev())
        one = gp.GCNConv(1, 3).to(dev())
        assert torch.equal(one(xv, e1), one(xv.view(-1, 1), e1))                                # one-dimensional x is [N, 1]


def test_capture_replays_the_same_bits():
    torch.manual_seed(6)
    ei, n = go.ladder()
    ei = ei.to(dev())
    net = TwoLayer(8, 64, 8).to(dev())
    x = torch.randn(n, 8, device=dev())
    with torch.no_grad():
        direct = net(x, ei)
        fwd = gp.capture(lambda t: net(t, ei), x)
        assert torch.equal(fwd(x), direct)
        x2 = torch.randn(n, 8, device=dev())
        assert torch.equal(fwd(x2), net(x2, ei)) and fwd.replays == 2


# ---- operand layouts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k in layouts.AWKWARD if k != "expanded"])
@pytest.mark.parametrize("route", ops.GCN_ROUTES)
def test_operand_layouts(kind, route):
    ei, n, _ = graph("selfloops")
    norm = native_norm("selfloops")
    g = torch.Generator().manual_seed(8)
    x, w, b = (t.to(dev()) for t in (torch.randn(n, 33, generator=g), torch.randn(33, 65, generator=g), torch.randn(65, generator=g)))
    go_ = torch.randn(n, 65, generator=g).to(dev())

    def run(xv, wv, gv):
        xs, ws, bs = xv.detach().requires_grad_(True), wv.detach().requires_grad_(True), b.clone().requires_grad_(True)
        out = gp.autograd.GCNFunction.apply(xs, ws, bs, norm, route)
        out.backward(gv)
        return out.detach(), xs.grad, ws.grad, bs.grad
    base = run(x, w, go_)
    (xv, xb), (wv, wb), (gv, gb) = (layouts.as_layout(t, kind) for t in (x, w, go_))
    got = run(xv, wv, gv)
    for a, r in zip(got, base):
        assert go.rel_l2(a, r) <= 1e-6
    for bk in (xb, wb, gb):
        layouts.guards_intact(bk)


def test_expanded_grad_out():
    """grad_out of `out.sum()` is one value with stride 0 in both dimensions."""
    ei, n, _ = graph("ladder")
    conv = gp.GCNConv(33, 65).to(dev())
    x = torch.randn(n, 33, device=dev(), requires_grad=True)
    conv(x, ei.to(dev())).sum().backward()
    _, gx, gw, gb = go.gradients(x, ei, conv.weight, conv.bias, torch.ones(n, 65))
    assert go.rel_l2(x.grad, gx) <= GRAD_BAR and go.rel_l2(conv.weight.grad, gw) <= GRAD_BAR and go.rel_l2(conv.bias.grad, gb) <= GRAD_BAR
