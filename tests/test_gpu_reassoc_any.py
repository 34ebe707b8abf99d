"""GPU tier: the RE-ASSOCIATED any-width NNConv (csrc/gpde_reassoc_any.hip: gpde_nnconv_fwd_hidden_any / gpde_nnconv_bwd_hidden_any).

A module whose widths are not (64, 64), whose `nn` is a Linear / ReLU chain and whose aggregation is add / mean can run without
the [E, in * out] per-edge weights: torch evaluates the hidden layers, the native call aggregates x_j (x) h_e per node and applies
the last Linear per node.  The route is chosen by ops.ANY_REASSOC (`on` here; `auto` only re-routes calls that were refused).
Bars: the project's own (tests/test_gpu_widths.py) - relative L2 against float64 <= 1e-5 forward, <= 2e-5 every gradient, and the
worst destination row among rows with in-degree >= 1 <= 1e-5.  Every test prints the figures it asserts on (-s shows them)."""
import copy

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops, synth
from oracle.nnconv_oracle import nnconv_forward, nnconv_grads
from tests.conftest import load_golden
from tests.helpers.any_tilings import worst_row
from tests.test_gpu_widths import DenseNet, DenseNetSin, _linears, _rel
from tests.test_oracle_golden import load_golden_grads

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD, TOL_ROW = 1e-5, 2e-5, 1e-5
LADDER = (0, 1, 2, 3, 5, 8, 17, 33, 64, 65, 130)


@pytest.fixture
def route_on(monkeypatch):
    monkeypatch.setattr(ops, "ANY_REASSOC", "on")


@pytest.fixture
def native_trace(monkeypatch):
    """Names of the any-width native entry points a test's calls went through, in order."""
    trace = []
    for name in ("nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw", "nnconv_forward_edgeweights_any_raw",
                 "nnconv_backward_edgeweights_any_raw"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            trace.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return trace


def ladder(device, seed=0, hub=None):
    """(edge_index in no sorted order, edge_attr [E, 6], n_nodes, in-degree per node): destinations of in-degree 0, 1, 2, 3, 5, 8, 17,
    33, 64, 65, 130 in a shuffled node order (`hub`: one more of that in-degree), self-loops, duplicates of one edge into the longest
    row, two trailing isolated nodes."""
    g = torch.Generator().manual_seed(seed)
    degs = LADDER + ((hub,) if hub else ())
    nd = len(degs)
    n = nd + 2
    order = torch.randperm(nd, generator=g).tolist()
    dst = torch.tensor([order[k] for k, d in enumerate(degs) for _ in range(d)], dtype=torch.int64)
    e = dst.numel()
    src = torch.randint(0, nd, (e,), generator=g)
    src[:20] = dst[:20]                                     # self-loops
    big = order[nd - 1]
    src[(dst == big).nonzero().flatten()[:10]] = (big + 1) % nd      # 10 copies of one edge
    perm = torch.randperm(e, generator=g)
    deg = torch.bincount(dst, minlength=n)
    return torch.stack([src[perm], dst[perm]]).to(device), torch.rand(e, 6, generator=g)[perm].to(device), n, deg


def _step(conv, x, ei, ea, aggr, tag, deg=None, chunk_edges=None):
    """One training step of `conv` against oracle.nnconv_forward(float64) / oracle.nnconv_grads: exactly two native calls, every bar.
    Returns (out, [gradients])."""
    lin = _linears(conv.nn)
    g = torch.randn(x.shape[0], conv.out_channels, device=x.device)
    conv.zero_grad()
    xin = x.clone().requires_grad_(True)
    calls0 = _lib.n_native_calls
    out = conv(xin, ei, ea)
    (out * g).sum().backward()
    ncalls = _lib.n_native_calls - calls0
    Ws, Bs = [l.weight for l in lin], [l.bias for l in lin]
    ref = nnconv_forward(x, ei, ea, Ws, Bs, conv.root, conv.bias, aggr=aggr, dtype=torch.float64, **({"chunk_edges": chunk_edges} if chunk_edges else {}))
    x2 = x.unsqueeze(-1) if x.dim() == 1 else x
    gx, gW, gb, groot, gbias = nnconv_grads(x2.cpu(), ei.cpu(), ea.cpu(), [w.detach().cpu() for w in Ws], [b.detach().cpu() for b in Bs],
                                            None if conv.root is None else conv.root.detach().cpu(),
                                            None if conv.bias is None else conv.bias.detach().cpu(), aggr, g.cpu(), chunk_edges=chunk_edges)
    errs = {"out": _rel(out.detach(), ref), "gx": _rel(xin.grad.reshape(gx.shape), gx)}
    if deg is not None:
        rows = (deg >= 1).nonzero().flatten()
        errs["row"] = worst_row(out.detach().cpu()[rows], ref[rows])
    for l, layer in enumerate(lin):
        errs[f"gW{l}"], errs[f"gb{l}"] = _rel(layer.weight.grad, gW[l]), _rel(layer.bias.grad, gb[l])
    if conv.root is not None:
        errs["groot"] = _rel(conv.root.grad, groot)
    if conv.bias is not None:
        errs["gbias"] = _rel(conv.bias.grad, gbias)
    print(f"[reassoc] {tag}: calls={ncalls} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert ncalls == 2, ncalls                                   # one native forward, one native backward
    assert out.shape == (x.shape[0], conv.out_channels)
    assert errs["out"] <= TOL_FWD, errs
    assert errs.get("row", 0.0) <= TOL_ROW, errs
    assert all(v <= TOL_BWD for k, v in errs.items() if k not in ("out", "row")), errs
    return out.detach(), [xin.grad.clone()] + [p.grad.clone() for p in conv.parameters()]


# every width class x every last hidden width of {1, 7, 32, 33, 100} (each side of a 4-float vector and of a 32-lane boundary; K = 8
# alone at 256 -> 256) x a 2- and a 3-Linear chain - and, below, add and mean: 8 * 5 * 2 * 2 + 1 * 1 * 2 * 2 = 164 cases of ~ 330 edges
WIDTHS = [(1, 1), (3, 5), (24, 40), (40, 24), (65, 64), (64, 63), (7, 64), (128, 96), (256, 256)]
HIDDEN = (1, 7, 32, 33, 100)
CASES = [(cin, cout, k, nl) for cin, cout in WIDTHS for k in ((8,) if (cin, cout) == (256, 256) else HIDDEN) for nl in (2, 3)]


@pytest.mark.parametrize("aggr", ["mean", "add"])
@pytest.mark.parametrize("cin,cout,k,n_linear", CASES)
def test_width_and_hidden_width_classes_vs_float64_oracle(cin, cout, k, n_linear, aggr, route_on, native_trace):
    d = torch.device("cuda:0")
    torch.manual_seed(cin * 1000 + cout + k)
    ei, ea, n, deg = ladder(d, seed=cin + cout + k)
    dims = [6, k, cin * cout] if n_linear == 2 else [6, 12, k, cin * cout]
    conv = gp.NNConv_old(cin, cout, DenseNet(dims), aggr=aggr).to(d)
    _step(conv, torch.randn(n, cin, device=d), ei, ea, aggr, f"{cin}->{cout} K={k} {n_linear}-Linear {aggr}", deg=deg)
    assert native_trace == ["nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw"], native_trace


@pytest.mark.parametrize("cin,cout,k", [(24, 40, 33), (128, 96, 64)])
def test_hub_row_of_8192_in_edges(cin, cout, k, route_on):
    """One destination with 8,192 in-edges: sequential fp32 summation failed the row-by-row bar at this length before the
    any-width forward summed two-level; the aggregation of Z' sums a pass of 32 in-edges on its own."""
    d = torch.device("cuda:0")
    torch.manual_seed(41)
    ei, ea, n, deg = ladder(d, seed=7, hub=8192)
    conv = gp.NNConv_old(cin, cout, DenseNet([6, 16, k, cin * cout]), aggr="add").to(d)
    _step(conv, torch.randn(n, cin, device=d), ei, ea, "add", f"hub 8192 {cin}->{cout} K={k}", deg=deg, chunk_edges=1024)


def _raw_case(d, cin=24, cout=40, k=33, seed=3):
    torch.manual_seed(seed)
    ei, ea, n, deg = ladder(d, seed=seed)
    csr = ops.csr_for(ei, n)
    e = csr.n_edges
    x, h = torch.randn(n, cin, device=d), torch.relu(torch.randn(e, k, device=d))      # h: rows in CSR slot order
    wl, bl = torch.randn(cin * cout, k, device=d) / (cin * k) ** 0.5, torch.randn(cin * cout, device=d) / cin ** 0.5
    root, bias, g = torch.randn(cin, cout, device=d) / cin ** 0.5, torch.randn(cout, device=d), torch.randn(n, cout, device=d)
    return csr, n, e, x, h, wl, bl, root, bias, g


def _raw_reference64(csr, x, h, wl, bl, root, bias, g, aggr):
    """float64 autograd through the operator given H (CSR slot order): out and the gradients of x, H, w_last, b_last, root, bias."""
    cin, cout = root.shape
    leaves = [t.double().cpu().requires_grad_(True) for t in (x, h, wl, bl, root, bias)]
    x6, h6, wl6, bl6, r6, b6 = leaves
    src, rowptr = csr.src.long().cpu(), csr.rowptr.long().cpu()
    dst = torch.repeat_interleave(torch.arange(csr.n_nodes), rowptr[1:] - rowptr[:-1])
    w = (h6 @ wl6.t() + bl6).view(-1, cin, cout)
    m = torch.matmul(x6[src].unsqueeze(1), w).squeeze(1)
    out = torch.zeros(csr.n_nodes, cout, dtype=torch.float64).index_add(0, dst, m)
    if aggr == "mean":
        out = out / (rowptr[1:] - rowptr[:-1]).clamp(min=1).double().unsqueeze(1)
    out = out + x6 @ r6 + b6
    (out * g.double().cpu()).sum().backward()
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_node_blocks_of_the_raw_operator(aggr):
    """The raw ops in workspaces that force 1, 2 and N node blocks (N blocks = one node each): out, grad_x, grad_hidden bitwise
    equal across block counts; grad_w_last / grad_b_last (summed over the blocks in order) within 2e-5 of float64 each; two
    identical calls bitwise equal in every output; less than one node's worth of workspace is refused."""
    d = torch.device("cuda:0")
    cin, cout, k = 24, 40, 33
    csr, n, e, x, h, wl, bl, root, bias, g = _raw_case(d, cin, cout, k)
    lib = _lib.lib()
    ref_out, ref_g = _raw_reference64(csr, x, h, wl, bl, root, bias, g, aggr)
    runs = {}
    for label, block in (("1", n), ("2", (n + 1) // 2), ("N", 1)):
        wf = int(lib.gpde_nnconv_fwd_hidden_any_workspace_bytes(block, e, cin, cout, k))
        wb = int(lib.gpde_nnconv_bwd_hidden_any_workspace_bytes(block, e, cin, cout, k))
        two = []
        for _ in range(2):
            out = ops.nnconv_forward_hidden_any_raw(x, csr, h, wl, bl, root, bias, aggr, ws_bytes=wf)
            two.append((out,) + ops.nnconv_backward_hidden_any_raw(x, csr, h, wl, bl, root, aggr, g, ws_bytes=wb))
        for u, v in zip(*two):
            assert torch.equal(u, v), label                      # two identical calls: identical bits
        runs[label] = two[0]
        errs = {nm: _rel(t, r) for nm, t, r in zip(("out", "gx", "gh", "gwl", "gbl", "groot", "gbias"), two[0], [ref_out] + ref_g)}
        print(f"[reassoc] node blocks {aggr} {label}: " + " ".join(f"{a}={b:.2e}" for a, b in errs.items()))
        assert errs["out"] <= TOL_FWD and all(v <= TOL_BWD for a, v in errs.items() if a != "out"), errs
    for label in ("2", "N"):
        for idx, nm in ((0, "out"), (1, "grad_x"), (2, "grad_hidden")):
            assert torch.equal(runs[label][idx], runs["1"][idx]), (label, nm)
    with pytest.raises(_lib.GpdeError):
        ops.nnconv_forward_hidden_any_raw(x, csr, h, wl, bl, root, bias, aggr,
                                          ws_bytes=int(lib.gpde_nnconv_fwd_hidden_any_workspace_bytes(1, e, cin, cout, k)) - 1)
    with pytest.raises(_lib.GpdeError):
        ops.nnconv_backward_hidden_any_raw(x, csr, h, wl, bl, root, aggr, g,
                                           ws_bytes=int(lib.gpde_nnconv_bwd_hidden_any_workspace_bytes(1, e, cin, cout, k)) - 1)


@pytest.mark.parametrize("name,cin,cout", [("nnconv_rect_24x40_mean", 24, 40), ("nnconv_rect_40x24_add", 40, 24), ("nnconv_rect_1x8_mean", 1, 8)])
def test_reference_made_fixtures_on_the_new_route(name, cin, cout, route_on, native_trace):
    """The reference's own NNConv_old + DenseNet at in != out (tests/golden/make_golden_widths.py): out_f64 and every stored gradient."""
    d = torch.device("cuda:0")
    g, r = load_golden(name), load_golden_grads(name)
    dims = [g["weights"][0].shape[1]] + [w.shape[0] for w in g["weights"]]
    conv = gp.NNConv_old(cin, cout, DenseNet(dims), aggr=g["aggr"], root_weight=g["root"] is not None, bias=g["bias"] is not None)
    with torch.no_grad():
        for l, w, b in zip(_linears(conv.nn), g["weights"], g["biases"]):
            l.weight.copy_(w)
            l.bias.copy_(b)
        if g["root"] is not None:
            conv.root.copy_(g["root"])
        if g["bias"] is not None:
            conv.bias.copy_(g["bias"])
    conv = conv.to(d)
    x = g["x"].to(d).requires_grad_(True)
    out = conv(x, g["edge_index"].to(d), g["edge_attr"].to(d))
    (out * r["gout"].to(d)).sum().backward()
    assert native_trace == ["nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw"], native_trace
    errs = {"out": _rel(out.detach(), g["out_f64"]), "gx": _rel(x.grad, r["gx"])}
    for l, layer in enumerate(_linears(conv.nn)):
        errs[f"gW{l}"], errs[f"gb{l}"] = _rel(layer.weight.grad, r["gW"][l]), _rel(layer.bias.grad, r["gb"][l])
    if r["groot"] is not None:
        errs["groot"] = _rel(conv.root.grad, r["groot"])
    if r["gbias"] is not None:
        errs["gbias"] = _rel(conv.bias.grad, r["gbias"])
    print(f"[reassoc] fixture {name}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= TOL_FWD and all(v <= TOL_BWD for k, v in errs.items() if k != "out"), errs


def test_routing_on_the_device(monkeypatch, native_trace):
    """auto: a call whose per-edge weights do not fit (2 E in out 4 > free) while the re-associated bytes do takes the new route
    instead of raising; off raises as before; with the true free bytes auto is bitwise off."""
    d = torch.device("cuda:0")
    torch.manual_seed(51)
    cin = cout = 128
    ei, ea, n = synth.darcy_graph(8, 0.3, device=d)
    conv = gp.NNConv_old(cin, cout, DenseNet([6, 16, cin * cout]), aggr="mean").to(d)
    x = torch.randn(n, cin, device=d)
    with torch.no_grad():
        monkeypatch.setattr(ops, "ANY_REASSOC", "off")
        y_off = conv(x, ei, ea)
        monkeypatch.setattr(ops, "ANY_REASSOC", "auto")
        y_auto = conv(x, ei, ea)
    assert native_trace == ["nnconv_forward_edgeweights_any_raw"] * 2 and torch.equal(y_off, y_auto)
    e = ei.shape[1]
    true_free = ops.device_free_bytes
    fake = e * cin * cout * 4                                    # the per-edge weights once: twice that does not fit
    monkeypatch.setattr(ops, "device_free_bytes", lambda dev: (fake, true_free(dev)[1]))
    r = ops.any_width_route(n, e, cin, cout, 16, "mean", True, fake, mode="auto")
    assert r["route"] == "reassociated" and 2 * r["bytes_materialised"] > fake >= 2 * r["bytes_reassociated"], r
    del native_trace[:]
    _step(conv, x, ei, ea, "mean", "routing auto, per-edge weights do not fit 128->128 K=16")
    assert native_trace == ["nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw"], native_trace
    monkeypatch.setattr(ops, "ANY_REASSOC", "off")
    with pytest.raises(RuntimeError, match="materialised"):
        conv(x, ei, ea)
    monkeypatch.setattr(ops, "ANY_REASSOC", "auto")
    monkeypatch.setattr(ops, "device_free_bytes", lambda dev: (1024, true_free(dev)[1]))
    with pytest.raises(RuntimeError, match="re-associated"):     # neither fits: both sizes named
        conv(x, ei, ea)


@pytest.mark.parametrize("kind", ["max", "sin", "64"])
def test_fall_through_is_bitwise_what_off_gives(kind, monkeypatch, native_trace):
    """aggr='max', a network that is no Linear / ReLU chain and a 64 -> 64 module are not re-associated under `on`: the same native
    calls and, bit for bit, the same outputs (inference and the training forward).  Gradients: bitwise where the backward is the
    native one; a training step under 'max' is PyG's chain over message() / update() (MessagePassing.propagate), whose
    `x.index_select` is differentiated by torch with fp32 atomics - two runs of ONE mode differ in grad_x at the last bit there,
    so those gradients are compared to 1e-6 of their norm."""
    d = torch.device("cuda:0")
    torch.manual_seed(61)
    ei, ea, n = synth.darcy_graph(8, 0.3, device=d)
    if kind == "max":
        conv = gp.NNConv_old(24, 40, DenseNet([6, 16, 960]), aggr="max").to(d)
    elif kind == "sin":
        conv = gp.NNConv_old(24, 40, DenseNetSin([6, 16, 960]), aggr="mean").to(d)
    else:
        conv = gp.NNConv_old(64, 64, DenseNet([6, 32, 4096]), aggr="mean").to(d)
    x = torch.randn(n, conv.in_channels, device=d)
    res = {}
    for mode in ("off", "on"):
        monkeypatch.setattr(ops, "ANY_REASSOC", mode)
        with torch.no_grad():
            y = conv(x, ei, ea)
        conv.zero_grad()
        xin = x.clone().requires_grad_(True)
        yt = conv(xin, ei, ea)
        yt.sum().backward()
        res[mode] = ([y, yt.detach()], [xin.grad.clone()] + [p.grad.clone() for p in conv.parameters()], list(native_trace))
        del native_trace[:]
    assert res["off"][2] == res["on"][2] and not any("hidden_any" in t for t in res["on"][2]), res["on"][2]
    for u, v in zip(res["off"][0], res["on"][0]):
        assert torch.equal(u, v)
    worst = max(_rel(u, v) for u, v in zip(res["on"][1], res["off"][1]))
    print(f"[reassoc] fall-through {kind}: gradients on vs off, worst relative difference {worst:.2e}")
    for u, v in zip(res["off"][1], res["on"][1]):
        assert _rel(v, u) <= 1e-6 if kind == "max" else torch.equal(u, v)


def test_zero_edges_and_zero_nodes(route_on, native_trace):
    d = torch.device("cuda:0")
    torch.manual_seed(71)
    conv = gp.NNConv_old(24, 40, DenseNet([6, 16, 960]), aggr="mean").to(d)
    n = 17
    x = torch.randn(n, 24, device=d, requires_grad=True)
    ei, ea = torch.empty(2, 0, dtype=torch.int64, device=d), torch.empty(0, 6, device=d)
    g = torch.randn(n, 40, device=d)
    out = conv(x, ei, ea)
    (out * g).sum().backward()
    assert native_trace == ["nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw"], native_trace
    ref = x.detach().double() @ conv.root.double() + conv.bias.double()
    assert _rel(out.detach(), ref.detach()) <= TOL_FWD
    assert _rel(x.grad, g.double() @ conv.root.double().t()) <= TOL_BWD
    assert _rel(conv.root.grad, x.detach().double().t() @ g.double()) <= TOL_BWD
    assert _rel(conv.bias.grad, g.double().sum(0)) <= TOL_BWD
    for p in conv.nn.parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0
    # zero nodes: accepted by both entry points
    lib = _lib.lib()
    rowptr, ws = torch.zeros(1, dtype=torch.int32, device=d), torch.empty(1 << 20, dtype=torch.uint8, device=d)
    wl = torch.randn(960, 16, device=d)
    assert lib.gpde_nnconv_fwd_hidden_any(None, 0, None, 0, 16, rowptr.data_ptr(), None, wl.data_ptr(), None, None, None, _lib.GPDE_AGGR_MEAN,
                                          24, 40, None, ws.data_ptr(), ws.numel(), None) == _lib.GPDE_OK
    groot, gbias = torch.ones(24, 40, device=d), torch.ones(40, device=d)
    assert lib.gpde_nnconv_bwd_hidden_any(None, 0, None, 0, 16, rowptr.data_ptr(), None, wl.data_ptr(), None, None, _lib.GPDE_AGGR_MEAN, 24, 40,
                                          None, None, None, None, None, groot.data_ptr(), gbias.data_ptr(), None, None, ws.data_ptr(),
                                          ws.numel(), None) == _lib.GPDE_OK
    torch.cuda.synchronize()
    assert float(groot.abs().max()) == 0.0 and float(gbias.abs().max()) == 0.0
    # ... neither needs a workspace without nodes
    assert lib.gpde_nnconv_fwd_hidden_any(None, 0, None, 0, 16, rowptr.data_ptr(), None, None, None, None, None, _lib.GPDE_AGGR_ADD, 24, 40, None,
                                          None, 0, None) == _lib.GPDE_OK
    assert lib.gpde_nnconv_bwd_hidden_any(None, 0, None, 0, 16, rowptr.data_ptr(), None, None, None, None, _lib.GPDE_AGGR_ADD, 24, 40, None, None,
                                          None, None, None, None, None, None, None, None, 0, None) == _lib.GPDE_OK
    # outside the built range: GPDE_EUNSUPPORTED (-2)
    for aggr, cin, k in ((_lib.GPDE_AGGR_MAX, 24, 16), (_lib.GPDE_AGGR_MEAN, 257, 16), (_lib.GPDE_AGGR_MEAN, 24, 4097), (_lib.GPDE_AGGR_MEAN, 24, 0)):
        assert lib.gpde_nnconv_fwd_hidden_any(None, 0, None, 0, k, rowptr.data_ptr(), None, wl.data_ptr(), None, None, None, aggr, cin, 40, None,
                                              ws.data_ptr(), ws.numel(), None) == -2


@pytest.mark.parametrize("root_weight,bias", [(False, False), (True, False), (False, True)])
def test_without_root_or_bias(root_weight, bias, route_on):
    d = torch.device("cuda:0")
    torch.manual_seed(72)
    ei, ea, n, deg = ladder(d, seed=9)
    conv = gp.NNConv(20, 36, DenseNet([6, 16, 20 * 36]), aggr="mean", root_weight=root_weight, bias=bias).to(d)
    _step(conv, torch.randn(n, 20, device=d), ei, ea, "mean", f"20->36 root={root_weight} bias={bias}", deg=deg)


def test_cpu_module_and_cpu_tensors_are_staged(route_on, native_trace):
    d = torch.device("cuda:0")
    torch.manual_seed(73)
    ei, ea, n = synth.darcy_graph(8, 0.3)
    conv = gp.NNConv_old(24, 40, DenseNet([6, 16, 960]), aggr="mean")
    x = torch.randn(n, 24)
    xin = x.clone().requires_grad_(True)
    out = conv(xin, ei, ea)
    out.sum().backward()
    assert native_trace == ["nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw"], native_trace
    assert out.device.type == "cpu" and out.shape == (n, 40) and xin.grad is not None
    assert all(p.grad is not None and p.grad.device.type == "cpu" for p in conv.parameters())
    g_cpu = [xin.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    conv_d = copy.deepcopy(conv).to(d)
    conv_d.zero_grad()
    xd = x.to(d).requires_grad_(True)
    out_d = conv_d(xd, ei.to(d), ea.to(d))
    out_d.sum().backward()
    print(f"[reassoc] cpu vs device: {_rel(out.detach(), out_d.detach()):.2e}")
    assert _rel(out.detach(), out_d.detach()) <= 1e-6            # (the hidden layers ran on the CPU: other fp32 sums)
    for u, v in zip(g_cpu, [xd.grad] + [p.grad for p in conv_d.parameters()]):
        assert _rel(u, v) <= 1e-5


def test_residual_and_relu_are_composed_after_the_call(route_on, native_trace):
    d = torch.device("cuda:0")
    torch.manual_seed(74)
    ei, ea, n = synth.darcy_graph(10, 0.25, device=d)
    conv = gp.NNConv_old(32, 32, DenseNet([6, 16, 1024]), aggr="mean").to(d)
    x = torch.randn(n, 32, device=d)
    with torch.no_grad():
        a = conv(x, ei, ea, residual=x, activation="relu")
        b = torch.relu(x + conv(x, ei, ea))
    xa = x.clone().requires_grad_(True)
    c = conv(xa, ei, ea, residual=xa, activation="relu")
    c.sum().backward()
    assert set(native_trace) == {"nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw"}, native_trace
    print(f"[reassoc] residual + relu: {_rel(a, b):.2e} {_rel(c.detach(), b):.2e}")
    assert _rel(a, b) <= 1e-6 and _rel(c.detach(), b) <= 1e-6 and xa.grad is not None


def test_null_gradient_outputs_leave_the_others_unchanged():
    """NULL grad_x / grad_root / grad_bias (and grad_w_last / grad_b_last) through the C ABI: the other outputs keep their bits."""
    d = torch.device("cuda:0")
    csr, n, e, x, h, wl, bl, root, bias, g = _raw_case(d, seed=5)
    full = ops.nnconv_backward_hidden_any_raw(x, csr, h, wl, bl, root, "mean", g)
    names = ("grad_x", "grad_hidden", "grad_w_last", "grad_b_last", "grad_root", "grad_bias")
    for skip in ({"need_x": False}, {"need_root": False}, {"need_bias": False}, {"need_x": False, "need_root": False, "need_bias": False},
                 {"need_w_last": False, "need_b_last": False}):
        part = ops.nnconv_backward_hidden_any_raw(x, csr, h, wl, bl, root, "mean", g, **skip)
        for nm, u, v in zip(names, part, full):
            if nm.replace("grad_", "need_") in skip:
                assert u is None, (skip, nm)
            else:
                assert torch.equal(u, v), (skip, nm)
