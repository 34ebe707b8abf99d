"""GPU tier: NNConv at widths other than 64 -> 64 (1 <= in_channels, out_channels <= 256).

The reference's classes take any two widths (graph-neural-operator/nn_conv.py:234-241; `weight = nn(pseudo).view(-1, in, out)`,
nn_conv.py:274).  A module whose widths are not (64, 64) evaluates `weight = nn(pseudo)` as the caller's torch module and runs
message / aggregate / update as ONE native kernel over it (csrc/gpde_weconv_any.hip: gpde_nnconv_fwd_edgeweights_any /
gpde_nnconv_bwd_edgeweights_any).  Bars: the project's own - forward 1e-5, gradients 2e-5 relative L2 against float64
(tests/test_gpu_general_nn.py); every test prints the figures it asserts on (run with -s to see them)."""
import copy

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops, synth
from oracle.nnconv_oracle import nnconv_forward, nnconv_grads
from tests.conftest import load_golden
from tests.test_oracle_golden import load_golden_grads

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD = 1e-5, 2e-5


class DenseNet(torch.nn.Module):
    """utilities.py:201-227 restated: Linear + nonlinearity ... Linear."""

    def __init__(self, layers, nonlinearity=torch.nn.ReLU):
        super().__init__()
        self.layers = torch.nn.ModuleList()
        for j in range(len(layers) - 1):
            self.layers.append(torch.nn.Linear(layers[j], layers[j + 1]))
            if j != len(layers) - 2:
                self.layers.append(nonlinearity())

    def forward(self, x):
        for l in self.layers:
            x = l(x)
        return x


class DenseNetSin(torch.nn.Module):
    """multipole utilities.py:233-252 restated (sin applied in forward): NOT a Linear / ReLU chain."""

    def __init__(self, layers):
        super().__init__()
        self.layers = torch.nn.ModuleList(torch.nn.Linear(layers[j], layers[j + 1]) for j in range(len(layers) - 1))

    def forward(self, x):
        for j, l in enumerate(self.layers):
            x = l(x)
            if j != len(self.layers) - 1:
                x = torch.sin(x)
        return x


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _linears(nn):
    return [l for l in nn.layers if isinstance(l, torch.nn.Linear)]


def _composite64(conv, nn64, x, ei, ea, aggr, cin, cout):
    """nn_conv.py:271-282 in float64 torch ops on the device (any kernel network, 'add' / 'mean' / 'max')."""
    x = x.double()
    n = x.shape[0]
    w = nn64(ea.double()).view(-1, cin, cout)
    m = torch.matmul(x[ei[0]].unsqueeze(1), w).squeeze(1)
    if aggr == "max":
        out = torch.full((n, cout), float("-inf"), dtype=torch.float64, device=x.device)
        out = out.scatter_reduce(0, ei[1].unsqueeze(1).expand_as(m), m, "amax", include_self=True)
        out = torch.where(torch.isinf(out), torch.zeros_like(out), out)
    else:
        out = torch.zeros(n, cout, dtype=torch.float64, device=x.device).index_add_(0, ei[1], m)
        if aggr == "mean":
            out = out / torch.bincount(ei[1], minlength=n).clamp(min=1).double().unsqueeze(1)
    if conv.root is not None:
        out = out + x @ conv.root.double()
    if conv.bias is not None:
        out = out + conv.bias.double()
    return out


def _check_against_oracle(conv, x, ei, ea, aggr, tag):
    """One training step of `conv` (a Linear / ReLU chain) against oracle.nnconv_forward(float64) / oracle.nnconv_grads; exactly two
    native calls.  Returns (out, gradient dict) for the callers that compare runs."""
    lin = _linears(conv.nn)
    cout = conv.out_channels
    g = torch.randn(x.shape[0], cout, device=x.device)
    conv.zero_grad()
    xin = x.clone().requires_grad_(True)
    calls0 = _lib.n_native_calls
    out = conv(xin, ei, ea)
    (out * g).sum().backward()
    assert _lib.n_native_calls - calls0 == 2, _lib.n_native_calls - calls0       # one native forward, one native backward
    Ws, Bs = [l.weight for l in lin], [l.bias for l in lin]
    ref = nnconv_forward(x, ei, ea, Ws, Bs, conv.root, conv.bias, aggr=aggr, dtype=torch.float64)
    x2 = x.unsqueeze(-1) if x.dim() == 1 else x
    gx, gW, gb, groot, gbias = nnconv_grads(x2.cpu(), ei.cpu(), ea.cpu(), [w.detach().cpu() for w in Ws], [b.detach().cpu() for b in Bs],
                                            None if conv.root is None else conv.root.detach().cpu(),
                                            None if conv.bias is None else conv.bias.detach().cpu(), aggr, g.cpu())
    errs = {"out": _rel(out.detach(), ref), "gx": _rel(xin.grad.reshape(gx.shape), gx)}
    for l, layer in enumerate(lin):
        errs[f"gW{l}"], errs[f"gb{l}"] = _rel(layer.weight.grad, gW[l]), _rel(layer.bias.grad, gb[l])
    if conv.root is not None:
        errs["groot"] = _rel(conv.root.grad, groot)
    if conv.bias is not None:
        errs["gbias"] = _rel(conv.bias.grad, gbias)
    print(f"[widths] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert out.shape == (x.shape[0], cout)
    assert errs["out"] <= TOL_FWD, errs
    assert all(v <= TOL_BWD for k, v in errs.items() if k != "out"), errs
    grads = {"gx": xin.grad.clone(), **{f"p{i}": p.grad.clone() for i, p in enumerate(conv.parameters())}}
    return out.detach(), grads


WIDTHS = [(32, 32), (128, 128), (24, 40), (40, 24), (96, 160), (3, 5), (7, 64), (64, 32)]


@pytest.mark.parametrize("aggr", ["mean", "add"])
@pytest.mark.parametrize("cin,cout", WIDTHS)
def test_forward_and_every_gradient_vs_float64_oracle(cin, cout, aggr):
    d = torch.device("cuda:0")
    torch.manual_seed(cin * 1000 + cout)
    ei, ea, n = synth.darcy_graph(8, 0.3, device=d)
    conv = gp.NNConv_old(cin, cout, DenseNet([6, 24, 16, cin * cout]), aggr=aggr).to(d)
    _check_against_oracle(conv, torch.randn(n, cin, device=d), ei, ea, aggr, f"{cin}->{cout} {aggr}")


@pytest.mark.parametrize("root_weight,bias", [(False, False), (True, False), (False, True)])
def test_without_root_or_bias(root_weight, bias):
    d = torch.device("cuda:0")
    torch.manual_seed(5)
    ei, ea, n = synth.darcy_graph(8, 0.3, device=d)
    conv = gp.NNConv(20, 36, DenseNet([6, 16, 20 * 36]), aggr="mean", root_weight=root_weight, bias=bias).to(d)
    _check_against_oracle(conv, torch.randn(n, 20, device=d), ei, ea, "mean", f"20->36 root={root_weight} bias={bias}")


@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_one_to_one_with_1d_x(aggr):
    d = torch.device("cuda:0")
    torch.manual_seed(11)
    ei, ea, n = synth.darcy_graph(8, 0.3, device=d)
    conv = gp.NNConv_old(1, 1, DenseNet([6, 12, 1]), aggr=aggr).to(d)
    _check_against_oracle(conv, torch.randn(n, device=d), ei, ea, aggr, f"1->1 1-D x {aggr}")


def test_256_to_256_on_a_tiny_graph():
    d = torch.device("cuda:0")
    torch.manual_seed(12)
    ei, ea, n = synth.darcy_graph(4, 0.5, device=d)
    conv = gp.NNConv_old(256, 256, DenseNet([6, 8, 256 * 256]), aggr="mean").to(d)
    _check_against_oracle(conv, torch.randn(n, 256, device=d), ei, ea, "mean", "256->256")


@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_non_chain_network_vs_float64_composite(aggr):
    d = torch.device("cuda:0")
    torch.manual_seed(13)
    cin, cout = 48, 80
    ei, ea, n = synth.darcy_graph(8, 0.3, device=d)
    nn32 = DenseNetSin([6, 24, cin * cout]).to(d)
    conv = gp.NNConv_old(cin, cout, nn32, aggr=aggr).to(d)
    nn64, conv64 = copy.deepcopy(nn32).double(), copy.deepcopy(conv)
    x, g = torch.randn(n, cin, device=d), torch.randn(n, cout, device=d)
    xin = x.clone().requires_grad_(True)
    calls0 = _lib.n_native_calls
    out = conv(xin, ei, ea)
    (out * g).sum().backward()
    assert _lib.n_native_calls - calls0 == 2
    x64 = x.double().requires_grad_(True)
    ref = _composite64(conv64, nn64, x64, ei, ea, aggr, cin, cout)
    (ref * g.double()).sum().backward()
    errs = {"out": _rel(out.detach(), ref.detach()), "gx": _rel(xin.grad, x64.grad), "groot": _rel(conv.root.grad, conv64.root.grad),
            "gbias": _rel(conv.bias.grad, conv64.bias.grad)}
    for (k, p32), (_, p64) in zip(nn32.named_parameters(), nn64.named_parameters()):
        errs[k] = _rel(p32.grad, p64.grad)
    print(f"[widths] sin 48->80 {aggr}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= TOL_FWD and all(v <= TOL_BWD for k, v in errs.items() if k != "out"), errs


@pytest.mark.parametrize("name,cin,cout", [("nnconv_rect_24x40_mean", 24, 40), ("nnconv_rect_40x24_add", 40, 24), ("nnconv_rect_1x8_mean", 1, 8)])
def test_rectangular_fixtures_replayed_on_the_device(name, cin, cout):
    """The reference's own NNConv_old + DenseNet at in != out (tests/golden/make_golden_widths.py): output vs out_f64, gradients vs
    the fixture's float64 autograd through the reference's module.  The graphs carry isolated nodes, duplicate edges, self-loops
    and unsorted edges."""
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
    errs = {"out": _rel(out.detach(), g["out_f64"]), "gx": _rel(x.grad, r["gx"])}
    for l, layer in enumerate(_linears(conv.nn)):
        errs[f"gW{l}"], errs[f"gb{l}"] = _rel(layer.weight.grad, r["gW"][l]), _rel(layer.bias.grad, r["gb"][l])
    if r["groot"] is not None:
        errs["groot"] = _rel(conv.root.grad, r["groot"])
    if r["gbias"] is not None:
        errs["gbias"] = _rel(conv.bias.grad, r["gbias"])
    print(f"[widths] fixture {name}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= TOL_FWD and all(v <= TOL_BWD for k, v in errs.items() if k != "out"), errs


def _ragged(n, e, d, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - 7, (e,), generator=g)        # the last 7 nodes have no in-edge
    dst[dst == 3] = 4                                       # node 3 neither
    src[:9], dst[:9] = 2, 5                                 # 9 duplicate edges 2 -> 5
    src[9:15] = dst[9:15]                                   # self-loops
    return torch.stack([src, dst]).to(d), torch.randn(e, 6, generator=g).to(d)


@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_graph_edge_cases_at_a_rectangular_width(aggr):
    """Nodes without in-edges, duplicate edges, self-loops, edge_index in no sorted order - and the same graph with its edges
    permuted gives the same result up to summation order."""
    d = torch.device("cuda:0")
    torch.manual_seed(21)
    n, e = 90, 600
    ei, ea = _ragged(n, e, d, 31)
    conv = gp.NNConv_old(24, 40, DenseNet([6, 16, 960]), aggr=aggr).to(d)
    x = torch.randn(n, 24, device=d)
    out, _ = _check_against_oracle(conv, x, ei, ea, aggr, f"ragged 24->40 {aggr}")
    iso = torch.tensor([3] + list(range(n - 7, n)), device=d)
    assert _rel(out[iso], (x[iso] @ conv.root + conv.bias).detach()) <= 1e-6      # no in-edge: update() alone
    perm = torch.randperm(e, device=d)
    with torch.no_grad():
        out_p = conv(x, ei[:, perm].contiguous(), ea[perm].contiguous())
    print(f"[widths] permuted edges {aggr}: {_rel(out_p, out):.2e}")
    assert _rel(out_p, out) <= 1e-6


def test_zero_edges():
    d = torch.device("cuda:0")
    torch.manual_seed(22)
    conv = gp.NNConv_old(24, 40, DenseNet([6, 16, 960]), aggr="mean").to(d)
    n = 17
    x = torch.randn(n, 24, device=d, requires_grad=True)
    ei, ea = torch.empty(2, 0, dtype=torch.int64, device=d), torch.empty(0, 6, device=d)
    g = torch.randn(n, 40, device=d)
    out = conv(x, ei, ea)
    (out * g).sum().backward()
    ref = x.detach().double() @ conv.root.double() + conv.bias.double()
    assert _rel(out.detach(), ref.detach()) <= TOL_FWD
    assert _rel(x.grad, g.double() @ conv.root.double().t()) <= TOL_BWD
    assert _rel(conv.root.grad, x.detach().double().t() @ g.double()) <= TOL_BWD
    assert _rel(conv.bias.grad, g.double().sum(0)) <= TOL_BWD
    for p in conv.nn.parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0


@pytest.mark.parametrize("cin,cout", [(24, 40), (5, 3), (160, 96)])
def test_max_aggregation(cin, cout):
    """Inference: the native kernel vs the oracle.  With gradients: PyG's chain over the native message() / update() vs a float64
    composite."""
    d = torch.device("cuda:0")
    torch.manual_seed(23)
    n, e = 60, 400
    ei, ea = _ragged(n, e, d, 32)
    nn32 = DenseNet([6, 16, cin * cout]).to(d)
    conv = gp.NNConv_old(cin, cout, nn32, aggr="max").to(d)
    x = torch.randn(n, cin, device=d)
    lin = _linears(nn32)
    calls0 = _lib.n_native_calls
    with torch.no_grad():
        y = conv(x, ei, ea)
    assert _lib.n_native_calls - calls0 == 1
    ref = nnconv_forward(x, ei, ea, [l.weight for l in lin], [l.bias for l in lin], conv.root, conv.bias, aggr="max", dtype=torch.float64)
    print(f"[widths] max {cin}->{cout} inference: {_rel(y, ref):.2e}")
    assert _rel(y, ref) <= TOL_FWD
    nn64, conv64 = copy.deepcopy(nn32).double(), copy.deepcopy(conv)
    g = torch.randn(n, cout, device=d)
    xin = x.clone().requires_grad_(True)
    out = conv(xin, ei, ea)
    (out * g).sum().backward()
    x64 = x.double().requires_grad_(True)
    ref64 = _composite64(conv64, nn64, x64, ei, ea, "max", cin, cout)
    (ref64 * g.double()).sum().backward()
    errs = {"out": _rel(out.detach(), ref64.detach()), "gx": _rel(xin.grad, x64.grad), "groot": _rel(conv.root.grad, conv64.root.grad),
            "gbias": _rel(conv.bias.grad, conv64.bias.grad)}
    for (k, p32), (_, p64) in zip(nn32.named_parameters(), nn64.named_parameters()):
        errs[k] = _rel(p32.grad, p64.grad)
    print(f"[widths] max {cin}->{cout} training: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= TOL_FWD and all(v <= TOL_BWD for k, v in errs.items() if k != "out"), errs


@pytest.mark.parametrize("aggr", ["mean", "add", "max"])
def test_raw_operator_at_64_against_the_64_wide_kernels(aggr):
    """The any-width kernels called at 64 x 64 on the inputs of the specialised kernels: equal, or within 1e-6 (two summation
    orders of the same fp32 sums)."""
    d = torch.device("cuda:0")
    torch.manual_seed(24)
    ei, ea, n = synth.darcy_graph(12, 0.2, device=d)
    csr = ops.csr_for(ei, n)
    e = csr.n_edges
    x, we = torch.randn(n, 64, device=d), torch.randn(e, 4096, device=d) / 8
    root, bias, res = torch.randn(64, 64, device=d) / 8, torch.randn(64, device=d), torch.randn(n, 64, device=d)
    a = ops.nnconv_forward_edgeweights_any_raw(x, csr, we, root, bias, aggr, residual=res, relu=True)
    b = ops.nnconv_forward_edgeweights_raw(x, csr, we, root, bias, aggr, residual=res, relu=True)
    print(f"[widths] raw 64x64 forward {aggr}: {_rel(a, b):.2e} equal={torch.equal(a, b)}")
    assert torch.equal(a, b) or _rel(a, b) <= 1e-6
    a = ops.nnconv_forward_edgeweights_any_raw(x, csr, we, None, None, aggr)
    b = ops.nnconv_forward_edgeweights_raw(x, csr, we, None, None, aggr)
    assert torch.equal(a, b) or _rel(a, b) <= 1e-6
    if aggr == "max":
        with pytest.raises(NotImplementedError):
            ops.nnconv_backward_edgeweights_any_raw(x, csr, we, root, aggr, res)
        return
    g = torch.randn(n, 64, device=d)
    ga = ops.nnconv_backward_edgeweights_any_raw(x, csr, we, root, aggr, g)
    gb = ops.nnconv_backward_edgeweights_raw(x, csr, we, root, aggr, g)
    for nm, u, v in zip(("gx", "gwe", "groot", "gbias"), ga, gb):
        print(f"[widths] raw 64x64 backward {aggr} {nm}: {_rel(u, v):.2e} equal={torch.equal(u, v)}")
        assert torch.equal(u, v) or _rel(u, v) <= 1e-6, nm


@pytest.mark.parametrize("cin,cout", [(24, 40), (3, 5), (128, 128)])
def test_two_runs_give_the_same_bits(cin, cout):
    d = torch.device("cuda:0")
    torch.manual_seed(25)
    ei, ea, n = synth.darcy_graph(10, 0.25, device=d)
    conv = gp.NNConv_old(cin, cout, DenseNet([6, 16, cin * cout]), aggr="mean").to(d)
    x, g = torch.randn(n, cin, device=d), torch.randn(n, cout, device=d)
    runs = []
    for _ in range(2):
        conv.zero_grad()
        xin = x.clone().requires_grad_(True)
        out = conv(xin, ei, ea)
        (out * g).sum().backward()
        runs.append([out.detach().clone(), xin.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    for k, (u, v) in enumerate(zip(*runs)):
        assert torch.equal(u, v), k


def test_residual_and_relu_at_32_to_48():
    d = torch.device("cuda:0")
    torch.manual_seed(26)
    ei, ea, n = synth.darcy_graph(10, 0.25, device=d)
    conv = gp.NNConv_old(32, 48, DenseNet([6, 16, 32 * 48]), aggr="mean").to(d)
    x, r = torch.randn(n, 32, device=d), torch.randn(n, 48, device=d)
    with torch.no_grad():
        calls0 = _lib.n_native_calls
        fused = conv(x, ei, ea, residual=r, activation="relu")
        assert _lib.n_native_calls - calls0 == 1
        composed = torch.relu(r + conv(x, ei, ea))
        assert torch.equal(fused, composed)
        assert torch.equal(conv(x, ei, ea, activation="relu"), torch.relu(conv(x, ei, ea)))
        assert torch.equal(conv(x, ei, ea, residual=r), r + conv(x, ei, ea))
        assert torch.equal(gp.nnconv_group([(conv, x, ei, ea, r, "relu"), (conv, x, ei, ea)])[0], fused)
    # with gradients: the composed form, value and gradients
    xa, ra = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    ya = conv(xa, ei, ea, residual=ra, activation="relu")
    ya.sum().backward()
    ga = [xa.grad.clone(), ra.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    conv.zero_grad()
    xb, rb = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    yb = torch.relu(rb + conv(xb, ei, ea))
    yb.sum().backward()
    gb = [xb.grad.clone(), rb.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    assert torch.equal(ya, yb)
    for u, v in zip(ga, gb):
        assert torch.equal(u, v)


def test_cpu_tensors_in_cpu_tensor_out():
    d = torch.device("cuda:0")
    torch.manual_seed(27)
    ei, ea, n = synth.darcy_graph(8, 0.3)
    conv = gp.NNConv_old(24, 40, DenseNet([6, 16, 960]), aggr="mean")
    x = torch.randn(n, 24)
    with torch.no_grad():
        y_cpu = conv(x, ei, ea)
    assert y_cpu.device.type == "cpu" and y_cpu.shape == (n, 40)
    xin = x.clone().requires_grad_(True)
    out = conv(xin, ei, ea)
    out.sum().backward()
    assert out.device.type == "cpu" and xin.grad is not None and conv.root.grad.device.type == "cpu"
    g_cpu = [xin.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
    conv_d = copy.deepcopy(conv).to(d)
    conv_d.zero_grad()
    xd = x.to(d).requires_grad_(True)
    with torch.no_grad():
        y_dev = conv_d(x.to(d), ei.to(d), ea.to(d))
    conv_d(xd, ei.to(d), ea.to(d)).sum().backward()
    print(f"[widths] cpu vs device: {_rel(y_cpu, y_dev):.2e}")
    assert _rel(y_cpu, y_dev) <= 1e-6 and _rel(out.detach(), y_dev) <= 1e-6        # (nn(pseudo) ran on the CPU: other fp32 sums)
    for u, v in zip(g_cpu, [xd.grad] + [p.grad for p in conv_d.parameters()]):
        assert _rel(u, v) <= 1e-5


def test_message_and_update_alone():
    """nn_conv.py:273-282: message = x_j . view(nn(pseudo), in, out); update = aggr_out + x . root + bias - in float64."""
    d = torch.device("cuda:0")
    torch.manual_seed(28)
    cin, cout, e, n = 24, 40, 150, 30
    nn32 = DenseNet([6, 16, cin * cout]).to(d)
    conv = gp.NNConv_old(cin, cout, nn32, aggr="add").to(d)
    x_j, pseudo = torch.randn(e, cin, device=d), torch.randn(e, 6, device=d)
    with torch.no_grad():
        m = conv.message(x_j, pseudo)
        w64 = copy.deepcopy(nn32).double()(pseudo.double()).view(-1, cin, cout)
        ref = torch.matmul(x_j.double().unsqueeze(1), w64).squeeze(1)
        assert m.shape == (e, cout) and _rel(m, ref) <= TOL_FWD
        aggr_out, x = torch.randn(n, cout, device=d), torch.randn(n, cin, device=d)
        u = conv.update(aggr_out, x)
        assert _rel(u, aggr_out.double() + x.double() @ conv.root.double() + conv.bias.double()) <= TOL_FWD
    xg = x_j.clone().requires_grad_(True)
    conv.message(xg, pseudo).sum().backward()
    x64 = x_j.double().requires_grad_(True)
    nn64 = copy.deepcopy(nn32).double()
    nn64.zero_grad()
    torch.matmul(x64.unsqueeze(1), nn64(pseudo.double()).view(-1, cin, cout)).sum().backward()
    assert _rel(xg.grad, x64.grad) <= TOL_BWD
    for p32, p64 in zip(nn32.parameters(), nn64.parameters()):
        assert _rel(p32.grad, p64.grad) <= TOL_BWD


@pytest.mark.parametrize("chain", [True, False])
def test_nothing_is_rerouted_at_64(chain, monkeypatch):
    """With the any-width wrappers made to raise, a 64 -> 64 module runs as before: inference and a training step."""
    def boom(*a, **k):
        raise AssertionError("a 64 -> 64 call reached the any-width operator")
    monkeypatch.setattr(ops, "nnconv_forward_edgeweights_any_raw", boom)
    monkeypatch.setattr(ops, "nnconv_backward_edgeweights_any_raw", boom)
    d = torch.device("cuda:0")
    torch.manual_seed(29)
    ei, ea, n = synth.darcy_graph(10, 0.25, device=d)
    nn32 = (DenseNet([6, 32, 48, 4096]) if chain else DenseNetSin([6, 32, 4096])).to(d)
    conv = gp.NNConv_old(64, 64, nn32, aggr="mean").to(d)
    x = torch.randn(n, 64, device=d)
    with torch.no_grad():
        y = conv(x, ei, ea)
        y2 = conv(x, ei, ea, residual=x, activation="relu")
    xin = x.clone().requires_grad_(True)
    out = conv(xin, ei, ea)
    out.sum().backward()
    nn64, conv64 = copy.deepcopy(nn32).double(), copy.deepcopy(conv)
    ref = _composite64(conv64, nn64, x, ei, ea, "mean", 64, 64).detach()
    assert _rel(y, ref) <= TOL_FWD and _rel(out.detach(), ref) <= TOL_FWD and _rel(y2, torch.relu(x.double() + ref)) <= TOL_FWD
    assert xin.grad is not None and all(p.grad is not None for p in conv.parameters())
