"""GPU tier: the STREAMED any-width NNConv for kernel networks with OTHER ACTIVATIONS than the ReLU (csrc/gpde_chain_any.hip:
gpde_nnconv_fwd_chain_act / gpde_nnconv_bwd_chain_act; ops.mlp_chain; GPDE_ACT_*).

Bars: those of tests/test_gpu_chain_any.py - relative L2 against float64 autograd of the reference's op chain <= 1e-5 forward,
<= 2e-5 every gradient, worst destination row with in-degree >= 1 <= 1e-5.  Every accuracy test also runs a float32 CPU restatement
of the same chain on the same inputs and asserts it within HALF of each bar: inputs on which plain float32 cannot do that are a bug of
the test, not a question of tolerance.  Every test prints the figures it asserts on (-s shows them)."""
import copy

import pytest
import torch
from torch import nn

import graph_pde_amd as gp
from graph_pde_amd import chain_any, ops, synth
from tests.helpers.any_tilings import worst_row
from tests.helpers.streams import HOLD_MS, IssueTimer, hold, stream_beside
from tests.test_gpu_chain_any import per_edge_bytes
from tests.test_gpu_reassoc_any import TOL_BWD, TOL_FWD, TOL_ROW
from tests.test_gpu_widths import _rel

pytestmark = pytest.mark.gpu

RELU, LEAKY, ELU, TANH, SIGMOID, GELU, GELU_TANH, SILU, SIN = range(9)
NAMES = ops.ACT_NAMES
PARAM = {LEAKY: 0.2, ELU: 1.5}                                   # p0 of the kinds that have one
F = torch.nn.functional
TORCH_ACT = {RELU: lambda p: torch.relu, LEAKY: lambda p: (lambda u: F.leaky_relu(u, p)), ELU: lambda p: (lambda u: F.elu(u, p)),
             TANH: lambda p: torch.tanh, SIGMOID: lambda p: torch.sigmoid, GELU: lambda p: F.gelu,
             GELU_TANH: lambda p: (lambda u: F.gelu(u, approximate="tanh")), SILU: lambda p: F.silu, SIN: lambda p: torch.sin}
MODULE = {RELU: nn.ReLU, LEAKY: lambda: nn.LeakyReLU(0.2), ELU: lambda: nn.ELU(1.5), TANH: nn.Tanh, SIGMOID: nn.Sigmoid, GELU: nn.GELU,
          GELU_TANH: lambda: nn.GELU(approximate="tanh"), SILU: nn.SiLU, SIN: gp.Sin}


def dev():
    return torch.device("cuda:0")


def acts_of(kinds):
    return [(k, PARAM.get(k, 0.0), 0.0) for k in kinds]


# ---- inputs, the float64 reference and its float32 restatement -----------------------------------------------------------------------------
def graph(n=70, e=400, seed=0, n_src=None):
    """(edge_index [2, E] in no sorted order, in-degree per destination): one row of 130 in-edges, the last five destinations without
    any, ten copies of one edge, self-loops."""
    g = torch.Generator().manual_seed(seed)
    ns = n if n_src is None else n_src
    dst = torch.cat([torch.full((130,), 3, dtype=torch.int64), torch.randint(0, n - 5, (e - 130,), generator=g)])
    src = torch.randint(0, ns, (e,), generator=g)
    src[130:140], dst[130:140] = 7, 11                           # ten copies of one edge
    if n_src is None:
        src[140:150] = dst[140:150]                              # self-loops
    perm = torch.randperm(e, generator=g)
    deg = torch.bincount(dst, minlength=n)
    assert int((deg == 0).sum()) >= 5
    return torch.stack([src[perm], dst[perm]]), deg


def raw_case(dims, cin=24, cout=40, seed=0, scale=40.0, n=70, e=400, cind=None, n_src=None):
    """The raw operator's operands on the device: default `Linear` initialisation, edge_attr = scale * U[0, 1) in CSR slot order."""
    d = dev()
    torch.manual_seed(seed)
    ei, deg = graph(n, e, seed, n_src)
    csr = ops.csr_for(ei.to(d), n) if n_src is None else ops.csr_for(ei.to(d), n, n_src=n_src)
    lins = [nn.Linear(dims[l], dims[l + 1]) for l in range(len(dims) - 1)]
    Ws, Bs = [l.weight.detach().to(d) for l in lins], [l.bias.detach().to(d) for l in lins]
    ea_s = (scale * torch.rand(e, dims[0])).to(d)
    ns = n if n_src is None else n_src
    cind = cin if cind is None else cind
    x, xd = torch.randn(ns, cin).to(d), torch.randn(n, cind).to(d)
    root, bias, g = (torch.randn(cind, cout) / cind ** 0.5).to(d), torch.randn(cout).to(d), torch.randn(n, cout).to(d)
    return dict(csr=csr, n=n, deg=deg, dims=list(dims), x=x, xd=xd, ea_s=ea_s, Ws=Ws, Bs=Bs, root=root, bias=bias, g=g, cin=cin, cind=cind, cout=cout)


def reference(c, acts, aggr, dtype, x_dst="one"):
    """Autograd on the CPU in `dtype` through the reference's op chain from edge_attr (CSR slot order): nn(pseudo) -> view ->
    matmul -> aggregate -> root, bias (nn_conv.py:274-282).  x_dst: "one" (one node set), "dst" (c['xd']) or None (no root term).
    (out, {name: gradient}), `max|U_1|` of the first pre-activation."""
    f = lambda t: t.detach().to(dtype).cpu().requires_grad_(True)
    csr = c["csr"]
    xs, ea, g = f(c["x"]), f(c["ea_s"]), c["g"].detach().to(dtype).cpu()
    xd = None if x_dst != "dst" else f(c["xd"])
    root = None if x_dst is None else f(c["root"])
    b = f(c["bias"])
    W, B = [f(w) for w in c["Ws"]], [f(v) for v in c["Bs"]]
    src, rowptr = csr.src.long().cpu(), csr.rowptr.long().cpu()
    cnt = rowptr[1:] - rowptr[:-1]
    dst = torch.repeat_interleave(torch.arange(csr.n_nodes), cnt)
    h, umax = ea, 0.0
    for l, (w, v, a) in enumerate(zip(W[:-1], B[:-1], acts)):
        u = h @ w.t() + v
        umax = float(u.detach().abs().max()) if l == 0 else umax
        h = TORCH_ACT[a[0]](a[1])(u)
    cin = xs.shape[1]
    w = (h @ W[-1].t() + B[-1]).view(-1, cin, W[-1].shape[0] // cin)
    out = torch.zeros(csr.n_nodes, w.shape[2], dtype=dtype).index_add(0, dst, torch.matmul(xs[src].unsqueeze(1), w).squeeze(1))
    if aggr == "mean":
        out = out / cnt.clamp(min=1).to(dtype).unsqueeze(1)
    if root is not None:
        out = out + (xs if x_dst == "one" else xd) @ root
    out = out + b
    (out * g).sum().backward()
    z = lambda t: None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad)
    grads = {"gxs": z(xs), "gxd": z(xd), "gea": z(ea), "groot": z(root), "gbias": z(b)}
    for l, (w_, v_) in enumerate(zip(W, B)):
        grads[f"gW{l}"], grads[f"gb{l}"] = z(w_), z(v_)
    return out.detach(), grads, umax


def errors(out, grads, ref_out, ref, deg):
    """Every asserted figure of `out` / `grads` (dict as `reference` returns; None entries skipped) against the float64 reference."""
    errs = {"out": _rel(out, ref_out), "row": worst_row(out.detach().cpu()[deg >= 1], ref_out[deg >= 1])}
    for nm, v in grads.items():
        if v is not None and ref.get(nm) is not None:
            errs[nm] = _rel(v, ref[nm])
    return errs


def within(errs, share=1.0):
    return errs["out"] <= share * TOL_FWD and errs["row"] <= share * TOL_ROW and \
        all(v <= share * TOL_BWD for k, v in errs.items() if k not in ("out", "row"))


def run_raw(c, acts, aggr, x_dst="one", blocks=None, n_bad=None):
    """The two raw wrappers on the case `c`: (out, gradient dict with the names of `reference`)."""
    xd = ops._ONE_SET if x_dst == "one" else c["xd"] if x_dst == "dst" else None
    root = None if x_dst is None else c["root"]
    out = ops.nnconv_forward_chain_any_raw(c["x"], xd, c["csr"], c["ea_s"], c["Ws"], c["Bs"], root, c["bias"], aggr, blocks=blocks, acts=acts)
    gxs, gxd, gea, gw, gb, groot, gbias = ops.nnconv_backward_chain_any_raw(c["x"], xd, c["csr"], c["ea_s"], c["Ws"], c["Bs"], root, aggr, c["g"],
                                                                            need_edge_attr=True, blocks=blocks, acts=acts)
    grads = {"gxs": gxs, "gxd": gxd, "gea": gea, "groot": groot, "gbias": gbias}
    for l, (w, b) in enumerate(zip(gw, gb)):
        grads[f"gW{l}"], grads[f"gb{l}"] = w, b
    return out, grads


def check_vs_float64(tag, c, acts, aggr, x_dst="one", got=None):
    """The GPU result within the bars, the float32 CPU restatement within half of them; both printed.  Returns (out, grads, max|U_1|)."""
    ref_out, ref, umax = reference(c, acts, aggr, torch.float64, x_dst)
    out32, g32, _ = reference(c, acts, aggr, torch.float32, x_dst)
    e32 = errors(out32, g32, ref_out, ref, c["deg"])
    out, grads = run_raw(c, acts, aggr, x_dst) if got is None else got
    torch.cuda.synchronize()
    errs = errors(out, grads, ref_out, ref, c["deg"])
    show = lambda e: " ".join(f"{a}={b:.1e}" for a, b in e.items())
    print(f"[chain_act] {tag}: max|U_1|={umax:.1f}\n    gpu   {show(errs)}\n    cpu32 {show(e32)}")
    assert within(e32, 0.5), ("the float32 restatement misses half the bars: a bug of the test's inputs", tag, e32)
    finite = all(bool(torch.isfinite(t).all()) for t in [out] + [v for v in grads.values() if v is not None])
    assert finite, tag
    assert set(errs) == set(e32) and within(errs), (tag, errs)
    return out, grads, umax


@pytest.fixture
def entry_points(monkeypatch):
    """Names of the streamed route's native entry points the test's calls went through, in order."""
    trace = []

    def spy(name, *a, _f=chain_any._chain_any_call, **k):
        trace.append(name)
        return _f(name, *a, **k)
    monkeypatch.setattr(chain_any, "_chain_any_call", spy)
    return trace


ACT_PAIR = ["gpde_nnconv_fwd_chain_act", "gpde_nnconv_bwd_chain_act"]
ANY_PAIR = ["gpde_nnconv_fwd_chain_any", "gpde_nnconv_bwd_chain_any"]


# ---- 1. every kind against float64 ---------------------------------------------------------------------------------------------------------
def chain_dims(k0, k, n_linear, cin, cout):
    """2 Linears: k is the width k_ch_first writes (65, 130: across its 64-column tile).  3: k comes out of the layer GEMM (130: across
    its 128-column tile) behind a padded-free 12.  5: k first AND last - k_ch_first's padded rows feed a GEMM, the GEMM's last layer
    has rows of K floats."""
    return {2: [k0, k, cin * cout], 3: [k0, 12, k, cin * cout], 5: [k0, k, 7, 20, k, cin * cout]}[n_linear]


HIDDEN = (7, 33, 65, 130)
# kinds 1 .. 8 x four hidden widths x chains of 2, 3, 5 Linears = 96 cases; k0 in {1, 6}, add / mean and the widths 3 -> 5 / 24 -> 40 go
# round over the four hidden widths at three different rotations (ki, ki // 2, ki + ki // 2), so that every kind meets every PAIR of
# them with every chain length
CASES = [(kind, k, nl, (1, 6)[(kind + ki + ni) % 2], ("mean", "add")[(kind + ki + ki // 2 + ni) % 2], ((3, 5), (24, 40))[(kind + ki // 2 + ni) % 2])
         for kind in range(1, 9) for ki, k in enumerate(HIDDEN) for ni, nl in enumerate((2, 3, 5))]
for _kind in range(1, 9):
    for _nl in (2, 3, 5):
        _c = [c for c in CASES if c[0] == _kind and c[2] == _nl]
        assert all(len({(c[i], c[j]) for c in _c}) == 4 for i, j in ((3, 4), (3, 5), (4, 5))), (_kind, _nl)


@pytest.mark.parametrize("kind,k,n_linear,k0,aggr,widths", CASES, ids=[f"{NAMES[c[0]]}-K{c[1]}-{c[2]}lin-k0_{c[3]}-{c[4]}-{c[5][0]}to{c[5][1]}" for c in CASES])
def test_every_kind_vs_float64(kind, k, n_linear, k0, aggr, widths, entry_points):
    cin, cout = widths
    dims = chain_dims(k0, k, n_linear, cin, cout)
    c = raw_case(dims, cin, cout, seed=kind * 100 + k + n_linear)
    check_vs_float64(f"{NAMES[kind]} {cin}->{cout} dims={dims} {aggr}", c, acts_of([kind] * (n_linear - 1)), aggr)
    assert entry_points == ACT_PAIR, entry_points


# ---- 2. RELU through the new entry points ----------------------------------------------------------------------------------------------------
def test_relu_through_the_new_entry_points_equals_the_existing_ones(monkeypatch, entry_points):
    c = raw_case([6, 33, 65, 960], seed=21)
    relu = acts_of([RELU, RELU])
    old_out, old = run_raw(c, None, "mean")
    also_out, also = run_raw(c, relu, "mean")                    # an all-RELU `acts` keeps the `_chain_any` entry points
    assert entry_points == ANY_PAIR * 2, entry_points
    monkeypatch.setattr(ops, "acts_all_relu", lambda acts: acts is None)      # ... unless the host is told not to
    new_out, new = run_raw(c, relu, "mean")
    assert entry_points[4:] == ACT_PAIR, entry_points
    for nm, got in (("all-RELU acts", (also_out, also)), ("chain_act entry points", (new_out, new))):
        assert torch.equal(got[0], old_out), nm
        for k, v in old.items():
            assert (v is None and got[1][k] is None) or torch.equal(got[1][k], v), (nm, k)
    monkeypatch.undo()
    check_vs_float64("RELU by the chain_act entry points", c, relu, "mean", got=(new_out, new))


# ---- 3. the padding trap -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [SIGMOID, GELU], ids=["sigmoid", "gelu"])
@pytest.mark.parametrize("k", [5, 6])
def test_padding_columns_hold_zero_whatever_act_of_zero_is(kind, k):
    """Hidden width k = 5 / 6 (KP - K = 3 / 2) in front of a layer GEMM: sigmoid(0) = 0.5 in a padding column must not reach the next
    layer.  Against float64, and `out` bit for bit against the same chain zero-extended to width 8 BY THE CALLER: W_1 / b_1 get zero
    rows, W_2 zero columns - the added units hold act(0) and are multiplied by zeros, as padding must be."""
    c = raw_case([6, k, 12, 960], seed=31 + k)
    acts = acts_of([kind, kind])
    out, _, _ = check_vs_float64(f"padding {NAMES[kind]} K={k}", c, acts, "add")
    wide = dict(c)
    W1, b1, W2 = torch.zeros(8, 6, device=dev()), torch.zeros(8, device=dev()), torch.zeros(12, 8, device=dev())
    W1[:k], b1[:k], W2[:, :k] = c["Ws"][0], c["Bs"][0], c["Ws"][1]
    wide["Ws"], wide["Bs"], wide["dims"] = [W1, W2, c["Ws"][2]], [b1, c["Bs"][1], c["Bs"][2]], [6, 8, 12, 960]
    out8, g8 = run_raw(wide, acts, "add")
    assert torch.equal(out8, out), float((out8 - out).abs().max())
    _, g5 = run_raw(c, acts, "add")
    assert torch.equal(g8["gxs"], g5["gxs"]) and torch.equal(g8["gea"], g5["gea"])
    assert torch.equal(g8["gW0"][:k], g5["gW0"]) and torch.equal(g8["gW1"][:, :k], g5["gW1"])


@pytest.mark.parametrize("kind", [SIGMOID, GELU], ids=["sigmoid", "gelu"])
@pytest.mark.parametrize("k", [5, 6])
def test_padding_columns_of_a_gemm_written_layer(kind, k):
    """The same with the padded width in the SECOND hidden layer of four Linears: its rows come out of the layer GEMM's epilogue
    (columns from act_n on store 0; GELU: U_l beside it) and feed the next GEMM."""
    c = raw_case([6, 12, k, 12, 960], seed=35 + k)
    acts = acts_of([kind] * 3)
    out, g5, _ = check_vs_float64(f"padding behind the GEMM {NAMES[kind]} K={k}", c, acts, "add")
    wide = dict(c)
    W2, b2, W3 = torch.zeros(8, 12, device=dev()), torch.zeros(8, device=dev()), torch.zeros(12, 8, device=dev())
    W2[:k], b2[:k], W3[:, :k] = c["Ws"][1], c["Bs"][1], c["Ws"][2]
    wide["Ws"], wide["Bs"] = [c["Ws"][0], W2, W3, c["Ws"][3]], [c["Bs"][0], b2, c["Bs"][2], c["Bs"][3]]
    wide["dims"] = [6, 12, 8, 12, 960]
    out8, g8 = run_raw(wide, acts, "add")
    assert torch.equal(out8, out), float((out8 - out).abs().max())
    assert torch.equal(g8["gxs"], g5["gxs"]) and torch.equal(g8["gea"], g5["gea"]) and torch.equal(g8["gW0"], g5["gW0"])
    assert torch.equal(g8["gW1"][:k], g5["gW1"]) and torch.equal(g8["gW2"][:, :k], g5["gW2"])


# ---- 4. a mixed chain --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_mixed_chain_vs_float64(aggr, entry_points):
    c = raw_case([6, 33, 65, 20, 960], seed=41)
    check_vs_float64(f"mixed tanh / gelu / leaky_relu(0.2) {aggr}", c, acts_of([TANH, GELU, LEAKY]), aggr)
    assert entry_points == ACT_PAIR


# ---- 5. block tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [TANH, SILU], ids=["tanh_from_h", "silu_from_u"])
def test_block_tables_give_the_same_bits(kind):
    c = raw_case([6, 33, 65, 960], seed=51)
    acts, csr, n = acts_of([kind, kind]), c["csr"], c["n"]
    rp = csr.rowptr_host.tolist()
    one_block = ops.chain_any_blocks(csr, c["dims"], 24, 24, 40, budget_bytes=1 << 30, acts=acts)
    per_node = ops.chain_any_table([[i, rp[i]] for i in range(n + 1)], n, csr.n_edges, c["dims"], 24, 24, 40, acts=acts)
    assert one_block.n_blocks == 1 and per_node.n_blocks == n
    ref_out, ref, _ = reference(c, acts, "mean", torch.float64)
    runs = {}
    for label, blocks in (("one block", one_block), ("node per block", per_node)):
        out, grads = run_raw(c, acts, "mean", blocks=blocks)
        errs = errors(out, grads, ref_out, ref, c["deg"])
        print(f"[chain_act] block table {NAMES[kind]} {label} (ws {blocks.ws_fwd} / {blocks.ws_bwd}): " + " ".join(f"{a}={b:.1e}" for a, b in errs.items()))
        assert within(errs), (label, errs)
        runs[label] = (out, grads)
    for nm in ("gxs", "gea"):
        assert torch.equal(runs["one block"][1][nm], runs["node per block"][1][nm]), nm
    assert torch.equal(runs["one block"][0], runs["node per block"][0])


# ---- 6. saturation -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [ELU, SILU, SIGMOID, TANH, GELU, GELU_TANH], ids=lambda k: NAMES[k])
def test_saturated_units_stay_finite_and_within_the_bars(kind):
    """edge_attr scaled until max|U_1| >= 90, past expf's float32 range: every output and gradient finite and within the bars (a
    0 * inf of a both-branches form would be NaN here).  SIN is left out: float32 loses digits to argument reduction at that size."""
    c = raw_case([6, 33, 65, 960], seed=61, scale=200.0)
    _, _, umax = check_vs_float64(f"saturation {NAMES[kind]}", c, acts_of([kind, kind]), "mean")
    assert umax >= 90.0, umax


# ---- 7. two node sets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_dst", ["dst", None], ids=["x_dst", "no_x_dst"])
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_two_node_sets_vs_float64(aggr, x_dst, entry_points):
    c = raw_case([6, 16, 33, 960], seed=71, n=40, e=400, n_src=150, cind=7)
    check_vs_float64(f"two node sets 150->40 x_dst={x_dst} gelu {aggr}", c, acts_of([GELU, GELU]), aggr, x_dst=x_dst)
    assert entry_points == ACT_PAIR


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
def composite64(conv, x, ei, ea, g):
    """float64 autograd on the CPU through nn_conv.py:271-282 with the module's own `nn`: (out, {gx, gea, groot, gbias, p<i>: nn's})."""
    m = copy.deepcopy(conv).double().cpu()
    x6, e6 = x.detach().double().cpu().requires_grad_(True), ea.detach().double().cpu().requires_grad_(True)
    ei = ei.cpu()
    n, cin, cout = x.shape[0], m.in_channels, m.out_channels
    w = m.nn(e6).view(-1, cin, cout)
    out = torch.zeros(n, cout, dtype=torch.float64).index_add(0, ei[1], torch.matmul(x6[ei[0]].unsqueeze(1), w).squeeze(1))
    if m.aggr == "mean":
        out = out / torch.bincount(ei[1], minlength=n).clamp(min=1).double().unsqueeze(1)
    out = out + x6 @ m.root + m.bias
    (out * g.double().cpu()).sum().backward()
    grads = {"gx": x6.grad, "gea": e6.grad, "groot": m.root.grad, "gbias": m.bias.grad}
    grads.update({f"p{i}": p.grad for i, p in enumerate(m.nn.parameters())})
    return out.detach(), grads


def module_step(conv, x, ei, ea, g):
    conv.zero_grad(set_to_none=True)
    xin, ein = x.clone().requires_grad_(True), ea.clone().requires_grad_(True)
    out = conv(xin, ei, ein)
    (out * g).sum().backward()
    grads = {"gx": xin.grad, "gea": ein.grad, "groot": conv.root.grad, "gbias": conv.bias.grad}
    grads.update({f"p{i}": p.grad for i, p in enumerate(conv.nn.parameters())})
    return out.detach(), grads


def module_errs(tag, got, want, deg):
    errs = {"out": _rel(got[0], want[0]), "row": worst_row(got[0].cpu()[deg >= 1], want[0][deg >= 1])}
    errs.update({k: _rel(v, want[1][k]) for k, v in got[1].items()})
    print(f"[chain_act] {tag}: " + " ".join(f"{a}={b:.1e}" for a, b in errs.items()))
    assert within(errs), (tag, errs)


@pytest.fixture
def weight_routes(monkeypatch):
    """Names of the per-edge-weight and hidden-form wrappers the test's calls went through."""
    trace = []
    for name in ("nnconv_forward_edgeweights_any_raw", "nnconv_backward_edgeweights_any_raw", "nnconv_forward_edgeweights_raw",
                 "nnconv_backward_edgeweights_raw", "nnconv_forward_hidden_any_raw", "nnconv_backward_hidden_any_raw"):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            trace.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return trace


# ---- 8. the module, streamed ---------------------------------------------------------------------------------------------------------------
def gelu_net():
    return nn.Sequential(nn.Linear(6, 16), nn.GELU(), nn.Linear(16, 32), nn.GELU(), nn.Linear(32, 960))


def test_module_streamed_runs_a_gelu_network_without_per_edge_weights(monkeypatch, entry_points, weight_routes):
    """FAILS ON THE PARENT, where a GELU network is "not eligible" and its [E, 960] per-edge weights are materialised."""
    d = dev()
    monkeypatch.setattr(ops, "ANY_REASSOC", "streamed")
    torch.manual_seed(81)
    ei, deg = graph(seed=81)
    ei, ea = ei.to(d), torch.rand(400, 6, device=d)
    conv = gp.NNConv_old(24, 40, gelu_net(), aggr="mean").to(d)
    x, g = torch.randn(70, 24, device=d), torch.randn(70, 40, device=d)
    got = module_step(conv, x, ei, ea, g)
    assert entry_points == ACT_PAIR and weight_routes == [], (entry_points, weight_routes)
    module_errs("module streamed gelu", got, composite64(conv, x, ei, ea, g), deg)
    # the capability: a training step on ~40 k edges.  K_max is read as the chain's widest layer, 960 - the per-edge weights [E, 960] the
    # other routes form, twice with their gradient; the last hidden width 32 cannot be meant: the route's per-edge dx rows [E, 24] alone
    # are 3/4 of E * 32 * 4.  The bar is an EIGHTH of that tensor, the share tests/test_gpu_chain_any.py grants the backward's workspace
    # of its capability test, for the workspace as for the step's whole peak
    ei, ea, n = synth.darcy_graph(31, 0.125, device=d)
    e = ei.shape[1]
    assert 35_000 <= e <= 45_000, e
    monkeypatch.setattr(ops, "CHAIN_ANY_PREF_BUDGET", 3 << 20)
    csr = ops.csr_for(ei, n)
    _ = csr.src_order                                            # (the graph's own tables are not the step's memory)
    x, g = torch.randn(n, 24, device=d), torch.randn(n, 40, device=d)
    blocks = ops.chain_any_blocks(csr, [6, 16, 32, 960], 24, 24, 40, acts=acts_of([GELU, GELU]))
    del entry_points[:]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = module_step(conv, x, ei, ea, g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[chain_act] capability: N={n} E={e} blocks={blocks.n_blocks} ws_bwd={blocks.ws_bwd} B, peak rise {peak} B; E * 960 * 4 / 8 = "
          f"{e * 960 * 4 // 8} B; E * 32 * 4 = {e * 32 * 4} B")
    assert entry_points == ACT_PAIR and weight_routes == []
    assert blocks.budget_bytes == 3 << 20 and blocks.ws_bwd <= e * 960 * 4 // 8, blocks
    assert peak < e * 960 * 4 // 8, peak
    module_errs("module streamed gelu, 40 k edges", got, composite64(conv, x, ei, ea, g), torch.bincount(ei[1].cpu(), minlength=n))


# ---- 9. 64 -> 64 that does not fit -------------------------------------------------------------------------------------------------------------
def test_a_64_wide_tanh_network_that_does_not_fit_runs_streamed(monkeypatch, entry_points, weight_routes):
    """RAISES RuntimeError ON THE PARENT (2 x E x 16 KiB of per-edge weights do not fit).  With the true free bytes the module keeps the
    route it has there: the per-edge-weight kernel."""
    d = dev()
    torch.manual_seed(91)
    ei, deg = graph(seed=91)
    ei, ea = ei.to(d), torch.rand(400, 6, device=d)
    conv = gp.NNConv_old(64, 64, nn.Sequential(nn.Linear(6, 32), nn.Tanh(), nn.Linear(32, 4096)), aggr="mean").to(d)
    x, g = torch.randn(70, 64, device=d), torch.randn(70, 64, device=d)
    want = composite64(conv, x, ei, ea, g)
    fits = module_step(conv, x, ei, ea, g)
    assert entry_points == [] and weight_routes == ["nnconv_forward_edgeweights_raw", "nnconv_backward_edgeweights_raw"], (entry_points, weight_routes)
    module_errs("64->64 tanh, fits: per-edge weights", fits, want, deg)
    need = 2 * 400 * 64 * 64 * 4
    own = 2 * ops.any_width_route(70, 400, 64, 64, 32, "mean", True, 0, mode="streamed", dims=[6, 32, 4096], acts=acts_of([TANH]))["bytes_streamed"]
    short = need // 2
    assert own < short < need, (own, short, need)
    true_free = ops.device_free_bytes
    monkeypatch.setattr(ops, "device_free_bytes", lambda dv: (short, true_free(dv)[1]))
    del weight_routes[:]
    got = module_step(conv, x, ei, ea, g)
    assert entry_points == ACT_PAIR and weight_routes == [], (entry_points, weight_routes)
    module_errs("64->64 tanh, does not fit: streamed", got, want, deg)
    monkeypatch.setattr(ops, "ANY_REASSOC", "off")               # ... and `off` is the behaviour before: refused
    with pytest.raises(RuntimeError, match="is not a Linear / ReLU chain"):
        conv(x, ei, ea)


# ---- 10. `on` and `auto` keep their routes -----------------------------------------------------------------------------------------------------
def test_on_and_auto_keep_their_routes_for_a_tanh_network_that_fits(monkeypatch, entry_points, weight_routes):
    d = dev()
    torch.manual_seed(101)
    ei, deg = graph(seed=101)
    ei, ea = ei.to(d), torch.rand(400, 6, device=d)
    conv = gp.NNConv_old(24, 40, nn.Sequential(nn.Linear(6, 12), nn.Tanh(), nn.Linear(12, 33), nn.Tanh(), nn.Linear(33, 960)), aggr="mean").to(d)
    x, g = torch.randn(70, 24, device=d), torch.randn(70, 40, device=d)
    want = composite64(conv, x, ei, ea, g)
    outs = {}
    for mode in ("on", "auto", "off"):
        monkeypatch.setattr(ops, "ANY_REASSOC", mode)
        del weight_routes[:]
        outs[mode] = module_step(conv, x, ei, ea, g)
        assert entry_points == [] and weight_routes == ["nnconv_forward_edgeweights_any_raw", "nnconv_backward_edgeweights_any_raw"], (mode, weight_routes)
        module_errs(f"tanh network that fits, mode {mode}: materialised", outs[mode], want, deg)
    assert torch.equal(outs["on"][0], outs["off"][0]) and torch.equal(outs["auto"][0], outs["off"][0])


# ---- 11. streams -----------------------------------------------------------------------------------------------------------------------------
def test_off_the_default_stream_and_back_to_back():
    """The two wrappers on a side stream S while the default stream and S are held (S twice as long), the inputs copied into
    zero-filled buffers behind S's hold: a launch that slipped onto another stream would read zeros.  Then two calls back to back.
    All outputs bitwise equal to the default-stream baseline.  SILU: the layer GEMM writes U_l next to H_l."""
    c = raw_case([6, 33, 65, 960], seed=111)
    acts, csr = acts_of([SILU, SILU]), c["csr"]
    blocks = ops.chain_any_blocks(csr, c["dims"], 24, 24, 40, budget_bytes=60 * ops.chain_edge_bytes(c["dims"], acts), acts=acts)
    assert blocks.n_blocks > 3 and ops.chain_edge_bytes(c["dims"], acts) > per_edge_bytes(c["dims"])
    _ = csr.src_order

    def call(x, ea_s, g, w0):
        cc = dict(c, x=x, ea_s=ea_s, g=g, Ws=[w0] + c["Ws"][1:])
        out, grads = run_raw(cc, acts, "mean", blocks=blocks)
        return [out] + [v for v in grads.values() if v is not None]
    ins = dict(x=c["x"], ea_s=c["ea_s"], g=c["g"], w0=c["Ws"][0])
    base = call(**ins)
    torch.cuda.synchronize()
    default = torch.cuda.current_stream()
    S = stream_beside(default)
    with torch.cuda.stream(S):                                   # once without a hold: S's allocator pool then holds every block
        first = call(**ins)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(first, base))
    del first
    staged = {k: torch.zeros_like(v) for k, v in ins.items()}
    held0, held_s = hold(default, HOLD_MS), hold(S, 2 * HOLD_MS)
    with IssueTimer() as t, torch.cuda.stream(S):
        for k, v in ins.items():
            staged[k].copy_(v)
        got = call(**staged)
        again = call(**staged)
    open0, open_s = not held0.query(), not held_s.query()
    torch.cuda.synchronize()
    print(f"[chain_act] side stream: three calls issued in {t.ms:.2f} ms of host time; windows open: default {open0}, side {open_s}")
    assert open0 and open_s, "a hold ended before the calls were issued: a call synchronised the host"
    for nm, r in (("side stream", got), ("back to back", again)):
        assert all(torch.equal(u, v) for u, v in zip(r, base)), nm
