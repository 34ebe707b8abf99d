"""GPU tier: the any-width NNConv kernels (csrc/gpde_weconv_any.hip) in EVERY lane tiling, on long rows, past 2^32 elements of W_e,
with misaligned buffers and through the branches only the C ABI reaches.

The host picks the tiling (V, LC, R, ES, B) from the widths; tests/helpers/any_tilings.py classifies all 65,536 width pairs by
what the kernels do differently (128 classes for add / mean; tests/test_widths_host.py pins the count) and this file runs the
smallest widths of each class, chosen from the library's plan query at collection time.  Every case asserts through
ops.any_width_plan that it ran the class it names.  No case is skipped or expected to fail.

Reference: float64 torch ops on the device for the same fp32 W_e (tests/helpers/any_tilings.reference64), gradients by float64
autograd of it.  Bars: forward 1e-5, every gradient 2e-5 relative L2 - and the same bars ROW BY ROW (per destination for out, per
edge for dW_e, per source for dx): |err_row| <= bar x max(|ref_row|, rms row norm of the reference), since a global norm hides
one wrong ladder node or tail edge.  Correct fp32 arithmetic is far inside the row bars on these short rows: the reference's own
fp32 chain on the ladder graphs, on the CPU (tests/test_widths_host.py), is at most
    1 -> 1      out 6.8e-07  dW_e 7.8e-08  dx 8.9e-07
    64 -> 255   out 1.4e-07  dW_e 3.7e-08  dx 3.0e-07
    256 -> 132  out 2.3e-07  dW_e 3.7e-08  dx 2.3e-07
Long rows (8,192 in-edges into one node, 8,192 out-edges of one node) are held to the rule of tests/test_gpu_regime_properties.py:
the hub row within max(1e-6, 4 x e32) of float64, and within 1e-5 outright when e32 <= 2.5e-6, e32 being the distance of the
reference's fp32 chain (oracle.nnconv_forward, float32) from float64 on that row.  Every test prints the figures it asserts on."""
import os

import pytest
import torch
from hypothesis import HealthCheck, assume, given, settings
from hypothesis import strategies as st

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from oracle.nnconv_oracle import nnconv_forward
from tests.helpers import any_tilings as at
from tests.helpers.kinks import edges_off_the_kink
from tests.test_gpu_widths import DenseNet, _check_against_oracle

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD = 1e-5, 2e-5
HUB_TOL_FWD, FWD_FACTOR, E32_WELL = 1e-6, 4, 2.5e-6      # tests/test_gpu_regime_properties.py
N_EXAMPLES = int(os.environ.get("GPDE_HYP_EXAMPLES", "8"))      # small graphs: 8 examples per test by default (the first drawn is the empty graph)
HUB = 8192

REPS = at.representatives()                     # [(name, class, cin, cout)] x 128, from the plan query
MAX_REPS = at.max_representatives()
# the residual + ReLU epilogue: the V = 1 class with the most column steps and the V = 4, LC = 64 classes among them
EPILOGUE_REPS = [r for r in REPS if (r[1][0] == 1 and r[1][5] == 4) or (r[1][0] == 4 and r[1][1] == 64)]


def _dev():
    return torch.device("cuda:0")


def _aligned(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def _bars(figs, tag):
    print(f"[tilings] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    bad = {k: v for k, v in figs.items() if not v <= (TOL_FWD if k.startswith("out") else TOL_BWD)}
    assert not bad, (tag, bad)


def _case(cin, cout, aggr, seed, plan=None):
    """Ladder graph of the widths' tiling, inputs on the device, the CSR, W_e in slot order."""
    d = _dev()
    gen = torch.Generator().manual_seed(seed)
    plan = plan or ops.any_width_plan(cin, cout, aggr=aggr)
    ei, n, by_deg = at.ladder_graph(plan, gen)
    x, w, root, bias, res, g = at.draw_inputs(n, ei.shape[1], cin, cout, gen, d)
    ei = ei.to(d)
    csr = ops.csr_for(ei, n)
    we = w[csr.perm.long()].contiguous()
    return dict(ei=ei, n=n, by_deg=by_deg, x=x, w=w, root=root, bias=bias, res=res, g=g, csr=csr, we=we, perm=csr.perm.long())


def _forward_figs(c, aggr, residual=False, relu=False):
    res = c["res"] if residual else None
    y = ops.nnconv_forward_edgeweights_any_raw(c["x"], c["csr"], c["we"], c["root"], c["bias"], aggr, residual=res, relu=relu)
    ref = at.reference64(c["x"].double(), c["ei"], c["w"].double(), c["root"].double(), c["bias"].double(), aggr,
                         residual=None if res is None else res.double(), relu=relu)
    assert y.shape == ref.shape and bool(torch.isfinite(y).all())
    return y, {"out": at.rel(y, ref), "out_row": at.worst_row(y, ref)}


def _backward_figs(c, aggr):
    gx, gwe, groot, gbias = ops.nnconv_backward_edgeweights_any_raw(c["x"], c["csr"], c["we"], c["root"], aggr, c["g"])
    lv = [t.double().requires_grad_(True) for t in (c["x"], c["w"], c["root"], c["bias"])]
    (at.reference64(lv[0], c["ei"], lv[1], lv[2], lv[3], aggr) * c["g"].double()).sum().backward()
    rwe = lv[1].grad[c["perm"]]
    for t in (gx, gwe, groot, gbias):
        assert bool(torch.isfinite(t).all())
    return {"dW_e": at.rel(gwe, rwe), "dW_e_row": at.worst_row(gwe, rwe), "dx": at.rel(gx, lv[0].grad),
            "dx_row": at.worst_row(gx, lv[0].grad), "droot": at.rel(groot, lv[2].grad), "dbias": at.rel(gbias, lv[3].grad)}


# ---- 3. every tiling class ----------------------------------------------------------------------------------------------------
def test_all_128_classes_are_parametrised():
    assert len(REPS) == at.N_CLASSES == 128 and len({r[0] for r in REPS}) == 128
    assert len(MAX_REPS) >= 8 and EPILOGUE_REPS and {r[1][0] for r in EPILOGUE_REPS} == {1, 4}


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("name,cls,cin,cout", REPS, ids=[r[0] for r in REPS])
def test_tiling_class_forward_and_gradients_vs_float64(name, cls, cin, cout, aggr):
    c = _case(cin, cout, aggr, 7 * cin + 1000 * cout)
    assert _aligned(c["we"], c["root"], c["bias"], c["g"])
    plan = ops.any_width_plan(cin, cout, aligned=True, aggr=aggr)
    assert at.tiling_class(cin, cout, plan) == cls and at.class_name(cls) == name, (name, plan)
    eb = plan["B"] * plan["ES"]
    assert {1, eb, eb + 1, 4 * eb + plan["ES"] + 1} <= set(c["by_deg"]) and c["csr"].max_in_degree == 4 * eb + plan["ES"] + 1
    _, figs = _forward_figs(c, aggr)
    figs.update(_backward_figs(c, aggr))
    _bars(figs, f"{name} {cin}->{cout} {aggr} E={c['csr'].n_edges}")


@pytest.mark.parametrize("cin", [1, 6])
@pytest.mark.parametrize("name,key,_cin,cout", MAX_REPS, ids=[r[0] for r in MAX_REPS])
def test_max_tiling_forward_vs_float64(name, key, _cin, cout, cin):
    """Each tiling of the 'max' plan (it depends on out_channels alone) at in_channels 1 and 6: the row loop's remainder arm
    alone, and its 4-row arm plus a remainder.  Continuous random W_e: no two messages of a node tie (duplicate edges carry
    their own W_e rows)."""
    plan = ops.any_width_plan(cin, cout, aggr="max")
    assert (plan["V"], plan["LC"], plan["ES"]) == key and plan["R"] == 1
    c = _case(cin, cout, "max", 13 * cin + 1000 * cout, plan)
    assert _aligned(c["we"], c["root"], c["bias"])
    y, figs = _forward_figs(c, "max")
    iso = c["by_deg"][0]
    assert at.rel(y[iso], c["x"][iso].double() @ c["root"].double() + c["bias"].double()) <= 1e-6     # no in-edge: 0, not -inf
    _bars(figs, f"max {name} {cin}->{cout}")


@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("name,cls,cin,cout", EPILOGUE_REPS, ids=[r[0] for r in EPILOGUE_REPS])
def test_residual_and_relu_epilogue_vs_float64(name, cls, cin, cout, aggr):
    c = _case(cin, cout, aggr, 17 * cin + 1000 * cout)
    assert _aligned(c["we"], c["root"], c["bias"], c["res"])
    assert at.tiling_class(cin, cout, ops.any_width_plan(cin, cout, aggr=aggr)) == cls
    y, figs = _forward_figs(c, aggr, residual=True, relu=True)
    assert float(y.min()) == 0.0 and float((y == 0).float().mean()) > 0.1             # the ReLU acted
    _, f2 = _forward_figs(c, aggr, residual=True, relu=False)
    figs.update({"out_res": f2["out"], "out_res_row": f2["out_row"]})
    _bars(figs, f"epilogue {name} {cin}->{cout} {aggr}")


# ---- 4. long rows ---------------------------------------------------------------------------------------------------------------
HUB_FIGURES = {}


def _assert_hub_forward(err, e32, what):
    if e32 <= E32_WELL:
        assert err <= TOL_FWD, (what, err, "fp32 chain vs float64:", e32)
    assert err <= max(HUB_TOL_FWD, FWD_FACTOR * e32), (what, err, "fp32 chain vs float64:", e32)


@pytest.mark.parametrize("cin,cout", [(256, 132), (64, 255), (8, 8), (1, 1)])
def test_hub_rows_vs_float64_and_the_fp32_chain(cin, cout):
    """Node n - 1 has 8,192 in-edges, node 0 has 8,192 out-edges (k_any_dx_finish's ordered sum); add and mean.  W_e is a Linear
    of 4 edge attributes (no ReLU: no kink), computed once in fp32 on the host - the float64 reference, the fp32 chain and the
    kernel see the same W_e."""
    d = _dev()
    gen = torch.Generator().manual_seed(100 * cin + cout)
    n = 48
    src = torch.cat([torch.randint(0, n, (HUB,), generator=gen), torch.zeros(HUB, dtype=torch.int64),
                     torch.randint(0, n, (300,), generator=gen)])
    dst = torch.cat([torch.full((HUB,), n - 1), torch.randint(1, n - 1, (HUB + 300,), generator=gen)])
    perm = torch.randperm(src.numel(), generator=gen)
    ei = torch.stack([src[perm], dst[perm]])
    e = ei.shape[1]
    assert int((ei[1] == n - 1).sum()) == HUB and int((ei[0] == 0).sum()) >= HUB
    ea = torch.randn(e, 4, generator=gen)
    wl, bl = torch.randn(cin * cout, 4, generator=gen) / (2 * cin ** 0.5), torch.randn(cin * cout, generator=gen) / (2 * cin ** 0.5)
    x, root, bias, g = (torch.randn(n, cin, generator=gen), torch.randn(cin, cout, generator=gen) / cin ** 0.5,
                        torch.randn(cout, generator=gen), torch.randn(n, cout, generator=gen))
    # fp32 W_e, edge order - in the chunks (and so the bits) of the fp32 chain's own evaluation below
    w = torch.cat([torch.nn.functional.linear(ea[lo:lo + 2048], wl, bl) for lo in range(0, e, 2048)])
    plan = ops.any_width_plan(cin, cout)
    assert HUB >= 16 * plan["B"] * plan["ES"]                                         # many passes of the batch loop
    xd, wd, rootd, biasd, gd, eid = (t.to(d) for t in (x, w, root, bias, g, ei))
    assert _aligned(wd, rootd, biasd, gd)
    csr = ops.csr_for(eid, n)
    we = wd[csr.perm.long()].contiguous()
    for aggr in ("add", "mean"):
        y32 = nnconv_forward(x, ei, ea, [wl], [bl], root, bias, aggr=aggr, dtype=torch.float32, chunk_edges=2048).to(d)
        y = ops.nnconv_forward_edgeweights_any_raw(xd, csr, we, rootd, biasd, aggr)
        gx, gwe, groot, gbias = ops.nnconv_backward_edgeweights_any_raw(xd, csr, we, rootd, aggr, gd)
        lv = [t.double().requires_grad_(True) for t in (xd, wd, rootd, biasd)]
        ref = at.reference64(lv[0], eid, lv[1], lv[2], lv[3], aggr)
        (ref * gd.double()).sum().backward()
        hub = slice(n - 1, n)
        err, e32 = at.rel(y[hub], ref[hub]), at.rel(y32[hub], ref[hub])
        rwe = lv[1].grad[csr.perm.long()]
        figs = {"hub_row": err, "hub_row_fp32_chain": e32, "out": at.rel(y, ref), "out_fp32_chain": at.rel(y32, ref),
                "out_row": at.worst_row(y, ref), "dx_hub_source_row": at.rel(gx[0:1], lv[0].grad[0:1]), "dx": at.rel(gx, lv[0].grad),
                "dW_e": at.rel(gwe, rwe), "dW_e_row": at.worst_row(gwe, rwe), "droot": at.rel(groot, lv[2].grad),
                "dbias": at.rel(gbias, lv[3].grad)}
        HUB_FIGURES[(cin, cout, aggr)] = figs
        print(f"[tilings] hub {cin}->{cout} {aggr} V={plan['V']} LC={plan['LC']} R={plan['R']} ES={plan['ES']} B={plan['B']}: " +
              " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
        _assert_hub_forward(err, e32, ("hub row", cin, cout, aggr))
        _assert_hub_forward(figs["out"], figs["out_fp32_chain"], ("whole output", cin, cout, aggr))
        bad = {k: v for k, v in figs.items() if k.startswith("d") and not v <= TOL_BWD}
        assert not bad, (cin, cout, aggr, bad)
        del lv, ref, rwe, gwe


# ---- 5. offsets past 2^31 and 2^32 elements ----------------------------------------------------------------------------------
def test_offsets_past_2_to_the_32_elements_at_256_to_256():
    """E = 66,000 edges of 256 x 256: W_e and dW_e are 17.3 GB each, slot 32,768 starts at element 2^31 and slot 65,536 at 2^32.
    1,024 destinations of ~64 in-edges (rows short enough that the fixed 1e-5 row bar measures addressing, not the length of a
    sum - long rows have their own test above), the last ones owning the highest slots; W_e is generated in slot order (the
    edge list is the CSR's own).  The float64 reference runs in edge chunks."""
    d = _dev()
    free = torch.cuda.mem_get_info(d)[0]
    if free < 60 << 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free: the 2^32-offset case needs 60 GiB (two 17.3 GB tensors)")
    cin = cout = 256
    mat = cin * cout
    n, e = 1100, 66000
    gen = torch.Generator().manual_seed(5)
    dst = torch.sort(torch.randint(0, 1024, (e - 1024,), generator=gen))[0]
    dst = torch.sort(torch.cat([dst, torch.arange(1024)]))[0]                         # every destination 0 .. 1023 has an in-edge
    src = torch.randint(0, n, (e,), generator=gen)
    eid = torch.stack([src, dst]).to(d)
    csr = ops.csr_for(eid, n)
    assert csr.n_edges == e and e * mat > 2 ** 32 and int(csr.dst[65536]) >= 1000
    sei = csr.edge_index                                                              # slot order
    torch.manual_seed(6)
    we = torch.empty(e, mat, device=d)
    for lo in range(0, e, 4096):
        we[lo:lo + 4096].normal_(0, 1 / 16)
    x, root, bias, g = torch.randn(n, cin, device=d), torch.randn(cin, cout, device=d) / 16, torch.randn(cout, device=d), torch.randn(n, cout, device=d)
    y = ops.nnconv_forward_edgeweights_any_raw(x, csr, we, root, bias, "mean")
    gx, gwe, groot, gbias = ops.nnconv_backward_edgeweights_any_raw(x, csr, we, root, "mean", g)
    # float64 in chunks: m_e = x_j W_e, out = mean + update; dW_e = x_j^T gT_i, dx_j += W_e gT_i (+ root g_j)
    deg = torch.bincount(sei[1], minlength=n).clamp(min=1).double().unsqueeze(1)
    x64, g64 = x.double(), g.double()
    gt = g64 / deg
    agg = torch.zeros(n, cout, dtype=torch.float64, device=d)
    rdx = torch.zeros(n, cin, dtype=torch.float64, device=d)
    windows = [(0, 64), (32768 - 32, 32768 + 32), (65536 - 32, 65536 + 32)]
    worst_dw = 0.0
    for lo in range(0, e, 1024):
        sl = slice(lo, min(lo + 1024, e))
        w64 = we[sl].double().view(-1, cin, cout)
        s, t = sei[0, sl], sei[1, sl]
        agg.index_add_(0, t, torch.matmul(x64[s].unsqueeze(1), w64).squeeze(1))
        rdx.index_add_(0, s, torch.matmul(w64, gt[t].unsqueeze(2)).squeeze(2))
    ref = agg / deg + x64 @ root.double() + bias.double()
    rdx += g64 @ root.double().t()
    figs = {"out": at.rel(y, ref), "out_row": at.worst_row(y, ref), "dx": at.rel(gx, rdx), "dx_row": at.worst_row(gx, rdx),
            "droot": at.rel(groot, x64.t() @ g64), "dbias": at.rel(gbias, g64.sum(0))}
    for k, (a, b) in enumerate(windows):
        rdw = (x64[sei[0, a:b]].unsqueeze(2) * gt[sei[1, a:b]].unsqueeze(1)).reshape(b - a, mat)
        figs[f"dW_e[{a}:{b}]"] = at.rel(gwe[a:b], rdw)
        figs[f"dW_e[{a}:{b}]_row"] = at.worst_row(gwe[a:b], rdw)
    _bars(figs, f"2^32 offsets 256->256 E={e} ({e * mat * 4 / 1e9:.1f} GB per tensor)")


# ---- 6. misaligned pointers and the branches only the C ABI reaches --------------------------------------------------------
def _off_by_one_float(t):
    """The same values as a contiguous view one float into a larger buffer: 4 bytes off every 16-byte boundary the base is on."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 and v.contiguous().data_ptr() == v.data_ptr()
    return v


@pytest.mark.parametrize("which", ["root", "bias", "residual", "grad_out", "edge_weights"])
@pytest.mark.parametrize("cin,cout", [(24, 40), (96, 160)])
def test_a_misaligned_buffer_takes_the_dword_tiling(cin, cout, which):
    pa, pm = ops.any_width_plan(cin, cout, aligned=True), ops.any_width_plan(cin, cout, aligned=False)
    assert pa["V"] == 4 and pm["V"] == 1 and pm != pa
    c = _case(cin, cout, "mean", 3 * cin + cout, pm)
    assert _aligned(c["we"], c["root"], c["bias"], c["res"], c["g"])
    key = {"edge_weights": "we", "residual": "res", "grad_out": "g"}.get(which, which)
    m = dict(c)
    m[key] = _off_by_one_float(c[key])
    assert not _aligned(m[key]) and torch.equal(m[key], c[key])
    figs = {}
    if which != "grad_out":
        ya, _ = _forward_figs(c, "mean", residual=True, relu=True)
        ym, f = _forward_figs(m, "mean", residual=True, relu=True)
        figs.update(f)
        figs["out_vs_aligned"] = at.rel(ym, ya)
        assert figs["out_vs_aligned"] <= 1e-6
    if which in ("grad_out", "edge_weights"):
        ga = ops.nnconv_backward_edgeweights_any_raw(c["x"], c["csr"], c["we"], c["root"], "mean", c["g"])
        gm = ops.nnconv_backward_edgeweights_any_raw(m["x"], m["csr"], m["we"], m["root"], "mean", m["g"])
        for nm, u, v in zip(("dx", "dW_e", "droot", "dbias"), gm, ga):
            figs[f"{nm}_vs_aligned"] = at.rel(u, v)
            assert figs[f"{nm}_vs_aligned"] <= 1e-6, (nm, figs)
        figs.update(_backward_figs(m, "mean"))
    _bars(figs, f"misaligned {which} {cin}->{cout} (V=1 LC={pm['LC']} R={pm['R']} ES={pm['ES']})")


def _abi_backward(c, aggr, ordered=True, want=("x", "root", "bias"), n_nodes=None, n_edges=None):
    """gpde_nnconv_bwd_edgeweights_any through the binding itself.  Outputs not asked for are passed as NULL; buffers given are
    pre-filled with NaN so that an output the library should write and does not shows."""
    l = _lib.lib()
    d = _dev()
    cin, cout = c["x"].shape[1], c["g"].shape[1]
    n = c["n"] if n_nodes is None else n_nodes
    e = c["csr"].n_edges if n_edges is None else n_edges
    nan = lambda *s: torch.full(s, float("nan"), device=d)
    gx = nan(max(n, 1), cin) if "x" in want else None
    gwe = nan(max(e, 1), cin * cout)
    groot = nan(cin, cout) if "root" in want else None
    gbias = nan(cout) if "bias" in want else None
    ws = torch.empty(int(l.gpde_nnconv_bwd_edgeweights_any_workspace_bytes(n, e, cin, cout)), dtype=torch.uint8, device=d)
    if e == n_edges == 0 and n > 0:
        rowptr = torch.zeros(n + 1, dtype=torch.int32, device=d)
    else:
        rowptr = c["csr"].rowptr
    srp, ssl = c["csr"].src_order if ordered and e > 0 else (None, None)
    p = lambda t: None if t is None else t.data_ptr()
    rc = l.gpde_nnconv_bwd_edgeweights_any(c["x"].data_ptr(), n, c["we"].data_ptr(), e, rowptr.data_ptr(), c["csr"].src.data_ptr(), p(srp), p(ssl),
                                           c["root"].data_ptr(), _lib.GPDE_AGGR_ADD if aggr == "add" else _lib.GPDE_AGGR_MEAN, cin, cout,
                                           c["g"].data_ptr(), p(gx), gwe.data_ptr(), p(groot), p(gbias), ws.data_ptr(), ws.numel(),
                                           ops._stream_ptr(d))
    _lib.check(rc, "gpde_nnconv_bwd_edgeweights_any")
    torch.cuda.synchronize()
    return gx, gwe, groot, gbias


@pytest.mark.parametrize("cin,cout", [(24, 40), (7, 13), (130, 255)])
def test_backward_branches_reached_through_the_c_abi(cin, cout):
    c = _case(cin, cout, "mean", 19 * cin + cout)
    lv = [t.double().requires_grad_(True) for t in (c["x"], c["w"], c["root"], c["bias"])]
    (at.reference64(lv[0], c["ei"], lv[1], lv[2], lv[3], "mean") * c["g"].double()).sum().backward()
    rx, rwe, rroot, rbias = lv[0].grad, lv[1].grad[c["perm"]], lv[2].grad, lv[3].grad
    base = _abi_backward(c, "mean")
    figs = {"dx": at.rel(base[0], rx), "dW_e": at.rel(base[1], rwe), "droot": at.rel(base[2], rroot), "dbias": at.rel(base[3], rbias)}
    # no source order: fp32 atomics on grad_x - the float64 bar, not bitwise
    gx, gwe, groot, gbias = _abi_backward(c, "mean", ordered=False)
    figs.update({"dx_atomic": at.rel(gx, rx), "dx_atomic_row": at.worst_row(gx, rx)})
    assert torch.equal(gwe, base[1]) and torch.equal(groot, base[2]) and torch.equal(gbias, base[3])
    # grad_x not wanted, with and without a source order: the other outputs are the same bits
    for ordered in (True, False):
        gx, gwe, groot, gbias = _abi_backward(c, "mean", ordered=ordered, want=("root", "bias"))
        assert gx is None and torch.equal(gwe, base[1]) and torch.equal(groot, base[2]) and torch.equal(gbias, base[3])
    # grad_root / grad_bias NULL in turn, then both
    for want in (("x", "bias"), ("x", "root"), ("x",)):
        gx, gwe, groot, gbias = _abi_backward(c, "mean", want=want)
        assert torch.equal(gx, base[0]) and torch.equal(gwe, base[1])
        assert (groot is None) == ("root" not in want) and (gbias is None) == ("bias" not in want)
        assert groot is None or torch.equal(groot, base[2])
        assert gbias is None or torch.equal(gbias, base[3])
    # no edge, some nodes: the root term, X^T g and colsum g alone
    gx, gwe, groot, gbias = _abi_backward(c, "mean", n_edges=0)
    g64, x64 = c["g"].double(), c["x"].double()
    figs.update({"dx_no_edge": at.rel(gx, g64 @ c["root"].double().t()), "droot_no_edge": at.rel(groot, x64.t() @ g64),
                 "dbias_no_edge": at.rel(gbias, g64.sum(0))})
    assert bool(torch.isnan(gwe).all())                                               # nothing to write
    gx, _, _, _ = _abi_backward(c, "mean", n_edges=0, ordered=False)
    figs["dx_no_edge_atomic"] = at.rel(gx, g64 @ c["root"].double().t())
    # no node: sums over nothing
    gx, gwe, groot, gbias = _abi_backward(c, "mean", n_nodes=0, n_edges=0)
    assert float(groot.abs().max()) == 0.0 and float(gbias.abs().max()) == 0.0 and bool(torch.isnan(gx).all())
    _bars(figs, f"C ABI branches {cin}->{cout}")


def test_forward_without_edges_or_nodes_through_the_c_abi():
    c = _case(24, 40, "mean", 77)
    l = _lib.lib()
    d = _dev()
    n = c["n"]
    out = torch.full((n, 40), float("nan"), device=d)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=d)
    for aggr in (_lib.GPDE_AGGR_ADD, _lib.GPDE_AGGR_MEAN, _lib.GPDE_AGGR_MAX):
        out.fill_(float("nan"))
        rc = l.gpde_nnconv_fwd_edgeweights_any(c["x"].data_ptr(), n, None, 0, rowptr.data_ptr(), None, c["root"].data_ptr(), c["bias"].data_ptr(),
                                               None, 0, aggr, 24, 40, out.data_ptr(), ops._stream_ptr(d))
        _lib.check(rc, "gpde_nnconv_fwd_edgeweights_any")
        torch.cuda.synchronize()
        assert at.rel(out, c["x"].double() @ c["root"].double() + c["bias"].double()) <= 1e-6
    out.fill_(float("nan"))
    rc = l.gpde_nnconv_fwd_edgeweights_any(None, 0, None, 0, rowptr.data_ptr(), None, None, None, None, 0, _lib.GPDE_AGGR_ADD, 24, 40, None,
                                           ops._stream_ptr(d))
    _lib.check(rc, "gpde_nnconv_fwd_edgeweights_any")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---- 7. random widths through the module ------------------------------------------------------------------------------------
@st.composite
def module_cases(draw, cout_mod4):
    cin = draw(st.integers(1, 256))
    cout = draw(st.integers(1, 64)) * 4 if cout_mod4 else draw(st.integers(1, 255).filter(lambda v: v % 4 != 0))
    assume((cin, cout) != (64, 64))                             # the 64-wide kernels' widths: tests/test_gpu_hypothesis.py
    n = draw(st.integers(2, 200))
    cap = max(1, (256 << 20) // (cin * cout * 4))               # E * cin * cout * 4 bytes <= 256 MB (<= the 1 GB the oracle could hold)
    e = draw(st.integers(0, min(3000, cap)))
    return {"cin": cin, "cout": cout, "n": n, "e": e, "k0": draw(st.integers(1, 6)), "hidden": draw(st.integers(4, 24)),
            "aggr": draw(st.sampled_from(["mean", "add"])), "root": draw(st.booleans()), "bias": draw(st.booleans()),
            "old": draw(st.booleans()), "n_dst": draw(st.integers(1, n)), "dup": draw(st.integers(0, 32)),
            "loops": draw(st.integers(0, 32)), "seed": draw(st.integers(0, 2 ** 31 - 1))}


def _run_module_case(c):
    d = _dev()
    gen = torch.Generator().manual_seed(c["seed"])
    torch.manual_seed(c["seed"])
    n, e, cin, cout = c["n"], c["e"], c["cin"], c["cout"]
    src, dst = torch.randint(0, n, (e,), generator=gen), torch.randint(0, c["n_dst"], (e,), generator=gen)   # nodes >= n_dst: no in-edge
    dup, loops = min(c["dup"], e // 4), min(c["loops"], e // 4)
    if dup:
        src[:dup], dst[:dup] = src[-1].item(), dst[-1].item()
    if loops:
        src[e - loops:] = dst[e - loops:]
    perm = torch.randperm(e, generator=gen)
    src, dst = src[perm], dst[perm]
    ea = torch.randn(e, c["k0"], generator=gen)
    nn = DenseNet([c["k0"], c["hidden"], cin * cout])
    cls = gp.NNConv_old if c["old"] else gp.NNConv
    conv = cls(cin, cout, nn, aggr=c["aggr"], root_weight=c["root"], bias=c["bias"])
    lin = [l for l in conv.nn.layers if isinstance(l, torch.nn.Linear)]
    keep = edges_off_the_kink(ea, [l.weight.detach() for l in lin], [l.bias.detach() for l in lin]) if e else torch.ones(0, dtype=torch.bool)
    ei, ea = torch.stack([src[keep], dst[keep]]).to(d), ea[keep].contiguous().to(d)
    _check_against_oracle(conv.to(d), torch.randn(n, cin, generator=gen).to(d), ei, ea, c["aggr"],
                          f"hypothesis {cin}->{cout} {c['aggr']} n={n} e={ei.shape[1]} {cls.__name__} root={c['root']} bias={c['bias']}")


@pytest.mark.parametrize("cout_mod4", [True, False], ids=["cout%4==0", "cout%4!=0"])
@settings(max_examples=N_EXAMPLES, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
@given(data=st.data())
def test_random_widths_one_training_step_vs_the_oracle(cout_mod4, data):
    _run_module_case(data.draw(module_cases(cout_mod4)))
