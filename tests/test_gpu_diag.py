"""The diagonal-kernel operator on the GPU (csrc/gpde_diagconv.hip; NNConvDiag / NNConvGaussian) against float64.

Reference: tests/helpers/diag_oracle.py, the reference's message / update (nn_conv.py:83-92, 174-190) as float64 torch ops on the
same float32 inputs; gradients by float64 autograd through it.  Bars are the project's (tests/test_gpu_width_tilings.py), row by
row with any_tilings.worst_row: forward 1e-5, gradients 2e-5 of max(row norm, rms row norm); a hub row of 8,192 in-edges
max(1e-6, 4 x e32), e32 the float32 torch chain's own distance from float64.  Graphs come from the kernel's own plan
(ops.diag_plan): in-degrees 0, 1 and one either side of every pass and chain boundary."""
import copy
import ctypes

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from tests.helpers import diag_oracle as do

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD = 1e-5, 2e-5
HUB_TOL_FWD, FWD_FACTOR = 1e-6, 4
HUB = 8192
ONE = ops._ONE_SET


def _dev():
    return torch.device("cuda:0")


def _class(w):
    p = ops.diag_plan(w)
    return (p["V"], p["LC"], p["ES"], p["per_lane"], p["consecutive"], p["active_lanes"] < p["lanes"])


def _widths():
    """The smallest width of every tiling class of ops.diag_plan, and the widths the issue names."""
    seen = {}
    for w in range(1, ops.ANY_MAX_WIDTH + 1):
        seen.setdefault(_class(w), w)
    return sorted(set(seen.values()) | {1, 3, 4, 63, 64, 65, 132, 256})


WIDTHS = _widths()


def _bars(figs, tag):
    print(f"[diag] {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    bad = {k: v for k, v in figs.items() if not v <= (TOL_FWD if k.startswith("out") else TOL_BWD)}
    assert not bad, (tag, bad)


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _case(w, seed, n_src=None, cind=None):
    """Ladder graph of the width's tiling; inputs on the device; the CSR; k in edge order (`k`) and in slot order (`ks`)."""
    d, gen = _dev(), torch.Generator().manual_seed(seed)
    ei, n, by_deg = do.ladder_graph(ops.diag_plan(w), gen, n_src=n_src)
    e = ei.shape[1]
    r = lambda *s: torch.randn(*s, generator=gen)
    cind = w if cind is None else cind
    ns = n if n_src is None else n_src
    c = dict(x=r(ns, w), k=r(e, w), root=r(cind, w) / cind ** 0.5, bias=r(w), res=r(n, w), g=r(n, w), xd=r(n, cind))
    c = {nm: t.to(d) for nm, t in c.items()}
    ei = ei.to(d)
    csr = ops.csr_for(ei, n) if n_src is None else ops.csr_for(ei, n, n_src=n_src)
    c.update(ei=ei, n=n, by_deg=by_deg, csr=csr, perm=csr.perm.long(), ks=c["k"][csr.perm.long()].contiguous(), w=w)
    return c


def _ref_and_grads(c, aggr, x_dst="one", root=True, bias=True):
    """float64: (out, {name: grad}) of sum(out * g)."""
    lv = {nm: c[nm].double().requires_grad_(True) for nm in ("x", "k", "root", "bias", "xd")}
    xd = lv["x"] if x_dst == "one" else lv["xd"] if x_dst == "two" else None
    ref = do.diag_reference(lv["x"], xd, c["ei"], lv["k"], lv["root"] if root else None, lv["bias"] if bias else None, aggr, n_dst=c["n"])
    if aggr != "max":
        (ref * c["g"].double()).sum().backward()
    return ref.detach(), {nm: t.grad for nm, t in lv.items()}


# ---- tilings --------------------------------------------------------------------------------------------------------------------
def test_the_widths_cover_every_tiling_class():
    assert {_class(w) for w in range(1, 257)} == {_class(w) for w in WIDTHS} and {1, 3, 4, 63, 64, 65, 132, 256} <= set(WIDTHS)
    assert {ops.diag_plan(w)["V"] for w in WIDTHS} == {1, 4} and {ops.diag_plan(w)["per_lane"] for w in WIDTHS} == {1, 2, 3, 4}


@pytest.mark.parametrize("w", WIDTHS)
def test_tiling_forward_and_gradients_vs_float64(w):
    c = _case(w, 1000 + w)
    p = ops.diag_plan(w)
    assert all(t.data_ptr() % 16 == 0 for t in (c["x"], c["ks"], c["root"], c["bias"], c["g"]))
    assert {0, 1, p["pass_edges"] - 1, p["pass_edges"] + 1, p["chain_edges"] - 1, p["chain_edges"], p["chain_edges"] + 1} <= set(c["by_deg"])
    assert int((c["ei"][0] == c["ei"][1]).sum()) > 0 and c["csr"].max_in_degree == max(c["by_deg"])
    for aggr in ("add", "mean", "max"):
        y = ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], aggr)
        ref, gr = _ref_and_grads(c, aggr)
        assert y.shape == ref.shape and bool(torch.isfinite(y).all())
        figs = {"out": _rel(y, ref), "out_row": do.worst_row(y, ref)}
        iso = c["by_deg"][0]                                    # no in-edge: the aggregate is 0, also under max
        assert _rel(y[iso], c["x"][iso].double() @ c["root"].double() + c["bias"].double()) <= 1e-6
        if aggr != "max":
            gx, gxd, gk, groot, gbias = ops.diagconv_backward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], aggr, c["g"])
            assert gxd is None and all(bool(torch.isfinite(t).all()) for t in (gx, gk, groot, gbias))
            rk = gr["k"][c["perm"]]
            figs.update({"dk": _rel(gk, rk), "dk_row": do.worst_row(gk, rk), "dx": _rel(gx, gr["x"]), "dx_row": do.worst_row(gx, gr["x"]),
                         "droot": _rel(groot, gr["root"]), "droot_row": do.worst_row(groot, gr["root"]), "dbias": _rel(gbias, gr["bias"])})
        _bars(figs, f"w={w} {aggr} V={p['V']} LC={p['LC']} ES={p['ES']} E={c['csr'].n_edges}")


@pytest.mark.parametrize("w", [3, 64, 132])
def test_residual_and_relu_epilogue_vs_float64(w):
    c = _case(w, 2000 + w)
    for aggr in ("add", "max"):
        y = ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], aggr, residual=c["res"], relu=True)
        x64 = c["x"].double()
        ref = do.diag_reference(x64, x64, c["ei"], c["k"].double(), c["root"].double(), c["bias"].double(), aggr, residual=c["res"].double(),
                                relu=True)
        assert float(y.min()) == 0.0 and float((y == 0).float().mean()) > 0.1             # the ReLU acted
        _bars({"out": _rel(y, ref), "out_row": do.worst_row(y, ref)}, f"epilogue w={w} {aggr}")


# ---- a hub row ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [256, 132])
def test_hub_row_vs_float64_and_the_fp32_chain(w):
    """Node n - 1 has 8,192 in-edges, node 0 has 8,192 out-edges (the source sum's long row)."""
    d, gen = _dev(), torch.Generator().manual_seed(300 + w)
    n = 48
    src = torch.cat([torch.randint(0, n, (HUB,), generator=gen), torch.zeros(HUB, dtype=torch.int64), torch.randint(0, n, (300,), generator=gen)])
    dst = torch.cat([torch.full((HUB,), n - 1), torch.randint(1, n - 1, (HUB + 300,), generator=gen)])
    perm = torch.randperm(src.numel(), generator=gen)
    ei = torch.stack([src[perm], dst[perm]]).to(d)
    e = ei.shape[1]
    assert HUB >= 16 * ops.diag_plan(w)["chain_edges"]                                  # many chains
    r = lambda *s: torch.randn(*s, generator=gen).to(d)
    x, k, root, bias, g = r(n, w), r(e, w), r(w, w) / w ** 0.5, r(w), r(n, w)
    csr = ops.csr_for(ei, n)
    ks = k[csr.perm.long()].contiguous()
    c = dict(x=x, k=k, root=root, bias=bias, g=g, xd=x, ei=ei, n=n)
    hub = slice(n - 1, n)
    for aggr in ("add", "mean"):
        y = ops.diagconv_forward_raw(x, ONE, csr, ks, root, bias, aggr)
        y32 = do.diag_reference(x, x, ei, k, root, bias, aggr)                           # the stock float32 torch chain
        ref, gr = _ref_and_grads(c, aggr)
        err, e32 = _rel(y[hub], ref[hub]), _rel(y32[hub], ref[hub])
        gx, _, gk, groot, gbias = ops.diagconv_backward_raw(x, ONE, csr, ks, root, aggr, g)
        rk = gr["k"][csr.perm.long()]
        figs = {"hub_row": err, "hub_row_fp32_chain": e32, "out_row": do.worst_row(y, ref), "dx_hub_source_row": _rel(gx[0:1], gr["x"][0:1]),
                "dx_row": do.worst_row(gx, gr["x"]), "dk_row": do.worst_row(gk, rk), "droot": _rel(groot, gr["root"]), "dbias": _rel(gbias, gr["bias"])}
        print(f"[diag] hub w={w} {aggr}: " + " ".join(f"{kk}={v:.2e}" for kk, v in figs.items()))
        assert err <= max(HUB_TOL_FWD, FWD_FACTOR * e32), (w, aggr, err, e32)
        assert figs["out_row"] <= TOL_FWD
        bad = {kk: v for kk, v in figs.items() if kk.startswith("d") and not v <= TOL_BWD}
        assert not bad, (w, aggr, bad)


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [3, 64])
def test_two_identical_calls_give_the_same_bits(w):
    c = _case(w, 4000 + w)
    assert int((c["ei"][0] == 1).sum()) >= c["csr"].n_edges // 5                        # one source feeds a quarter of the edges
    for aggr in ("add", "mean", "max"):
        a = ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], aggr)
        b = ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], aggr)
        assert torch.equal(a, b)
    for aggr in ("add", "mean"):
        ga = ops.diagconv_backward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], aggr, c["g"])
        gb = ops.diagconv_backward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], aggr, c["g"])
        assert all(torch.equal(s, t) for s, t in zip(ga, gb) if s is not None)


# ---- alignment and strides -------------------------------------------------------------------------------------------------------
def _off_by_one_float(t):
    """The same values as a contiguous view one float into a larger buffer: 4 bytes off every 16-byte boundary the base is on."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("w", [24, 64, 256])
def test_buffers_off_a_16_byte_boundary_give_the_aligned_bits(w):
    """w % 4 == 0: the aligned call reads 16 bytes per access, the others four dwords of the same channels - the same numbers added
    in the same order (ops.diag_plan: only V changes)."""
    c = _case(w, 5000 + w)
    assert ops.diag_plan(w)["V"] == 4 and ops.diag_plan(w, aligned=False)["V"] == 1
    for aggr in ("add", "mean", "max"):
        base = ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], aggr, residual=c["res"])
        for which in ("ks", "x", "out"):
            kw = {nm: c[nm] for nm in ("x", "ks")}
            out = None
            if which == "out":
                out = _off_by_one_float(torch.zeros_like(base))
            else:
                kw[which] = _off_by_one_float(c[which])
            y = ops._diagconv_forward(kw["x"], ONE, c["csr"], kw["ks"], c["root"], c["bias"], aggr, c["res"], False, out)
            assert (out is None or y is out) and torch.equal(y, base), (w, aggr, which)
    base = ops.diagconv_backward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], "mean", c["g"])
    for which in ("ks", "x", "g"):
        kw = {nm: c[nm] for nm in ("x", "ks", "g")}
        kw[which] = _off_by_one_float(c[which])
        got = ops.diagconv_backward_raw(kw["x"], ONE, c["csr"], kw["ks"], c["root"], "mean", kw["g"])
        assert all(torch.equal(s, t) for s, t in zip(got, base) if s is not None), (w, which)


def test_strided_inputs_are_made_dense_and_a_strided_out_is_refused():
    c = _case(24, 5555)
    base = ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], "add")
    wide = torch.zeros(c["n"], 48, device=_dev())
    wide[:, ::2] = c["x"]
    kt = c["ks"].t().contiguous().t()                           # column-major k
    assert not wide[:, ::2].is_contiguous() and not kt.is_contiguous()
    assert torch.equal(ops.diagconv_forward_raw(wide[:, ::2], ONE, c["csr"], kt, c["root"].t().contiguous().t(), c["bias"], "add"), base)
    got = ops.diagconv_backward_raw(wide[:, ::2], ONE, c["csr"], kt, c["root"], "add", c["g"].t().contiguous().t())
    want = ops.diagconv_backward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], "add", c["g"])
    assert all(torch.equal(s, t) for s, t in zip(got, want) if s is not None)
    with pytest.raises(ValueError, match="must be contiguous"):
        ops._diagconv_forward(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], "add", None, False, wide[:, ::2])
    with pytest.raises(ValueError, match=r"out must be float32 \["):
        ops._diagconv_forward(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], "add", None, False, torch.zeros(c["n"], 25, device=_dev()))
    with pytest.raises(ValueError, match="shares memory with x"):
        ops._diagconv_forward(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], "add", None, False, c["x"])
    with pytest.raises(ValueError, match=r"edge_kernel must be float32 \["):
        ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"][:, :23], c["root"], c["bias"], "add")
    with pytest.raises(ValueError, match=r"root must be float32 \[24,24\]"):
        ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"][:5], c["bias"], "add")
    with pytest.raises(ValueError, match="edge_kernel must be float32"):
        ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"].double(), c["root"], c["bias"], "add")
    with pytest.raises(RuntimeError, match="runs only on an MI355X"):
        ops.diagconv_forward_raw(c["x"].cpu(), ONE, c["csr"], c["ks"], c["root"], c["bias"], "add")
    with pytest.raises(NotImplementedError, match="'add' and 'mean'"):
        ops.diagconv_backward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], "max", c["g"])


# ---- two node sets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,cind,more_sources", [(12, 5, True), (64, 7, False), (65, 130, True)])
def test_two_node_sets_vs_float64(w, cind, more_sources):
    n_probe = len(do.ladder_degrees(ops.diag_plan(w))) + 3
    n_src = 2 * n_probe + 5 if more_sources else 7
    c = _case(w, 6000 + w, n_src=n_src, cind=cind)
    assert c["csr"].n_src == n_src != c["n"] and cind != w
    for aggr in ("add", "mean", "max"):
        y = ops.diagconv_forward_raw(c["x"], c["xd"], c["csr"], c["ks"], c["root"], c["bias"], aggr)
        ref, gr = _ref_and_grads(c, aggr, x_dst="two")
        figs = {"out": _rel(y, ref), "out_row": do.worst_row(y, ref)}
        if aggr != "max":
            gxs, gxd, gk, groot, gbias = ops.diagconv_backward_raw(c["x"], c["xd"], c["csr"], c["ks"], c["root"], aggr, c["g"])
            rk = gr["k"][c["perm"]]
            figs.update({"dx_src_row": do.worst_row(gxs, gr["x"]), "dx_dst_row": do.worst_row(gxd, gr["xd"]), "dk_row": do.worst_row(gk, rk),
                         "droot_row": do.worst_row(groot, gr["root"]), "dbias": _rel(gbias, gr["bias"])})
        _bars(figs, f"two sets w={w} in_dst={cind} n_src={n_src} n_dst={c['n']} {aggr}")
    # x_dst None: no root term, no grad_x_dst; root / bias None
    y = ops.diagconv_forward_raw(c["x"], None, c["csr"], c["ks"], None, c["bias"], "mean")
    ref, gr = _ref_and_grads(c, "mean", x_dst=None, root=False)
    gxs, gxd, gk, groot, gbias = ops.diagconv_backward_raw(c["x"], None, c["csr"], c["ks"], None, "mean", c["g"])
    assert gxd is None and groot is None
    _bars({"out_row": do.worst_row(y, ref), "dx_src_row": do.worst_row(gxs, gr["x"]), "dk_row": do.worst_row(gk, gr["k"][c["perm"]]),
           "dbias": _rel(gbias, gr["bias"])}, f"two sets w={w} without x_dst")
    with pytest.raises(ValueError, match="root without x_dst"):
        ops.diagconv_forward_raw(c["x"], None, c["csr"], c["ks"], c["root"], c["bias"], "add")
    y = ops.diagconv_forward_raw(c["x"], c["xd"], c["csr"], c["ks"], None, None, "add")
    ref, gr = _ref_and_grads(c, "add", x_dst="two", root=False, bias=False)
    gxs, gxd, gk, groot, gbias = ops.diagconv_backward_raw(c["x"], c["xd"], c["csr"], c["ks"], None, "add", c["g"], need_bias=False)
    assert groot is None and gbias is None and float(gxd.abs().max()) == 0.0           # no root: a zero grad_x_dst
    _bars({"out_row": do.worst_row(y, ref), "dx_src_row": do.worst_row(gxs, gr["x"])}, f"two sets w={w} without root and bias")
    gxs2, gxd2, _, _, _ = ops.diagconv_backward_raw(c["x"], c["xd"], c["csr"], c["ks"], c["root"], "add", c["g"], need_x_src=False, need_x_dst=False,
                                                    need_root=False)
    assert gxs2 is None and gxd2 is None


@pytest.mark.parametrize("w", [8, 132])
def test_one_node_set_is_the_two_set_call_given_one_table_twice(w):
    c = _case(w, 7000 + w)
    for aggr in ("add", "mean", "max"):
        one = ops.diagconv_forward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], c["bias"], aggr)
        assert torch.equal(one, ops.diagconv_forward_raw(c["x"], c["x"], c["csr"], c["ks"], c["root"], c["bias"], aggr))
        assert torch.equal(one, ops.diagconv_forward_raw(c["x"], c["x"].clone(), c["csr"], c["ks"], c["root"], c["bias"], aggr))
    for aggr in ("add", "mean"):
        gx, none, gk, groot, gbias = ops.diagconv_backward_raw(c["x"], ONE, c["csr"], c["ks"], c["root"], aggr, c["g"])
        for xd in (c["x"], c["x"].clone()):
            gxs, gxd, gk2, groot2, gbias2 = ops.diagconv_backward_raw(c["x"], xd, c["csr"], c["ks"], c["root"], aggr, c["g"])
            assert none is None and torch.equal(gx, gxs + gxd) and torch.equal(gk, gk2) and torch.equal(groot, groot2) and torch.equal(gbias, gbias2)
        # the same table twice without grad_x_dst is still a two-set call: grad_x_src holds no root term
        gxs3 = ops.diagconv_backward_raw(c["x"], c["x"], c["csr"], c["ks"], c["root"], aggr, c["g"], need_x_dst=False)[0]
        assert torch.equal(gxs3, gxs)


# ---- empty shapes ---------------------------------------------------------------------------------------------------------------
def test_no_edges_and_no_nodes():
    d, w, n = _dev(), 20, 9
    gen = torch.Generator().manual_seed(8)
    x, root, bias, g = (torch.randn(*s, generator=gen).to(d) for s in ((n, w), (w, w), (w,), (n, w)))
    csr = ops.build_csr(torch.empty(2, 0, dtype=torch.int64, device=d), n)
    k0 = torch.empty(0, w, device=d)
    upd = x.double() @ root.double() + bias.double()
    for aggr in ("add", "mean", "max"):
        assert _rel(ops.diagconv_forward_raw(x, ONE, csr, k0, root, bias, aggr), upd) <= 1e-6            # update() alone
    gx, _, gk, groot, gbias = ops.diagconv_backward_raw(x, ONE, csr, k0, root, "mean", g)
    assert tuple(gk.shape) == (0, w) and _rel(gx, g.double() @ root.double().t()) <= 1e-6
    assert _rel(groot, x.double().t() @ g.double()) <= 1e-6 and _rel(gbias, g.double().sum(0)) <= 1e-6
    gxs, gxd, _, _, _ = ops.diagconv_backward_raw(x, x.clone(), csr, k0, root, "add", g)
    assert float(gxs.abs().max()) == 0.0 and _rel(gxd, g.double() @ root.double().t()) <= 1e-6
    # no node: through the C ABI (a CSR of no node is one rowptr entry)
    l, rp = _lib.lib(), torch.zeros(1, dtype=torch.int32, device=d)
    st = ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream)
    assert l.gpde_diagconv_fwd(None, 0, None, 0, None, 0, rp.data_ptr(), None, root.data_ptr(), bias.data_ptr(), None, 0, 0, w, w, None, st) == 0
    ws = torch.empty(int(l.gpde_diagconv_bwd_workspace_bytes(0, w, w)), dtype=torch.uint8, device=d)
    groot.fill_(7.0), gbias.fill_(7.0)
    assert l.gpde_diagconv_bwd(None, 0, None, 0, None, 0, rp.data_ptr(), None, None, None, None, root.data_ptr(), 0, w, w, None, None, None, None,
                               groot.data_ptr(), gbias.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert float(groot.abs().max()) == 0.0 and float(gbias.abs().max()) == 0.0          # sums over nothing


# ---- offsets past 2^31 elements -------------------------------------------------------------------------------------------------
def test_offsets_past_2_to_the_31_elements_at_w_256():
    """E = 2^23 + 64 edges of w = 256: k is 8.6 GB and slot 2^23 starts at element 2^31.  4,096 destinations of 2,048 in-edges,
    then 8 destinations of 8 in-edges that own the highest slots: those 8 rows (and the dk rows of their 64 slots) are checked."""
    d = _dev()
    free = torch.cuda.mem_get_info(d)[0]
    if free < 24 << 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free: the 2^31-offset case needs 24 GiB (k and dk of 8.6 GB each)")
    w, nb, tail = 256, 4096, 8
    e = (1 << 23) + 64
    n = nb + tail
    dst = torch.cat([torch.arange(nb, device=d).repeat_interleave((1 << 23) // nb), nb + torch.arange(tail, device=d).repeat_interleave(8)])
    src = (torch.arange(e, device=d) * 7919) % n
    csr = ops.csr_for(torch.stack([src, dst]), n)
    assert csr.n_edges == e and e * w > 2 ** 31 and torch.equal(csr.perm.long(), torch.arange(e, device=d))      # sorted: slot = edge
    k = torch.empty(e, w, device=d)
    col = torch.arange(w, device=d, dtype=torch.float32) * 0.37
    for lo in range(0, e, 1 << 20):                             # a closed formula, filled on the device in 1 GB pieces
        hi = min(lo + (1 << 20), e)
        k[lo:hi] = torch.sin(((torch.arange(lo, hi, device=d) % 1013).float() * 0.11).unsqueeze(1) + col)
    gen = torch.Generator().manual_seed(9)
    x, root, bias, g = (torch.randn(*s, generator=gen).to(d) for s in ((n, w), (w, w), (w,), (n, w)))
    root /= 16
    y = ops.diagconv_forward_raw(x, ONE, csr, k, root, bias, "mean")
    gx, _, gk, groot, gbias = ops.diagconv_backward_raw(x, ONE, csr, k, root, "mean", g)
    lo = 1 << 23
    s, t = src[lo:], dst[lo:] - nb
    x64, g64 = x.double(), g.double()
    agg = torch.zeros(tail, w, dtype=torch.float64, device=d).index_add(0, t, x64[s] * k[lo:].double()) / 8
    ref = agg + x64[nb:] @ root.double() + bias.double()
    rdk = x64[s] * (g64[nb:][t] / 8)
    _bars({"out_row": do.worst_row(y[nb:], ref), "dk_row": do.worst_row(gk[lo:], rdk), "dbias": _rel(gbias, g64.sum(0))},
          f"2^31 offsets w=256 E={e} ({e * w * 4 / 1e9:.1f} GB)")
    assert bool(torch.isfinite(gx).all())


# ---- modules --------------------------------------------------------------------------------------------------------------------
def _golden_module(name):
    g = do.load_golden(name)
    w = g["x"].shape[1]
    if "W1" in g:
        nn = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, w))
        conv = gp.NNConvDiag(w, w, nn, aggr=g["aggr"])
        sd = {"nn.0.weight": g["W0"], "nn.0.bias": g["b0"], "nn.2.weight": g["W1"], "nn.2.bias": g["b1"]}
    else:
        conv = gp.NNConvGaussian(w, w, torch.nn.Linear(1, w), aggr=g["aggr"])
        sd = {"nn.weight": g["W0"], "nn.bias": g["b0"]}
    conv.load_state_dict(dict(sd, root=g["root"], bias=g["bias"]))
    return g, conv


@pytest.mark.parametrize("name", ["diag_w8", "diag_gauss_w64"])
def test_modules_reproduce_the_reference(name):
    g, conv = _golden_module(name)
    d = _dev()
    before = _lib.n_native_calls
    with torch.no_grad():
        y = conv.to(d)(g["x"].to(d), g["edge_index"].to(d), g["edge_attr"].to(d))
    assert _lib.n_native_calls == before + 1                   # gather, message, aggregate and update(): ONE native call
    figs = {"out": _rel(y, g["out_f64"].to(d)), "out_row": do.worst_row(y, g["out_f64"].to(d))}
    # CPU-resident module and inputs: `nn` runs where the module lives (the CPU's float32 k differs from the device's in its last
    # bits, so the bar is the same 1e-5 against float64, not equality), the operator is staged and the result returns to the CPU
    before = _lib.n_native_calls
    with torch.no_grad():
        yc = conv.cpu()(g["x"], g["edge_index"], g["edge_attr"])
    assert yc.device.type == "cpu" and _lib.n_native_calls == before + 1
    figs.update({"out_cpu_resident": _rel(yc, g["out_f64"]), "out_cpu_resident_row": do.worst_row(yc, g["out_f64"])})
    _bars(figs, f"golden {name}")


def _net(kind, w):
    if kind == "batchnorm":
        # (no bias in front of BatchNorm: its gradient is an exact 0 - the mean is subtracted - and has no relative error)
        return torch.nn.Sequential(torch.nn.Linear(3, 16, bias=False), torch.nn.BatchNorm1d(16), torch.nn.ReLU(), torch.nn.Linear(16, w))
    return torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, w))


@pytest.mark.parametrize("kind,aggr", [("batchnorm", "add"), ("batchnorm", "mean"), ("chain", "add"), ("chain", "mean"), ("chain", "max")])
def test_training_step_gradients_vs_float64(kind, aggr):
    """add / mean through DiagConvFunction; max (one node set) through MessagePassing.propagate over the torch message()."""
    d, w = _dev(), 24
    torch.manual_seed(11)
    c = _case(w, 9000 + len(kind) + len(aggr))
    ea = torch.randn(c["csr"].n_edges, 3, device=d)
    conv = gp.NNConvDiag(w, w, _net(kind, w), aggr=aggr).to(d).train()
    conv64 = copy.deepcopy(conv).double()
    x = c["x"].clone().requires_grad_(True)
    y = conv(x, c["ei"], ea)
    (y * c["g"]).sum().backward()
    x64 = c["x"].double().requires_grad_(True)
    ref = do.diag_reference(x64, x64, c["ei"], conv64.nn(ea.double()), conv64.root, conv64.bias, aggr)
    (ref * c["g"].double()).sum().backward()
    figs = {"out": _rel(y, ref), "out_row": do.worst_row(y, ref), "dx": _rel(x.grad, x64.grad), "dx_row": do.worst_row(x.grad, x64.grad)}
    for (nm, p), (_, p64) in zip(conv.named_parameters(), conv64.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), nm
        figs["d" + nm] = _rel(p.grad, p64.grad)
    _bars(figs, f"training step {kind} {aggr}")


def test_max_with_a_gradient_on_two_node_sets_is_refused():
    d = _dev()
    conv = gp.NNConvDiag((8, 5), 8, _net("chain", 8), aggr="max").to(d)
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=d)
    xs, xd, ea = torch.randn(6, 8, device=d), torch.randn(4, 5, device=d), torch.randn(3, 3, device=d)
    with pytest.raises(NotImplementedError, match="aggr='max' with a gradient"):
        conv((xs, xd), ei, ea, size=(6, 4))
    with torch.no_grad():
        y = conv((xs, xd), ei, ea, size=(6, 4))
    ref = do.diag_reference(xs.double(), xd.double(), ei, conv.nn(ea).double(), conv.root.double(), conv.bias.double(), "max")
    assert do.worst_row(y, ref) <= TOL_FWD


@pytest.mark.parametrize("flow", ["source_to_target", "target_to_source"])
def test_module_between_two_node_sets_and_both_flows(flow):
    d, w, cind = _dev(), 12, 5
    c = _case(w, 9500, n_src=11, cind=cind)
    torch.manual_seed(12)
    conv = gp.NNConvDiag((w, cind), w, _net("chain", w), aggr="mean", flow=flow).to(d)
    conv64 = copy.deepcopy(conv).double()
    ea = torch.randn(c["csr"].n_edges, 3, device=d)
    ei_call = c["ei"] if flow == "source_to_target" else c["ei"].flip(0)      # the module reads (source, target) by its flow
    xs, xd = c["x"].clone().requires_grad_(True), c["xd"].clone().requires_grad_(True)
    y = conv((xs, xd), ei_call, ea, size=(11, c["n"]))
    (y * c["g"]).sum().backward()
    xs64, xd64 = c["x"].double().requires_grad_(True), c["xd"].double().requires_grad_(True)
    ref = do.diag_reference(xs64, xd64, c["ei"], conv64.nn(ea.double()), conv64.root, conv64.bias, "mean")
    (ref * c["g"].double()).sum().backward()
    figs = {"out_row": do.worst_row(y, ref), "dx_src_row": do.worst_row(xs.grad, xs64.grad), "dx_dst_row": do.worst_row(xd.grad, xd64.grad)}
    for (nm, p), (_, p64) in zip(conv.named_parameters(), conv64.named_parameters()):
        figs["d" + nm] = _rel(p.grad, p64.grad)
    _bars(figs, f"module two sets {flow}")
    # one node set under the same flow (the constructor re-draws `nn`, as the reference's does: the float64 copy is taken after it)
    one = gp.NNConvDiag(w, w, conv.nn, aggr="add", flow=flow).to(d)
    conv64 = copy.deepcopy(one).double()
    n1 = 11
    ei1 = torch.stack([c["ei"][0], c["ei"][1] % n1])
    with torch.no_grad():
        y1 = one(c["x"], ei1 if flow == "source_to_target" else ei1.flip(0), ea)
    ref1 = do.diag_reference(c["x"].double(), c["x"].double(), ei1, conv64.nn(ea.double()), one.root.double(), one.bias.double(), "add")
    assert do.worst_row(y1, ref1.detach()) <= TOL_FWD


@pytest.mark.parametrize("aggr", ["add", "max"])
def test_fused_residual_and_relu_inference_is_the_composed_value(aggr):
    """The epilogue adds the residual to the rounded float32 result and clamps: ONE rounding of the sum, as `residual + out` by
    torch rounds once - the two agree to 1 ulp per element (in fact they are the same additions)."""
    d, w = _dev(), 64
    c = _case(w, 9700)
    torch.manual_seed(13)
    conv = gp.NNConvDiag(w, w, _net("chain", w), aggr=aggr).to(d)
    ea = torch.randn(c["csr"].n_edges, 3, device=d)
    with torch.no_grad():
        before = _lib.n_native_calls
        fused = conv(c["x"], c["ei"], ea, residual=c["res"], activation="relu")
        assert _lib.n_native_calls == before + 1
        composed = torch.relu(c["res"] + conv(c["x"], c["ei"], ea))
    ulps = (fused.view(torch.int32) - composed.view(torch.int32)).abs()                # both >= 0: ordered like their bit patterns
    assert float(fused.min()) == 0.0 and int(ulps.max()) <= 1
    if aggr == "add":                                           # with a gradient: the unfused operator, then the same torch ops
        x = c["x"].clone().requires_grad_(True)
        y = conv(x, c["ei"], ea, residual=c["res"], activation="relu")
        assert y.requires_grad and int((y.detach().view(torch.int32) - composed.view(torch.int32)).abs().max()) <= 1


def test_a_csr_from_radius_csr_as_edge_index_and_node_attributes():
    d, w = _dev(), 16
    gen = torch.Generator().manual_seed(14)
    pos = torch.rand(200, 2, generator=gen).to(d)
    csr = ops.radius_csr(pos, 0.2)
    ei = csr.edge_index                                         # slot order: perm is the identity
    torch.manual_seed(15)
    conv = gp.NNConvDiag(w, w, torch.nn.Sequential(torch.nn.Linear(4, 16), torch.nn.ReLU(), torch.nn.Linear(16, w)), aggr="mean").to(d)
    x = torch.randn(200, w, device=d)
    ea = torch.cat([pos[ei[0]], pos[ei[1]]], dim=1)             # attributes in slot order
    with torch.no_grad():
        y = conv(x, csr, ea)
        y_list = conv(x, ei, ea)
        y_na = conv(x, csr, ops.NodeAttr(pos, [(0, 0), (0, 1), (1, 0), (1, 1)]))
        y_na_list = conv(x, ei[:, torch.randperm(ei.shape[1], generator=gen).to(d)], ops.NodeAttr(pos, [(0, 0), (0, 1), (1, 0), (1, 1)]))
        k64 = copy.deepcopy(conv.nn).double()(ea.double())
    ref = do.diag_reference(x.double(), x.double(), ei, k64, conv.root.double(), conv.bias.double(), "mean")
    assert csr.n_edges > 1000 and do.worst_row(y, ref.detach()) <= TOL_FWD
    assert torch.equal(y, y_list) and torch.equal(y, y_na) and do.worst_row(y_na_list, ref.detach()) <= TOL_FWD


def test_the_module_replays_under_capture_with_the_same_bits():
    d, w = _dev(), 64
    c = _case(w, 9900)
    torch.manual_seed(16)
    conv = gp.NNConvGaussian(w, w, torch.nn.Linear(1, w), aggr="mean").to(d)
    with torch.no_grad():
        conv.nn.weight.uniform_(0.6, 1.4)
        conv.nn.bias.zero_()
    ea = torch.cat([2 * torch.rand(c["csr"].n_edges, 1, device=d) - 1, 0.5 + torch.rand(c["csr"].n_edges, 2, device=d)], dim=1)
    with torch.no_grad():
        direct = conv(c["x"], c["ei"], ea).clone()
        fwd = gp.capture(lambda t: conv(t, c["ei"], ea), c["x"])
        assert torch.equal(fwd(c["x"]), direct) and torch.equal(fwd(c["x"]), direct) and fwd.replays == 2
        x2 = torch.randn_like(c["x"])
        assert torch.equal(fwd(x2), conv(x2, c["ei"], ea))
    k64 = do.gaussian_kernel(ea.double(), conv.nn.weight.double().view(-1) + conv.nn.bias.double())
    ref = do.diag_reference(c["x"].double(), c["x"].double(), c["ei"], k64, conv.root.double(), conv.bias.double(), "mean")
    assert do.worst_row(direct, ref.detach()) <= TOL_FWD
