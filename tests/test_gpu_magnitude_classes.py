"""GPU tier: the power-of-two scales of the split-f16 paths on graphs whose rows differ in magnitude
(tests/helpers/magnitude_classes.py: four disjoint, interleaved classes; x / grad_out / edge_attr of a class carry its own
power of two, one class exact zeros).  On randn inputs every per-row, per-node, per-step and per-tile maximum has one binary
exponent, so un-scaling a lane with another row's scale returns the right bits; here it does not.  Every case asserts

  * float64 per class: relative L2 over the rows of ONE class (out, grad_x by node; grad_edge_attr, grad_hidden by edge) at the
    project's bars - 1e-5 forward, 2e-5 gradients - for every class that is not zero;
  * exact zeros: rows of grad_x whose class has grad_out == 0, rows of grad_edge_attr / grad_hidden whose class has x == 0 or
    grad_out == 0; forward rows of the zero-x class are exactly `bias`;
  * the summed gradients (dW_l, db_l, droot, dbias) globally at 2e-5 - and once more with only the 2^-24 class's grad_out
    non-zero, the training-sized gradient on its own;
  * exact homogeneity where every scale on the path is per row or per node, or where there is none (gpde_edge_bwd_kernel, fp32
    MFMA; grad_x and dL/dU of gpde_edge_bwd3_kernel - full, hidden form and light pass - with ordered per-source sums: dZ by fp32 GEMM, one scale per destination node, per edge row of x, per row and step of H; the
    per-source reduction and the root term are plain fp32): one class's grad_out times 2^k (k = -7, +5) returns that class's
    rows times 2^k and every other row unchanged, bit for bit.  The atomics path sums in an arbitrary order: float64 bar only.

and, from the backward's trace / the forward's route queries and launch counts, that the intended branch ran.

Every case prints its figures before it asserts (lines starting with MAGNITUDE under `pytest -s`); the float32 composite of
tests/test_magnitude_host.py measures 1.5e-7 .. 4.8e-7 per class on the same inputs."""
import pytest
import torch

from graph_pde_amd import _lib, ops
from oracle.nnconv_oracle import nnconv_grads, nnconv_grads_shared, rel_l2
from tests.helpers import magnitude_classes as mc
from tests.helpers.bwd_walk import traced as _traced, walk as _walk, ws_for as _ws_for

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD = mc.TOL_FWD, mc.TOL_BWD
SOLO_F = tuple(f if k == mc.SMALL_CLASS else 0.0 for k, f in enumerate(mc.GRAD_OUT_F))
_DEV = {}


class _NoPack:
    """`packed` of a PackedMlp without the packed image (a null pointer to the library)."""
    @staticmethod
    def data_ptr():
        return None


class _OnDevice:
    def __init__(self, c):
        d = torch.device("cuda:0")
        self.c, self.d = c, d
        self.x, self.gout, self.ea = c.x.to(d), c.gout.to(d), c.ea.to(d)
        self.W, self.B = [w.to(d) for w in c.W], [b.to(d) for b in c.B]
        self.root, self.bias = c.root.to(d), c.bias.to(d)
        self.csr = ops.build_csr(c.ei.to(d), c.n)
        self.pm = ops.pack_mlp(self.W, self.B)
        self.perm = self.csr.perm.cpu().long()                     # CSR slot -> edge of c.ei
        self.cls_slot = c.cls_edge[self.perm]
        self.rowptr = self.csr.rowptr_host.tolist()
        assert torch.equal(self.cls_slot, c.cls_node[self.csr.dst.cpu().long()])


def _on_device(name, seed):
    if (name, seed) not in _DEV:
        _DEV[name, seed] = _OnDevice(mc.case(name, seed))
    return _DEV[name, seed]


def _report(what, errs):
    print("MAGNITUDE", what, "worst", f"{max(errs.values()):.2e}", {k: f"{v:.2e}" for k, v in errs.items()})


def _check_bwd(c, res, ref, fx, fg, what, attr=None, global_dx=False):
    """grad_x per class against float64 + exact zeros; the summed gradients globally; `attr`: dL/d edge_attr per class too."""
    gx, gW, gb, groot, gbias = res[:5]
    errs = {f"dx[{k}]": v for k, v in mc.per_class_errors(gx, ref[0], c.cls_node, mc.live_classes(fg)).items()}
    if global_dx:
        errs["dx"] = rel_l2(gx.cpu(), ref[0])
    for l in range(len(gW)):
        errs[f"dW{l + 1}"], errs[f"db{l + 1}"] = rel_l2(gW[l].cpu(), ref[1][l]), rel_l2(gb[l].cpu(), ref[2][l])
    errs["droot"], errs["dbias"] = rel_l2(groot.cpu(), ref[3]), rel_l2(gbias.cpu(), ref[4])
    dead = [k for k in range(mc.C) if fx[k] == 0 or fg[k] == 0]
    if attr is not None:
        errs.update({f"dattr[{k}]": v for k, v in mc.per_class_errors(attr, ref[5], c.cls_edge, mc.live_classes(fx, fg)).items()})
    _report(what, errs)
    bad = {k: v for k, v in errs.items() if not v <= TOL_BWD}
    assert not bad, (what, bad)
    assert mc.nonzero_rows(gx, c.cls_node, mc.zero_classes(fg)) == 0, what
    if attr is not None:
        assert mc.nonzero_rows(attr, c.cls_edge, dead) == 0, what
    return errs


def _check_homogeneous(c, call, base, cls_rows, what, pick=lambda r: [r[0]]):
    """One class's grad_out times 2^k: its rows of every tensor `pick` returns times 2^k, the others unchanged - the bits."""
    for cc in mc.live_classes(mc.GRAD_OUT_F):
        for k in (-7, 5):
            g = c.gout.clone()
            g[c.cls_node == cc] *= 2.0 ** k
            res = call(g.to("cuda:0"))
            torch.cuda.synchronize()
            for t, t0, cls in zip(pick(res), pick(base), cls_rows):
                t, t0 = t.cpu(), t0.cpu()
                mine = cls == cc
                assert torch.equal(t[mine], t0[mine] * 2.0 ** k), (what, cc, k, rel_l2(t[mine], t0[mine] * 2.0 ** k))
                assert torch.equal(t[~mine], t0[~mine]), (what, cc, k, "other classes moved", int((t[~mine] != t0[~mine]).sum()))


def _assert_eb3(recs, phase="full", kernel=3, **want):
    """Every chunk with edges ran the per-edge kernel `kernel` (3: gpde_edge_bwd3_kernel, rows >= 4 nodes; 1: the fp32 kernel)."""
    live = [q for q in recs if q["phase"] == phase and q["rows"]]
    assert live, recs
    for q in live:
        assert q["edge_kernel"] == kernel and (q["rows"] >= 4 * (q["nb"] - q["na"])) == (kernel == 3), q
        for k, v in want.items():
            assert q[k] == v, (k, v, q)
    return live


def _full_backward(v, aggr, what, want, ws=None, z=None, hidden=None, attr_in=None, need_attr=False, homogeneous=True,
                   name=None, kernel=3):
    """One input set through nnconv_backward_raw: the per-class checks, the solo call, homogeneity; returns the trace."""
    c = v.c
    call = lambda g: ops.nnconv_backward_raw(v.x, v.csr, v.ea if attr_in is None else attr_in, v.W, v.B, v.root, aggr, g, ws=ws,
                                             z_saved=z, hidden_saved=hidden, need_attr=need_attr)
    res, recs = _traced(lambda: call(v.gout))
    _assert_eb3(recs, kernel=kernel, **want)
    name = name or c.name
    ref = mc.reference_grads(name, c.seed, aggr)
    _check_bwd(c, res, ref, mc.X_F, mc.GRAD_OUT_F, what, attr=res[5] if need_attr else None)
    sres = call(c.solo_gout().to(v.d))                  # only the 2^-24 class has grad_out: the training-sized gradient on its own
    torch.cuda.synchronize()
    _check_bwd(c, sres, mc.reference_grads(name, c.seed, aggr, solo=True), mc.X_F, SOLO_F, what + ("solo",),
               attr=sres[5] if need_attr else None, global_dx=True)
    if homogeneous:
        _check_homogeneous(c, call, res, [c.cls_node], what)
    return res, recs


# ---- 1. eb3 + zagg32, ordered and atomic -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dx", ["ordered", "atomic"])
@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_eb3_zagg32(seed, aggr, dx, monkeypatch):
    v = _on_device("small", seed)
    if dx == "atomic":
        monkeypatch.setattr(ops, "DX_MODE", "atomic")
    _, recs = _full_backward(v, aggr, ("eb3_zagg32", seed, aggr, dx), dict(z="zagg32", ordered=int(dx == "ordered"), du_pre=0),
                             homogeneous=dx == "ordered")       # (atomics: the order of a source's sum is not fixed)
    assert len(recs) == 1 and mc.max_destinations_per_group(torch.sort(v.c.ei[1], stable=True).values) >= 3


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_fp32_edge_kernel(seed):
    """Mean in-degree 3 (rows < 4 nodes): gpde_edge_bwd_kernel, fp32 MFMA without any scale - the per-class bars and the exact
    homogeneity hold there by construction; a CSR group of 128 slots spans ~40 destinations of all four classes."""
    v = _on_device("low", seed)
    _full_backward(v, mc.aggr_of(seed), ("fp32_edge_kernel", seed), dict(z="zagg32", ordered=1), kernel=1)


# ---- 2. zagg16 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_zagg16(seed):
    """>= 32768 edges: Z re-aggregated on split f16 with one scale per call for x and one for H (class-dependent both):
    dW_3 is the observable; grad_x never sees Z (homogeneous as in case 1)."""
    v = _on_device("z16", seed)
    assert v.c.e >= 32768
    _full_backward(v, mc.aggr_of(seed), ("zagg16", seed), dict(z="zagg16", ordered=1))


# ---- 3. one chunk of >= 8192 rows, and the same inputs as two chunks ---------------------------------------------------------------

@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_big_chunk_and_two_chunks(seed):
    v = _on_device("big", seed)
    c, aggr = v.c, mc.aggr_of(seed)
    _, recs = _full_backward(v, aggr, ("big_chunk", seed), dict(z="zagg32", du_pre=1, call_amax=1, dw1="epilogue", h1="on_the_fly",
                                                                dw2="tn_split", du1="f16s"))
    assert len(recs) == 1 and recs[0]["rows"] >= 8192, recs
    ws_bytes = _ws_for(c.n, c.e, c.dims, 3 * c.e // 4)         # (the plan bounds the nodes of a chunk too: 3/4 of the edges give two)
    plan = ops.bwd_plan(c.n, c.e, c.dims, ws_bytes)
    want = _walk(v.rowptr, plan["edges_per_chunk"], plan["nodes_per_chunk"])
    assert len(want) == 2 and all(v.rowptr[b] - v.rowptr[a] < 8192 for a, b in want), want
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.d)
    _, recs2 = _full_backward(v, aggr, ("two_chunks", seed), dict(z="zagg32", du_pre=0, dw2="tn_acc"), ws=ws)
    assert [(q["na"], q["nb"]) for q in recs2] == want, (recs2, want)


# ---- 4. need_attr ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_grad_edge_attr(seed):
    """dL/d edge_attr per class: the per-row observable of the dU_2 row scales that feed the dU_1 GEMM."""
    v = _on_device("small", seed)
    _full_backward(v, mc.aggr_of(seed), ("grad_attr", seed), dict(grad_attr=1, du1="f16s"), need_attr=True, homogeneous=False)


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_grad_edge_attr_big_chunk(seed):
    """... and in a chunk of >= 8192 rows, where the row scales come out of the per-edge kernel (du_pre) or the split dW_2 pass."""
    v = _on_device("big", seed)
    _full_backward(v, mc.aggr_of(seed), ("grad_attr_big", seed), dict(grad_attr=1, du1="f16s", dw2="tn_split"), need_attr=True,
                   homogeneous=False)


# ---- 5. the hidden form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_hidden_form_and_accumulation(seed):
    v = _on_device("small", seed)
    c, aggr = v.c, mc.aggr_of(seed)
    H = ops.hidden_forward_raw(v.csr, v.ea, v.pm, v.W, v.B)[0]
    call = lambda g, x=v.x, acc=None: ops.nnconv_backward_hidden_raw(x, v.csr, H, c.dims, v.W[-1], v.B[-1], v.root, aggr, g,
                                                                     grad_hidden_acc=acc)
    res, recs = _traced(lambda: call(v.gout))
    _assert_eb3(recs, phase="conv", hlast="given", from_h=1, ordered=1)
    ref = mc.reference_grads("small", seed, aggr)
    gh0 = mc.grad_hidden_f64(c, aggr, c.x, c.gout)
    live, dead = mc.live_classes(mc.X_F, mc.GRAD_OUT_F), [mc.ZERO_CLASS]
    errs = {f"dx[{k}]": e for k, e in mc.per_class_errors(res[0], ref[0], c.cls_node, mc.live_classes(mc.GRAD_OUT_F)).items()}
    errs.update({f"dU[{k}]": e for k, e in mc.per_class_errors(res[1], gh0[v.perm], v.cls_slot, live).items()})
    errs["dW3"], errs["db3"] = rel_l2(res[2].cpu(), ref[1][2]), rel_l2(res[3].cpu(), ref[2][2])
    errs["droot"], errs["dbias"] = rel_l2(res[4].cpu(), ref[3]), rel_l2(res[5].cpu(), ref[4])
    _report(("hidden_form", seed), errs)
    assert all(e <= TOL_BWD for e in errs.values()), errs
    assert mc.nonzero_rows(res[0], c.cls_node, dead) == 0 and mc.nonzero_rows(res[1], v.cls_slot, dead) == 0
    # grad_x and dL/dU: per-node (dZ) and per-row (x, H) scales only
    _check_homogeneous(c, call, res, [c.cls_node, v.cls_slot], ("hidden_form", seed), pick=lambda r: [r[0], r[1]])

    # only the 2^-24 class has grad_out: every output of the conv phase globally
    sg = c.solo_gout()
    sres, sref = call(sg.to(v.d)), mc.reference_grads("small", seed, aggr, solo=True)
    errs = {"dx": rel_l2(sres[0].cpu(), sref[0]), "dU": rel_l2(sres[1].cpu(), mc.grad_hidden_f64(c, aggr, c.x, sg)[v.perm]),
            "dW3": rel_l2(sres[2].cpu(), sref[1][2]), "db3": rel_l2(sres[3].cpu(), sref[2][2]),
            "droot": rel_l2(sres[4].cpu(), sref[3]), "dbias": rel_l2(sres[5].cpu(), sref[4])}
    _report(("hidden_form", seed, "solo"), errs)
    assert all(e <= TOL_BWD for e in errs.values()), errs
    others = [k for k in range(mc.C) if k != mc.SMALL_CLASS]
    assert mc.nonzero_rows(sres[0], c.cls_node, others) == 0 and mc.nonzero_rows(sres[1], v.cls_slot, others) == 0

    # a second application ADDS its dL/dU (GPDE_BWD_ACCUMULATE_GRAD_HIDDEN): class factors rotated, other zero classes
    kx, kg = mc.APPLICATIONS[1]
    x1, g1 = c.operand("x", kx, 1), c.operand("grad_out", kg, 1)
    fx1, fg1 = mc.rotate(mc.X_F, kx), mc.rotate(mc.GRAD_OUT_F, kg)
    first = call(v.gout)
    res1, recs1 = _traced(lambda: call(g1.to(v.d), x1.to(v.d), first[1]))
    _assert_eb3(recs1, phase="conv", hlast="given", from_h=1)
    assert res1[1].data_ptr() == first[1].data_ptr()
    ref1 = nnconv_grads(x1, c.ei, c.ea, c.W, c.B, c.root, c.bias, aggr, g1, chunk_edges=mc.ORACLE_CHUNK)
    gh_sum = (gh0 + mc.grad_hidden_f64(c, aggr, x1, g1))[v.perm]
    live1 = mc.live_classes(fx1, fg1)
    errs = {f"dx[{k}]": e for k, e in mc.per_class_errors(res1[0], ref1[0], c.cls_node, mc.live_classes(fg1)).items()}
    errs.update({f"dU[{k}]": e for k, e in mc.per_class_errors(res1[1], gh_sum, v.cls_slot, sorted(set(live) | set(live1))).items()})
    errs["dW3"], errs["droot"] = rel_l2(res1[2].cpu(), ref1[1][2]), rel_l2(res1[4].cpu(), ref1[3])
    _report(("hidden_accumulate", seed), errs)
    assert all(e <= TOL_BWD for e in errs.values()), errs
    assert mc.nonzero_rows(res1[0], c.cls_node, mc.zero_classes(fg1)) == 0
    # a class dead in the second application keeps the first application's rows, bit for bit
    only0 = [k for k in live if k not in live1]
    for k in only0:
        assert torch.equal(res1[1][v.cls_slot.to(v.d) == k], res[1][v.cls_slot.to(v.d) == k]), k
    assert mc.nonzero_rows(res1[1], v.cls_slot, [k for k in range(mc.C) if k not in live and k not in live1]) == 0


# ---- 6. kept Z / kept H, node table ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_kept_z_and_kept_h(seed):
    v = _on_device("small", seed)
    c, aggr = v.c, mc.aggr_of(seed)
    z = torch.zeros(c.n, 64 * ops.hidden_width(c.dims), dtype=torch.float32, device=v.d)
    y = ops.nnconv_forward_raw(v.x, v.csr, v.ea, v.pm, v.root, v.bias, aggr, z_keep=z)
    _check_fwd(v, y, aggr, ("keep_z_forward", seed))
    _full_backward(v, aggr, ("kept_z", seed), dict(z="kept", from_h=0), z=z)
    H = ops.hidden_forward_raw(v.csr, v.ea, v.pm, v.W, v.B)[0]
    _full_backward(v, aggr, ("kept_h", seed), dict(z="kept", hlast="given", from_h=1), z=z, hidden=H)


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_node_table(seed):
    """Attributes gathered from a node table whose columns carry the class factors."""
    v = _on_device("table", seed)
    c = v.c
    na = ops.NodeAttr(c.table.to(v.d), c.sel)
    assert torch.equal(na.materialize(c.ei.to(v.d)), v.ea)
    _full_backward(v, mc.aggr_of(seed), ("node_table", seed), dict(z="zagg32"), attr_in=na)


# ---- 7. light + deferred -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", mc.SEEDS)
def test_backward_light_and_deferred(seed):
    """L = 3 applications of a shared module, x and grad_out with their class factors rotated between them: the deferred pass
    contracts K = 64 L per edge over stacks of mixed magnitude."""
    v = _on_device("small", seed)
    c, aggr, L = v.c, mc.aggr_of(seed), len(mc.APPLICATIONS)
    xs = [c.x] + [c.operand("x", kx, l) for l, (kx, _) in enumerate(mc.APPLICATIONS[1:], start=1)]
    gs = [c.gout] + [c.operand("grad_out", kg, l) for l, (_, kg) in enumerate(mc.APPLICATIONS[1:], start=1)]
    H = ops.hidden_forward_raw(v.csr, v.ea, v.pm, v.W, v.B)[0]
    h_nodes = next(i for i in range(1, c.n) if v.rowptr[i] >= c.e // 2)
    want = _walk(v.rowptr, c.e, c.n, h_nodes)

    def run():
        light = [ops.nnconv_backward_light_raw(xs[l].to(v.d), v.csr, v.ea, v.W, v.B, v.root, aggr, gs[l].to(v.d), hidden_part=H,
                                               hidden_nodes=h_nodes) for l in range(L)]
        return light, ops.nnconv_backward_deferred_raw([t.to(v.d) for t in xs], [t.to(v.d) for t in gs], v.csr, v.ea, v.W, v.B, aggr,
                                                       hidden_part=H, hidden_nodes=h_nodes)
    (light, (hW, hb)), recs = _traced(run)
    assert [(q["na"], q["nb"]) for q in recs if q["phase"] == "light"] == want * L, recs
    assert [(q["na"], q["nb"]) for q in recs if q["phase"] == "deferred"] == want, recs
    _assert_eb3(recs, phase="light", z="zagg32", ordered=1)
    for q in recs:
        if q["rows"]:
            assert (q["hlast"], q["from_h"]) == (("given", 1) if q["na"] < h_nodes else ("store", 0)), q
    rxs, rW, rb, rroot, rbias = nnconv_grads_shared(xs, c.ei, c.ea, c.W, c.B, c.root, c.bias, aggr, gs, chunk_edges=mc.ORACLE_CHUNK)
    errs = {}
    for l, (_, kg) in enumerate(mc.APPLICATIONS):
        fg = mc.rotate(mc.GRAD_OUT_F, kg)
        errs.update({f"dx{l}[{k}]": e for k, e in mc.per_class_errors(light[l][0], rxs[l], c.cls_node, mc.live_classes(fg)).items()})
        assert mc.nonzero_rows(light[l][0], c.cls_node, mc.zero_classes(fg)) == 0, l
    errs["dW3"], errs["db3"] = rel_l2(sum(r[1] for r in light).cpu(), rW[2]), rel_l2(sum(r[2] for r in light).cpu(), rb[2])
    errs["droot"], errs["dbias"] = rel_l2(sum(r[3] for r in light).cpu(), rroot), rel_l2(sum(r[4] for r in light).cpu(), rbias)
    for l in range(2):
        errs[f"dW{l + 1}"], errs[f"db{l + 1}"] = rel_l2(hW[l].cpu(), rW[l]), rel_l2(hb[l].cpu(), rb[l])
    _report(("light_deferred", seed), errs)
    assert all(e <= TOL_BWD for e in errs.values()), errs
    # the light pass runs gpde_edge_bwd3_kernel for grad_x alone: the same per-node / per-row scales, the same exact homogeneity
    light0 = lambda g: ops.nnconv_backward_light_raw(v.x, v.csr, v.ea, v.W, v.B, v.root, aggr, g, hidden_part=H, hidden_nodes=h_nodes)
    _check_homogeneous(c, light0, light[0], [c.cls_node], ("light", seed))

    # every application with only ITS 2^-24 class's grad_out: the training-sized gradients through the K = 64 L contraction
    gs = [mc.solo_of(g, c.cls_node, mc.rotate(mc.GRAD_OUT_F, kg)) for g, (_, kg) in zip(gs, mc.APPLICATIONS)]
    (light, (hW, hb)), _ = _traced(run)
    rxs, rW, rb, rroot, rbias = nnconv_grads_shared(xs, c.ei, c.ea, c.W, c.B, c.root, c.bias, aggr, gs, chunk_edges=mc.ORACLE_CHUNK)
    errs = {f"dx{l}": rel_l2(light[l][0].cpu(), rxs[l]) for l in range(L)}
    errs["dW3"], errs["db3"] = rel_l2(sum(r[1] for r in light).cpu(), rW[2]), rel_l2(sum(r[2] for r in light).cpu(), rb[2])
    errs["droot"], errs["dbias"] = rel_l2(sum(r[3] for r in light).cpu(), rroot), rel_l2(sum(r[4] for r in light).cpu(), rbias)
    for l in range(2):
        errs[f"dW{l + 1}"], errs[f"db{l + 1}"] = rel_l2(hW[l].cpu(), rW[l]), rel_l2(hb[l].cpu(), rb[l])
    _report(("light_deferred", seed, "solo"), errs)
    assert all(e <= TOL_BWD for e in errs.values()), errs


# ---- 8. forward --------------------------------------------------------------------------------------------------------------

def _check_fwd(v, y, aggr, what, name=None):
    c = v.c
    errs = {f"out[{k}]": e for k, e in mc.per_class_errors(y, mc.reference_out(name or c.name, c.seed, aggr), c.cls_node,
                                                         mc.live_classes(mc.X_F)).items()}
    _report(what, errs)
    assert all(e <= TOL_FWD for e in errs.values()), (what, errs)
    zero = y[(c.cls_node == mc.ZERO_CLASS).to(y.device)]
    assert torch.equal(zero, v.bias.expand_as(zero)), (what, "rows of the zero-x class are not exactly the bias")


@pytest.mark.parametrize("seed", mc.SEEDS)
@pytest.mark.parametrize("route", ["v3", "agg16", "8wave", "v6", "edge"])
def test_forward_fused(route, seed):
    name = {"v3": "small", "agg16": "small", "8wave": "z16", "v6": "z16", "edge": "low"}[route]
    precision = {"agg16": "f16split_agg16", "8wave": "f16split_8wave"}.get(route)
    v = _on_device(name, seed)
    c, aggr = v.c, mc.aggr_of(seed)
    r = ops.forward_route(v.csr, v.pm, aggr, precision=precision)
    assert r["association"] == "node" and r["n_chunks"] == 1 and r["edge_path"] == (route == "edge"), r
    if route in ("v3", "8wave"):
        assert r["kernel"] == "gpde_fused_f16v3_kernel", r
    if route == "8wave":                                       # ... where the default is the other kernel
        assert c.e >= 32768 and ops.fused_kernel_name(c.n, c.e, v.pm) == "gpde_fused_f16v6_kernel"
    if route == "v6":
        assert c.e >= 32768 and r["kernel"] == "gpde_fused_f16v6_kernel", r
    if route == "agg16":        # the forced split-f16 aggregation: on the one-wave-per-SIMD kernel where it is built (k1 >= 225)
        assert r["kernel"] == ("gpde_fused_f16v6_kernel" if c.dims[1] >= 225 else "gpde_fused_f16v3_kernel"), r
    _lib.profile_begin()
    y = ops.nnconv_forward_raw(v.x, v.csr, v.ea, v.pm, v.root, v.bias, aggr, precision=precision)
    torch.cuda.synchronize()
    prof = _lib.profile_end()
    if route == "edge":
        assert prof["gemm3"][1] >= 1, prof                     # the per-edge last layer
    else:
        assert prof["fused"][1] >= 1, prof
        assert (prof["prep"][1] > 0) == (route != "v3"), (route, prof)      # the split-f16 aggregation's pre-passes (one x / h scale per call)
    _check_fwd(v, y, aggr, ("forward", route, seed))


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_forward_from_hidden_with_recorded_absmax(seed):
    """hidden_forward_raw records max |H|; with it (and >= 32768 edges) the aggregation from H runs on split f16 under that one
    scale - H rows of the 2^6-attribute class next to those of the 2^-6 one."""
    v = _on_device("z16", seed)
    c, aggr = v.c, mc.aggr_of(seed)
    assert c.e >= 32768
    H, hmax = ops.hidden_forward_raw(v.csr, v.ea, v.pm, v.W, v.B)
    assert hmax is not None and float(hmax) == float(H.max()) > 0
    y = ops.nnconv_forward_hidden_raw(v.x, v.csr, H, v.pm, v.root, v.bias, aggr, hmax=hmax)
    y32 = ops.nnconv_forward_hidden_raw(v.x, v.csr, H, v.pm, v.root, v.bias, aggr, hmax=None)
    assert not torch.equal(y, y32)                             # the split-f16 aggregation did run
    _check_fwd(v, y, aggr, ("forward_hidden_absmax", seed))
    _check_fwd(v, y32, aggr, ("forward_hidden_fp32", seed))


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_forward_from_edge_weights(seed):
    """W_e from the split-f16 builder (k2 = 256: per-row scales of H), then the grouped 64-wide operator."""
    v = _on_device("small", seed)
    c, aggr = v.c, mc.aggr_of(seed)
    assert c.dims[2] >= 256
    H, _ = ops.hidden_forward_raw(v.csr, v.ea, v.pm, v.W[:-1] + [None], v.B[:-1] + [None], "f16split")
    we = ops.edge_weights_raw(H, v.pm, v.W[-1], v.B[-1])
    # without the packed image gpde_edge_weights_fwd takes its fp32 GEMM: other bits, the same W_e - the split-f16 builder did run
    we32 = ops.edge_weights_raw(H, ops.PackedMlp(v.pm.dims, _NoPack(), v.pm.dims_c), v.W[-1], v.B[-1])
    assert not torch.equal(we, we32) and rel_l2(we.cpu(), we32.cpu()) <= 2e-6
    y = ops.nnconv_forward_edgeweights_raw(v.x, v.csr, we, v.root, v.bias, aggr)
    torch.cuda.synchronize()
    _check_fwd(v, y, aggr, ("forward_edge_weights", seed))
