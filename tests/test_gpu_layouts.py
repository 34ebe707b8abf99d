"""GPU tier of the operand-layout contract (DESIGN.md "Operand layouts").

Every float operand of every native entry family is handed over once in each awkward memory layout of tests/helpers/layouts.py
(a column slice of a wider buffer, every other row, transposed storage, dense but 4 / 8 bytes off a 16-byte boundary, stride 0)
while the other operands stay dense.  The call must return the BITS of the all-dense call (same kernel, same values, same
summation order: torch.equal, no tolerance), leave the operand's own bits alone and leave the sentinel floats around it
untouched.  A caller-given `out` / `z_keep` / `acc` that is dense and aligned in the middle of a larger buffer is filled with
the same bits, guards intact; an awkward one raises ValueError and keeps its sentinels.  One float64 oracle comparison per
family on the row_strided call (the project's bars: forward 1e-5, gradients 2e-5) sees a change that broke the awkward and the
dense call alike.

On the 64-wide families the offset4 / offset8 cases go through the wrappers only: ops._operand realigns them, no 64-wide kernel
receives a pointer that is not 16-byte aligned.  The any-width kernels receive them and take their dword tiling."""
import os

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from oracle.nnconv_oracle import nnconv_forward, nnconv_grads, rel_l2
from tests.helpers.kinks import edges_off_the_kink
from tests.helpers.layouts import all_sentinel, as_layout, carve_out, guards_intact, sentinel_like

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
TOL_FWD, TOL_BWD = 1e-5, 2e-5
# GPDE_LAYOUT_KINDS=row_strided,transposed_storage restricts the sweeps (a mutation check of a 64-wide wrapper must not hand its
# kernels the offset kinds: tests/test_gpu_layouts.py is then run without them)
_ALLOWED = [k for k in os.environ.get("GPDE_LAYOUT_KINDS", "").split(",") if k]
KINDS_2D = tuple(k for k in ("row_strided", "row_skipping", "transposed_storage", "offset4", "offset8") if not _ALLOWED or k in _ALLOWED)
KINDS_1D = tuple(k for k in ("row_strided", "row_skipping", "offset4", "offset8") if not _ALLOWED or k in _ALLOWED)

# route -> (n, e, kernel-MLP widths, precision): the smallest graph on which that route's kernel has a full and a partial tile
ROUTES = {
    "f16v3_k40": (70, 300, [3, 40, 64, 4096], None),          # split-f16 8-wave kernel, the narrow k1 class
    "f16v3_k256": (70, 300, [3, 256, 256, 4096], None),       # ... the k1 class that the one-wave-per-SIMD kernel shares
    "generic": (70, 300, [3, 32, 4096], None),                # fp32 MFMA kernel (2 Linear layers)
    "f32": (70, 300, [3, 256, 256, 4096], "f32"),             # fp32 MFMA kernel by precision
    "edge": (2000, 4600, [3, 256, 256, 4096], None),          # per-edge last layer of low in-degree graphs
    "f16v6": (320, 33000, [3, 256, 256, 4096], None),         # one wave per SIMD, split-f16 aggregation, slot-ordered attributes
}
_CASES = {}


def _graph(n, e, g, n_src=None):
    """[2, e] edges in shuffled order: node n - 1 without in-edges, one destination (3) of 40 in-edges, a self-loop, a duplicate."""
    ns = n if n_src is None else n_src
    src = torch.randint(0, ns, (e,), generator=g)
    dst = torch.randint(0, n - 1, (e,), generator=g)
    dst[:40] = 3
    src[40] = dst[40] = min(5, ns - 1)
    src[41], dst[41] = src[42], dst[42]
    p = torch.randperm(e, generator=g)
    return torch.stack([src[p], dst[p]])


def _mlp_params(dims, g):
    W = [torch.empty(dims[i + 1], dims[i]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    B = [torch.empty(dims[i + 1]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    return W, B


def _case(route):
    """Host tensors, device graph and packed MLP of a route, built once and shared (never modified)."""
    if route in _CASES:
        return _CASES[route]
    n, e, dims, precision = ROUTES[route]
    g = torch.Generator().manual_seed(1234 + len(route))
    ei = _graph(n, e, g)
    ea = torch.randn(e, dims[0], generator=g)
    W, B = _mlp_params(dims, g)
    keep = edges_off_the_kink(ea, W, B)
    ei, ea = ei[:, keep].contiguous(), ea[keep].contiguous()
    c = dict(route=route, n=n, e=int(ei.shape[1]), dims=dims, precision=precision, ei=ei, ea=ea, W=W, B=B,
             x=torch.randn(n, 64, generator=g), root=torch.empty(64, 64).uniform_(-0.125, 0.125, generator=g),
             bias=torch.empty(64).uniform_(-0.125, 0.125, generator=g), res=torch.randn(n, 64, generator=g),
             g=torch.randn(n, 64, generator=g))
    c["csr"] = ops.build_csr(ei.to(D), n)
    c["Wd"], c["Bd"] = [w.to(D) for w in W], [b.to(D) for b in B]
    c["pm"] = ops.pack_mlp(c["Wd"], c["Bd"])
    assert int(c["csr"].rowptr_host[-1]) == c["e"] and c["csr"].max_in_degree >= 40
    _CASES[route] = c
    return c


def _assert_route(c, aggr="mean"):
    r = ops.forward_route(c["csr"], c["pm"], aggr, precision=c["precision"])
    assert r["association"] == "node", r
    name = ops.fused_kernel_name(c["n"], c["e"], c["pm"], c["precision"])
    route = c["route"]
    if route.startswith("f16v3"):
        assert r["kernel"] == name == "gpde_fused_f16v3_kernel" and not r["edge_path"], r
    elif route in ("generic", "f32"):
        assert r["kernel"] == name == "gpde_fused_kernel" and not r["edge_path"], r
    elif route == "edge":
        assert r["edge_path"] and c["e"] >= 4096, r
    else:
        assert r["kernel"] == name == "gpde_fused_f16v6_kernel" and not r["edge_path"] and c["e"] >= 32768, r


def _bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _flat(res):
    out = []
    for r in (res if isinstance(res, (tuple, list)) else [res]):
        out.extend(_flat(r) if isinstance(r, (tuple, list)) else [r])
    return out


def _kinds(t, name, extra=()):
    return (KINDS_2D if t.dim() == 2 else KINDS_1D) + tuple(extra.get(name, ()) if isinstance(extra, dict) else ())


def _sweep(call, operands, expanded=None, what="", retile=None):
    """`call(**operands)` with every operand in every awkward layout, one at a time: the bits of the all-dense call, operand and
    guards untouched.  `expanded`: {operand: constant} - that operand also as a stride-0 tensor, compared with the dense call on the
    same constant.  `retile`: {operand: indices of the outputs whose launch receives it} for the operands of an any-width call that
    its kernels read with 16-byte accesses - offset4 / offset8 of one of them moves those launches to the dword tiling (V = 1), whose
    sums run in another order.  The reference for them is the call with the FIRST operand of `retile` (the per-edge weights, which
    every launch receives) at offset4: the same kernels in the same V = 1 tiling.  Every retiled output must carry that call's bits,
    every other output the dense call's; the offset4 results are returned as `name@offset4` for the caller's oracle bar.
    Returns (dense result, {operand: result of its row_strided call})."""
    dense = {k: (None if v is None else as_layout(v, "dense")[0]) for k, v in operands.items()}
    base = _flat(call(**dense))
    again = _flat(call(**dense))
    torch.cuda.synchronize()
    assert all(_bits_equal(a, b) for a, b in zip(base, again)), (what, "the dense call twice gives different bits")
    bad, strided, v1 = [], {}, None
    retile = retile or {}
    if retile and "offset4" in KINDS_2D:
        first = next(iter(retile))
        v1 = _flat(call(**{**dense, first: as_layout(operands[first], "offset4")[0]}))
    for name, t in operands.items():
        if t is None:
            continue
        for kind in _kinds(t, name):
            view, backing = as_layout(t, kind)
            got = _flat(call(**{**dense, name: view}))
            torch.cuda.synchronize()
            if name in retile and kind in ("offset4", "offset8"):
                strided.setdefault(name + "@offset4", got)
                want = [v1[i] if i in retile[name] else base[i] for i in range(len(base))]
                if len(got) != len(want) or not all(_bits_equal(a, b) for a, b in zip(got, want)):
                    bad.append((what, name, kind, "V = 1", [i for i, (a, b) in enumerate(zip(got, want)) if not _bits_equal(a, b)]))
            elif len(got) != len(base) or not all(_bits_equal(a, b) for a, b in zip(got, base)):
                bad.append((what, name, kind, [i for i, (a, b) in enumerate(zip(got, base)) if not _bits_equal(a, b)]))
            guards_intact(backing)
            if kind == "row_strided":
                strided[name] = got
    for name, const in ({} if (_ALLOWED and "expanded" not in _ALLOWED) else (expanded or {})).items():
        full = torch.full_like(operands[name], const)
        ref = _flat(call(**{**dense, name: as_layout(full, "dense")[0]}))
        view, backing = as_layout(full, "expanded")
        got = _flat(call(**{**dense, name: view}))
        torch.cuda.synchronize()
        if not all(_bits_equal(a, b) for a, b in zip(got, ref)):
            bad.append((what, name, "expanded"))
        guards_intact(backing)
    assert not bad, bad
    return base, strided


def _dev(c, *names):
    return {k: c[k].to(D) for k in names}


# ---------------------------------------------------------------------------------------------------------------------------
# fused forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_fused_forward_layouts(route):
    c = _case(route)
    _assert_route(c)
    csr, pm, prec = c["csr"], c["pm"], c["precision"]

    def plain(x, ea, root, bias):
        return ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "mean", precision=prec)

    def glue(x, ea, root, bias, res):
        return ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "add", precision=prec, residual=res, relu=True)

    calls = _lib.n_native_calls
    base, strided = _sweep(plain, _dev(c, "x", "ea", "root", "bias"), expanded={"bias": 0.25}, what=route)
    assert _lib.n_native_calls > calls
    ref = nnconv_forward(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], aggr="mean", dtype=torch.float64, chunk_edges=4096)
    err = rel_l2(strided["x"][0].cpu(), ref)
    print(f"{route}: forward (row_strided x) vs float64 {err:.3e}")
    assert err <= TOL_FWD, err
    operands = _dev(c, "x", "ea", "root", "bias")
    operands["res"] = c["res"].to(D)
    base, strided = _sweep(glue, operands, what=route + " residual+relu")
    ref = torch.relu(c["res"].double() + nnconv_forward(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], aggr="add",
                                                        dtype=torch.float64, chunk_edges=4096))
    err = rel_l2(strided["res"][0].cpu(), ref)
    print(f"{route}: residual + relu forward (row_strided residual) vs float64 {err:.3e}")
    assert err <= TOL_FWD, err
    # without root / bias: the NULL branches of the same kernels
    _sweep(lambda x, ea: ops.nnconv_forward_raw(x, csr, ea, pm, None, None, "mean", precision=prec), _dev(c, "x", "ea"),
           what=route + " no root/bias")


# ---------------------------------------------------------------------------------------------------------------------------
# keep-Z forward + full backward
# ---------------------------------------------------------------------------------------------------------------------------
def _named_params(c):
    ops_ = {f"W{l}": w for l, w in enumerate(c["Wd"])}
    ops_.update({f"b{l}": b for l, b in enumerate(c["Bd"])})
    return ops_


def _split_params(kw, nl):
    return [kw[f"W{l}"] for l in range(nl)], [kw[f"b{l}"] for l in range(nl)]


def _grad_errs(c, got, aggr="mean"):
    rx, rW, rb, rroot, rbias = nnconv_grads(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], aggr, c["g"], chunk_edges=4096)
    gx, gW, gb, groot, gbias = got
    errs = {"dx": rel_l2(gx.cpu(), rx), "droot": rel_l2(groot.cpu(), rroot), "dbias": rel_l2(gbias.cpu(), rbias)}
    for l in range(len(rW)):
        errs[f"dW{l}"], errs[f"db{l}"] = rel_l2(gW[l].cpu(), rW[l]), rel_l2(gb[l].cpu(), rb[l])
    return errs


@pytest.mark.parametrize("route", ["f16v3_k256", "f16v3_k40"])
def test_keepz_forward_and_full_backward_layouts(route):
    c = _case(route)
    csr, pm, nl = c["csr"], c["pm"], len(c["W"])
    zshape = (c["n"], 64 * ops.hidden_width(c["dims"]))

    def fwd_bwd(x, ea, root, bias, g, **params):
        W, B = _split_params(params, nl)
        z = torch.zeros(zshape, device=D)
        y = ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "mean", z_keep=z)
        r = ops.nnconv_backward_raw(x, csr, ea, W, B, root, "mean", g, z_saved=z)
        r2 = ops.nnconv_backward_raw(x, csr, ea, W, B, root, "mean", g)             # ... and re-aggregating
        return [y, z] + _flat(r) + _flat(r2)

    operands = {**_dev(c, "x", "ea", "root", "bias", "g"), **_named_params(c)}
    base, strided = _sweep(fwd_bwd, operands, expanded={"g": 1.0}, what=route)
    got = strided["g"]
    k = 2 + 3 + 2 * nl                                                             # r2 starts after y, z and r
    r2 = (got[k], got[k + 1:k + 1 + nl], got[k + 1 + nl:k + 1 + 2 * nl], got[k + 1 + 2 * nl], got[k + 2 + 2 * nl])
    errs = _grad_errs(c, r2)
    print(route, "backward (row_strided grad_out) vs float64", {k_: f"{v:.2e}" for k_, v in errs.items()})
    assert all(v <= TOL_BWD for v in errs.values()), errs
    r1 = (got[2], got[3:3 + nl], got[3 + nl:3 + 2 * nl], got[3 + 2 * nl], got[4 + 2 * nl])
    errs = _grad_errs(c, r1)
    assert all(v <= TOL_BWD for v in errs.values()), ("kept Z", errs)
    # the edge-attribute gradient reads the caller's rows through perm
    _sweep(lambda x, ea, g: ops.nnconv_backward_raw(x, csr, ea, c["Wd"], c["Bd"], c["root"].to(D), "mean", g, need_attr=True),
           _dev(c, "x", "ea", "g"), what=route + " need_attr")


# ---------------------------------------------------------------------------------------------------------------------------
# light + deferred backward (depth-shared module)
# ---------------------------------------------------------------------------------------------------------------------------
def test_light_and_deferred_backward_layouts():
    c = _case("f16v3_k256")
    assert ops.deferred_supported(c["dims"])
    csr, nl = c["csr"], 3
    x2, g2 = c["res"].to(D), (c["g"] * 0.5 + c["x"]).to(D)

    def light(x, ea, root, g, **params):
        W, B = _split_params(params, nl)
        return ops.nnconv_backward_light_raw(x, csr, ea, W, B, root, "mean", g)

    def deferred(x, ea, g, **params):
        W, B = _split_params(params, nl)
        return ops.nnconv_backward_deferred_raw([x, x2], [g, g2], csr, ea, W, B, "mean")

    base_l, strided_l = _sweep(light, {**_dev(c, "x", "ea", "root", "g"), **_named_params(c)}, expanded={"g": 1.0}, what="light")
    base_d, strided_d = _sweep(deferred, {**_dev(c, "x", "ea", "g"), **_named_params(c)}, what="deferred")
    # oracle: light gives dx, dW_last, db_last, droot, dbias of one application; deferred the hidden layers' gradients summed over both
    rx, rW, rb, rroot, rbias = nnconv_grads(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], "mean", c["g"])
    gx, gw, gb, groot, gbias = strided_l["x"]
    errs = {"dx": rel_l2(gx.cpu(), rx), "dW_last": rel_l2(gw.cpu(), rW[-1]), "db_last": rel_l2(gb.cpu(), rb[-1]),
            "droot": rel_l2(groot.cpu(), rroot), "dbias": rel_l2(gbias.cpu(), rbias)}
    _, rW2, rb2, _, _ = nnconv_grads(c["res"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], "mean", g2.cpu())
    got = strided_d["x"]
    for l in range(nl - 1):
        errs[f"dW{l}"] = rel_l2(got[l].cpu(), rW[l] + rW2[l])
        errs[f"db{l}"] = rel_l2(got[nl - 1 + l].cpu(), rb[l] + rb2[l])
    print("light + deferred vs float64", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= TOL_BWD for v in errs.values()), errs


# ---------------------------------------------------------------------------------------------------------------------------
# hidden forward -> conv from hidden -> backward from hidden -> hidden backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["f16v3_k256", "f16v6"])
def test_hidden_chain_layouts(route):
    c = _case(route)
    csr, pm, nl, dims = c["csr"], c["pm"], 3, c["dims"]

    def build_h(ea, **params):
        W, B = _split_params(params, nl)
        h, hmax = ops.hidden_forward_raw(csr, ea, pm, W[:-1] + [None], B[:-1] + [None])
        return [h] if hmax is None else [h, hmax]

    hp = {k: v for k, v in _named_params(c).items() if k not in ("W2", "b2")}
    hp.update(W2=None, b2=None)
    base, _ = _sweep(build_h, {"ea": c["ea"].to(D), **hp}, what=route + " hidden_forward")
    hidden, hmax = base[0], (base[1] if len(base) > 1 else None)

    def conv(x, hidden, root, bias, res):
        return [ops.nnconv_forward_hidden_raw(x, csr, hidden, pm, root, bias, "mean", hmax=hmax),
                ops.nnconv_forward_hidden_raw(x, csr, hidden, pm, root, bias, "add", hmax=hmax, residual=res, relu=True)]

    base_c, strided = _sweep(conv, {**_dev(c, "x", "root", "bias", "res"), "hidden": hidden}, what=route + " conv from hidden")
    ref = nnconv_forward(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], aggr="mean", dtype=torch.float64, chunk_edges=4096)
    err = rel_l2(strided["hidden"][0].cpu(), ref)
    print(f"{route}: conv from hidden (row_strided hidden) vs float64 {err:.3e}")
    assert err <= TOL_FWD, err

    def bwd(x, hidden, w_last, b_last, root, g):
        return ops.nnconv_backward_hidden_raw(x, csr, hidden, dims, w_last, b_last, root, "mean", g)

    base_b, strided_b = _sweep(bwd, {**_dev(c, "x", "root", "g"), "hidden": hidden, "w_last": c["Wd"][-1], "b_last": c["Bd"][-1]},
                               expanded={"g": 1.0}, what=route + " backward from hidden")
    grad_h = base_b[1]

    def hbwd(ea, grad_hidden, **params):
        W, B = _split_params({**params, "W2": None, "b2": None}, nl)
        return ops.hidden_backward_raw(csr, ea, dims, W[:-1], B[:-1], grad_hidden)

    hp2 = {k: v for k, v in _named_params(c).items() if k not in ("W2", "b2")}
    base_h, strided_h = _sweep(hbwd, {"ea": c["ea"].to(D), "grad_hidden": grad_h, **hp2}, what=route + " hidden_backward")
    if route == "f16v3_k256":
        rx, rW, rb, rroot, rbias = nnconv_grads(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], "mean", c["g"])
        gx, _, gw, gb, groot, gbias = strided_b["hidden"]
        hW = strided_h["grad_hidden"]
        errs = {"dx": rel_l2(gx.cpu(), rx), "dW2": rel_l2(gw.cpu(), rW[2]), "db2": rel_l2(gb.cpu(), rb[2]), "droot": rel_l2(groot.cpu(), rroot),
                "dbias": rel_l2(gbias.cpu(), rbias), "dW0": rel_l2(hW[0].cpu(), rW[0]), "dW1": rel_l2(hW[1].cpu(), rW[1]),
                "db0": rel_l2(hW[2].cpu(), rb[0]), "db1": rel_l2(hW[3].cpu(), rb[1])}
        print("hidden chain gradients vs float64", {k: f"{v:.2e}" for k, v in errs.items()})
        assert all(v <= TOL_BWD for v in errs.values()), errs


# ---------------------------------------------------------------------------------------------------------------------------
# node-attribute form
# ---------------------------------------------------------------------------------------------------------------------------
def test_node_attribute_layouts():
    c = _case("f16v6")
    n, csr, pm = c["n"], c["csr"], c["pm"]
    g = torch.Generator().manual_seed(77)
    table = torch.randn(n, 2, generator=g).to(D)
    sel = [(0, 0), (1, 0), (1, 1)]

    def fwd(x, table, root, bias):
        return ops.nnconv_forward_nodeattr_raw(x, csr, ops.NodeAttr(table, sel), pm, root, bias, "mean")

    base, strided = _sweep(fwd, {**_dev(c, "x", "root", "bias"), "table": table}, what="node table")
    ei_slots = csr.edge_index.cpu()
    ea = ops.NodeAttr(table, sel).materialize(csr.edge_index).cpu()
    ref = nnconv_forward(c["x"], ei_slots, ea, c["W"], c["B"], c["root"], c["bias"], aggr="mean", dtype=torch.float64, chunk_edges=4096)
    err = rel_l2(strided["table"][0].cpu(), ref)
    print(f"node-attribute forward (row_strided table) vs float64 {err:.3e}")
    assert err <= TOL_FWD, err


# ---------------------------------------------------------------------------------------------------------------------------
# per-edge weights: build, group forward, backward, acc, edge-weights backward
# ---------------------------------------------------------------------------------------------------------------------------
def test_edge_weights_family_layouts():
    c = _case("f16v3_k256")
    csr, pm, dims = c["csr"], c["pm"], c["dims"]
    hidden, _ = ops.hidden_forward_raw(csr, c["ea"].to(D), pm, c["Wd"][:-1] + [None], c["Bd"][:-1] + [None], "f32")

    base, strided = _sweep(lambda hidden, w_last, b_last: ops.edge_weights_raw(hidden, pm, w_last, b_last),
                           {"hidden": hidden, "w_last": c["Wd"][-1], "b_last": c["Bd"][-1]}, what="edge_weights_raw")
    we = base[0]

    def group(x, we, root, bias, res):
        return ops.nnconv_forward_edgeweights_group([
            dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="add"),
            dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="mean", residual=res, relu=True),
            dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="max"),
            dict(x=x, csr=csr, edge_weights=we, root=None, bias=None, aggr="mean")]) + \
            [ops.nnconv_forward_edgeweights_raw(x, csr, we, root, bias, "mean")]

    base_g, strided_g = _sweep(group, {**_dev(c, "x", "root", "bias", "res"), "we": we}, expanded={"bias": 0.25}, what="group forward")
    for aggr, k in (("add", 0), ("max", 2)):
        ref = nnconv_forward(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], aggr=aggr, dtype=torch.float64)
        err = rel_l2(strided_g["we"][k].cpu(), ref)
        print(f"group forward {aggr} (row_strided edge_weights) vs float64 {err:.3e}")
        assert err <= TOL_FWD, (aggr, err)

    def bwd(x, we, root, g):
        first = ops.nnconv_backward_edgeweights_raw(x, csr, we, root, "mean", g)
        acc = tuple(t.clone() for t in first[1:])
        second = ops.nnconv_backward_edgeweights_raw(x, csr, we, root, "mean", g, acc=acc)     # adds in the kernels
        return _flat(first) + _flat(second)

    base_b, strided_b = _sweep(bwd, {**_dev(c, "x", "root", "g"), "we": we}, expanded={"g": 1.0}, what="edge-weights backward + acc")
    gwe = base_b[1]
    assert _bits_equal(base_b[5], gwe + gwe)                     # acc: the second application added to the first (x + x is exact)

    base_e, strided_e = _sweep(lambda grad_we, hidden, w_last: ops.edge_weights_backward_raw(grad_we, hidden, dims, w_last),
                               {"grad_we": gwe, "hidden": hidden, "w_last": c["Wd"][-1]}, what="edge_weights_backward_raw")
    rx, rW, rb, rroot, rbias = nnconv_grads(c["x"], c["ei"], c["ea"], c["W"], c["B"], c["root"], c["bias"], "mean", c["g"])
    gx, _, groot, gbias = strided_b["we"][:4]
    _, gw, gb = strided_e["grad_we"]
    errs = {"dx": rel_l2(gx.cpu(), rx), "droot": rel_l2(groot.cpu(), rroot), "dbias": rel_l2(gbias.cpu(), rbias),
            "dW_last": rel_l2(gw.cpu(), rW[-1]), "db_last": rel_l2(gb.cpu(), rb[-1])}
    print("edge-weights gradients vs float64", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= TOL_BWD for v in errs.values()), errs


# ---------------------------------------------------------------------------------------------------------------------------
# any width: materialised, re-associated, bipartite (offset4 / offset8 reach these kernels: their dword tiling)
# ---------------------------------------------------------------------------------------------------------------------------
def _any_case(cin, cout, n_src=None, k=24):
    n, e = 70, 300
    g = torch.Generator().manual_seed(cin * 1000 + cout + (n_src or 0))
    ns = n if n_src is None else n_src
    ei = _graph(n, e, g, n_src=n_src)
    csr = ops.build_csr(ei.to(D), n, n_src=n_src)
    slots = csr.edge_index.cpu()                         # per-edge tensors of the any-width operators are in CSR slot order
    t = lambda *s: torch.randn(*s, generator=g)
    return dict(n=n, ns=ns, e=e, cin=cin, cout=cout, csr=csr, ei=slots, x=t(ns, cin), xd=t(n, cin + 1 if n_src else cin),
                we=t(e, cin * cout) / cin ** 0.5, root=t(cin + 1 if n_src else cin, cout) / 4, bias=t(cout), res=t(n, cout), g=t(n, cout),
                hidden=torch.relu(t(e, k)), w_last=t(cin * cout, k) / k ** 0.5, b_last=t(cin * cout) / 4)


def _any_oracle(a, aggr, we=None, xd=None, grads=False):
    """float64: out = aggr_e x_src[j] . W_e + x_dst . root + bias, W_e given or hidden . w_last^T + b_last; with `grads` also
    d/d(x, xd, we or (hidden, w_last, b_last), root, bias) of sum(out * g)."""
    f = lambda t: t.double().requires_grad_(grads)
    x, root, bias = f(a["x"]), f(a["root"]), f(a["bias"])
    xdst = x if xd is None else f(xd)
    if we is not None:
        leaves = [f(we)]
        w = leaves[0]
    else:
        leaves = [f(a["hidden"]), f(a["w_last"]), f(a["b_last"])]
        w = leaves[0] @ leaves[1].t() + leaves[2]
    src, dst = a["ei"][0], a["ei"][1]
    m = torch.matmul(x[src].unsqueeze(1), w.view(-1, a["cin"], a["cout"])).squeeze(1)
    n = a["n"]
    if aggr == "max":
        out = torch.full((n, a["cout"]), float("-inf"), dtype=torch.float64).scatter_reduce(0, dst.unsqueeze(1).expand_as(m), m, reduce="amax")
        out = torch.where(torch.bincount(dst, minlength=n).unsqueeze(1) > 0, out, torch.zeros_like(out))
    else:
        out = torch.zeros(n, a["cout"], dtype=torch.float64).index_add(0, dst, m)
        if aggr == "mean":
            out = out / torch.bincount(dst, minlength=n).clamp(min=1).double().unsqueeze(1)
    out = out + xdst @ root + bias
    if not grads:
        return out
    (out * a["g"].double()).sum().backward()
    return out.detach(), dict(x=x.grad, xd=None if xd is None else xdst.grad, root=root.grad, bias=bias.grad, leaves=[t.grad for t in leaves])


@pytest.mark.parametrize("cin,cout", [(8, 12), (5, 7)])       # a vec4 width pair and an odd one (dword tiling at any alignment)
def test_any_width_layouts(cin, cout):
    a = _any_case(cin, cout)
    csr = a["csr"]
    dv = lambda *names: {k: a[k].to(D) for k in names}

    def fwd(x, we, root, bias, res):
        return [ops.nnconv_forward_edgeweights_any_raw(x, csr, we, root, bias, "mean"),
                ops.nnconv_forward_edgeweights_any_raw(x, csr, we, root, bias, "max", residual=res, relu=True),
                ops.nnconv_forward_edgeweights_any_raw(x, csr, we, None, None, "add")]

    vec4 = cout % 4 == 0
    assert ops.any_width_plan(cin, cout, aligned=True)["V"] == (4 if vec4 else 1) and ops.any_width_plan(cin, cout, aligned=False)["V"] == 1
    base, strided = _sweep(fwd, dv("x", "we", "root", "bias", "res"), expanded={"bias": 0.25}, what=f"any {cin}x{cout} forward",
                           retile={"we": (0, 1, 2), "root": (0, 1), "bias": (0, 1), "res": (1,)} if vec4 else None)
    ref = _any_oracle(a, "mean", we=a["we"])
    for key in ["x"] + (["we@offset4"] if vec4 else []):
        err = rel_l2(strided[key][0].cpu(), ref)
        print(f"any-width {cin}x{cout} forward ({key}) vs float64 {err:.3e}")
        assert err <= TOL_FWD, (key, err)

    def bwd(x, we, root, g):
        return ops.nnconv_backward_edgeweights_any_raw(x, csr, we, root, "mean", g)

    base_b, strided_b = _sweep(bwd, dv("x", "we", "root", "g"), expanded={"g": 1.0}, what=f"any {cin}x{cout} backward",
                               retile={"we": (0, 1, 2, 3), "g": (0, 1, 2, 3)} if vec4 else None)
    _, r = _any_oracle(a, "mean", we=a["we"], grads=True)
    for key in ["g"] + (["g@offset4"] if vec4 else []):
        gx, gwe, groot, gbias = strided_b[key]
        errs = {"dx": rel_l2(gx.cpu(), r["x"]), "dwe": rel_l2(gwe.cpu(), r["leaves"][0]), "droot": rel_l2(groot.cpu(), r["root"]),
                "dbias": rel_l2(gbias.cpu(), r["bias"])}
        print(f"any-width {cin}x{cout} gradients ({key}) vs float64", {k: f"{v:.2e}" for k, v in errs.items()})
        assert all(v <= TOL_BWD for v in errs.values()), (key, errs)


@pytest.mark.parametrize("cin,cout", [(8, 12), (5, 7)])
def test_reassociated_any_width_layouts(cin, cout):
    a = _any_case(cin, cout)
    csr = a["csr"]
    dv = lambda *names: {k: a[k].to(D) for k in names}

    def fwd(x, hidden, w_last, b_last, root, bias):
        return ops.nnconv_forward_hidden_any_raw(x, csr, hidden, w_last, b_last, root, bias, "mean")

    base, strided = _sweep(fwd, dv("x", "hidden", "w_last", "b_last", "root", "bias"), expanded={"bias": 0.25}, what="reassoc forward")
    err = rel_l2(strided["hidden"][0].cpu(), _any_oracle(a, "mean"))
    print(f"re-associated {cin}x{cout} forward vs float64 {err:.3e}")
    assert err <= TOL_FWD, err

    def bwd(x, hidden, w_last, b_last, root, g):
        return ops.nnconv_backward_hidden_any_raw(x, csr, hidden, w_last, b_last, root, "mean", g)

    base_b, strided_b = _sweep(bwd, dv("x", "hidden", "w_last", "b_last", "root", "g"), expanded={"g": 1.0}, what="reassoc backward")
    _, r = _any_oracle(a, "mean", grads=True)
    gx, gh, gwl, gbl, groot, gbias = strided_b["g"]
    errs = {"dx": rel_l2(gx.cpu(), r["x"]), "dh": rel_l2(gh.cpu(), r["leaves"][0]), "dw_last": rel_l2(gwl.cpu(), r["leaves"][1]),
            "db_last": rel_l2(gbl.cpu(), r["leaves"][2]), "droot": rel_l2(groot.cpu(), r["root"]), "dbias": rel_l2(gbias.cpu(), r["bias"])}
    print(f"re-associated {cin}x{cout} gradients vs float64", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= TOL_BWD for v in errs.values()), errs


@pytest.mark.parametrize("flip", [False, True])
def test_bipartite_layouts(flip):
    cin, cout, n_src = 8, 12, 45
    a = _any_case(cin, cout, n_src=n_src)
    if flip:                       # flow='target_to_source': the same graph from edge_index with its rows swapped
        ei_d = a["ei"].flip(0).contiguous().to(D)
        a["csr"] = ops.build_csr(ei_d, a["n"], n_src=n_src, flip=True)
        assert torch.equal(a["csr"].edge_index.cpu(), a["ei"])          # (slot order is stable: the per-edge rows stay valid)
    csr = a["csr"]
    dv = lambda *names: {k: a[k].to(D) for k in names}

    def fwd(x, xd, we, hidden, w_last, b_last, root, bias, res):
        return [ops.nnconv_forward_edgeweights_bip_raw(x, xd, csr, we, root, bias, "mean", residual=res, relu=False),
                ops.nnconv_forward_edgeweights_bip_raw(x, None, csr, we, None, bias, "max"),
                ops.nnconv_forward_hidden_bip_raw(x, xd, csr, hidden, w_last, b_last, root, bias, "add")]

    base, strided = _sweep(fwd, dv("x", "xd", "we", "hidden", "w_last", "b_last", "root", "bias", "res"), what="bipartite forward",
                           retile={"we": (0, 1), "root": (0,), "bias": (0, 1), "res": (0,)})
    err = rel_l2(strided["xd"][0].cpu(), _any_oracle(a, "mean", we=a["we"], xd=a["xd"]) + a["res"].double())
    err2 = rel_l2(strided["xd"][2].cpu(), _any_oracle(a, "add", xd=a["xd"]))
    print(f"bipartite forward vs float64: per-edge weights {err:.3e}, re-associated {err2:.3e}")
    assert err <= TOL_FWD and err2 <= TOL_FWD, (err, err2)

    def bwd(x, xd, we, hidden, w_last, b_last, root, g):
        return _flat(ops.nnconv_backward_edgeweights_bip_raw(x, xd, csr, we, root, "mean", g)) + \
            _flat(ops.nnconv_backward_hidden_bip_raw(x, xd, csr, hidden, w_last, b_last, root, "mean", g))

    base_b, strided_b = _sweep(bwd, dv("x", "xd", "we", "hidden", "w_last", "b_last", "root", "g"), expanded={"g": 1.0},
                               what="bipartite backward", retile={"we": (0, 1, 2, 3, 4), "g": (0, 1, 2, 3, 4)})
    _, r = _any_oracle(a, "mean", we=a["we"], xd=a["xd"], grads=True)
    gxs, gxd, gwe, groot, gbias = strided_b["g"][:5]
    errs = {"dx_src": rel_l2(gxs.cpu(), r["x"]), "dx_dst": rel_l2(gxd.cpu(), r["xd"]), "dwe": rel_l2(gwe.cpu(), r["leaves"][0]),
            "droot": rel_l2(groot.cpu(), r["root"]), "dbias": rel_l2(gbias.cpu(), r["bias"])}
    _, r = _any_oracle(a, "mean", xd=a["xd"], grads=True)
    gxs, gxd, gh, gwl, gbl, groot, gbias = strided_b["g"][5:]
    errs.update({"h:dx_src": rel_l2(gxs.cpu(), r["x"]), "h:dx_dst": rel_l2(gxd.cpu(), r["xd"]), "h:dh": rel_l2(gh.cpu(), r["leaves"][0]),
                 "h:dw_last": rel_l2(gwl.cpu(), r["leaves"][1]), "h:db_last": rel_l2(gbl.cpu(), r["leaves"][2]),
                 "h:droot": rel_l2(groot.cpu(), r["root"])})
    print("bipartite gradients vs float64", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= TOL_BWD for v in errs.values()), errs


def test_gather_rows_layouts():
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(300, 6, generator=g).to(D)
    perm = torch.randperm(300, generator=g).to(torch.int32).to(D)
    base, _ = _sweep(lambda rows: ops.gather_rows(rows, perm), {"rows": rows}, what="gather_rows")
    assert torch.equal(base[0], rows[perm.long()])
    big = torch.zeros(600, dtype=torch.int32, device=D)
    big[::2] = perm
    assert torch.equal(ops.gather_rows(rows, big[::2]), base[0])          # a strided permutation


# ---------------------------------------------------------------------------------------------------------------------------
# written operands
# ---------------------------------------------------------------------------------------------------------------------------
def _awkward(shape):
    kinds = ("row_strided", "row_skipping", "offset4", "offset8") + (("transposed_storage",) if len(shape) == 2 else ())
    for kind in kinds:
        view, backing = as_layout(sentinel_like(shape, D), kind)
        yield kind, view, backing


def test_caller_given_out_z_keep_and_acc():
    c = _case("f16v3_k256")
    csr, pm, n, e = c["csr"], c["pm"], c["n"], c["e"]
    x, ea, root, bias, g = (c[k].to(D) for k in ("x", "ea", "root", "bias", "g"))
    hidden, hmax = ops.hidden_forward_raw(csr, ea, pm, c["Wd"][:-1] + [None], c["Bd"][:-1] + [None])
    h32, _ = ops.hidden_forward_raw(csr, ea, pm, c["Wd"][:-1] + [None], c["Bd"][:-1] + [None], "f32")
    we = ops.edge_weights_raw(h32, pm, c["Wd"][-1], c["Bd"][-1])
    na = ops.NodeAttr(torch.randn(n, 3, device=D), [(0, 0), (1, 1), (0, 2)])
    zshape = (n, 64 * ops.hidden_width(c["dims"]))
    forwards = {
        "nnconv_forward_raw": lambda **k: ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "mean", **k),
        "nnconv_forward_hidden_raw": lambda **k: ops.nnconv_forward_hidden_raw(x, csr, hidden, pm, root, bias, "mean", hmax=hmax, **k),
        "nnconv_forward_mixed_raw": lambda **k: ops.nnconv_forward_mixed_raw(x, csr, ea, None, None, 0, pm, root, bias, "mean", **k),
        "nnconv_forward_nodeattr_raw": lambda **k: ops.nnconv_forward_nodeattr_raw(x, csr, na, pm, root, bias, "mean", **k),
        "nnconv_forward_edgeweights_raw": lambda **k: ops.nnconv_forward_edgeweights_raw(x, csr, we, root, bias, "mean", **k),
        "nnconv_forward_edgeweights_group": lambda **k: ops.nnconv_forward_edgeweights_group(
            [dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="add"),
             dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr="mean", **k)])[1],
    }
    for name, fwd in forwards.items():
        own = fwd()
        out, backing = carve_out((n, 64), D)
        got = fwd(out=out)
        torch.cuda.synchronize()
        assert got is out and _bits_equal(out, own), name        # filled with the bits of the allocate-it-yourself call
        guards_intact(backing, value=False)
        calls = _lib.n_native_calls
        for kind, view, b in _awkward((n, 64)):
            with pytest.raises(ValueError, match="out"):
                fwd(out=view)
            torch.cuda.synchronize()
            assert all_sentinel(b.buf), (name, kind)              # nothing was written anywhere
        for bad in (torch.zeros(n, 64, dtype=torch.float64, device=D), torch.zeros(n + 1, 64, device=D), torch.zeros(n, 64)):
            with pytest.raises(ValueError, match="out"):
                fwd(out=bad)
        assert _lib.n_native_calls == calls, name
    for name in ("nnconv_forward_raw", "nnconv_forward_hidden_raw", "nnconv_forward_mixed_raw"):
        fwd = forwards[name]
        z_own = torch.zeros(zshape, device=D)
        y_own = fwd(z_keep=z_own)
        z, backing = carve_out(zshape, D)
        z.zero_()
        y = fwd(z_keep=z)
        torch.cuda.synchronize()
        assert _bits_equal(y, y_own) and _bits_equal(z, z_own), name
        guards_intact(backing, value=False)
        for kind, view, b in _awkward(zshape):
            with pytest.raises(ValueError, match="z_keep"):
                fwd(z_keep=view)
            assert all_sentinel(b.buf), (name, kind)
    # acc of the edge-weights backward
    first = ops.nnconv_backward_edgeweights_raw(x, csr, we, root, "mean", g)
    own = ops.nnconv_backward_edgeweights_raw(x, csr, we, root, "mean", g, acc=tuple(t.clone() for t in first[1:]))
    carved = [carve_out(t.shape, D) for t in first[1:]]
    for (v, _), t in zip(carved, first[1:]):
        v.copy_(t)
    got = ops.nnconv_backward_edgeweights_raw(x, csr, we, root, "mean", g, acc=tuple(v for v, _ in carved))
    torch.cuda.synchronize()
    assert all(_bits_equal(a, b) for a, b in zip(got, own))
    for _, backing in carved:
        guards_intact(backing, value=False)
    for i, t in enumerate(first[1:]):
        for kind, view, b in _awkward(tuple(t.shape)):
            acc = [u.clone() for u in first[1:]]
            acc[i] = view
            with pytest.raises(ValueError, match="acc"):
                ops.nnconv_backward_edgeweights_raw(x, csr, we, root, "mean", g, acc=tuple(acc))
            assert all_sentinel(b.buf), (i, kind)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16])
def test_wrong_dtypes_never_reach_the_library(dtype):
    c = _case("f16v3_k256")
    csr, pm, n = c["csr"], c["pm"], c["n"]
    good = dict(x=c["x"].to(D), root=c["root"].to(D), bias=c["bias"].to(D), residual=c["res"].to(D), out=torch.zeros(n, 64, device=D))
    ea, g = c["ea"].to(D), c["g"].to(D)
    hidden, hmax = ops.hidden_forward_raw(csr, ea, pm, c["Wd"][:-1] + [None], c["Bd"][:-1] + [None])
    we = torch.zeros(c["e"], 4096, device=D)
    na = ops.NodeAttr(torch.randn(n, 3, device=D), [(0, 0), (1, 1), (0, 2)])
    calls = _lib.n_native_calls
    for operand in good:
        k = {**good, operand: good[operand].to(dtype)}
        wrappers = {
            "forward": lambda: ops.nnconv_forward_raw(k["x"], csr, ea, pm, k["root"], k["bias"], "mean", out=k["out"], residual=k["residual"]),
            "hidden": lambda: ops.nnconv_forward_hidden_raw(k["x"], csr, hidden, pm, k["root"], k["bias"], "mean", hmax=hmax, out=k["out"],
                                                            residual=k["residual"]),
            "edgeweights": lambda: ops.nnconv_forward_edgeweights_raw(k["x"], csr, we, k["root"], k["bias"], "mean", residual=k["residual"],
                                                                      out=k["out"]),
        }
        if operand != "residual":
            wrappers["mixed"] = lambda: ops.nnconv_forward_mixed_raw(k["x"], csr, ea, None, None, 0, pm, k["root"], k["bias"], "mean", out=k["out"])
            wrappers["nodeattr"] = lambda: ops.nnconv_forward_nodeattr_raw(k["x"], csr, na, pm, k["root"], k["bias"], "mean", out=k["out"])
        if operand in ("x", "root"):
            wrappers["backward"] = lambda: ops.nnconv_backward_raw(k["x"], csr, ea, c["Wd"], c["Bd"], k["root"], "mean", g)
            wrappers["light"] = lambda: ops.nnconv_backward_light_raw(k["x"], csr, ea, c["Wd"], c["Bd"], k["root"], "mean", g)
            wrappers["hidden backward"] = lambda: ops.nnconv_backward_hidden_raw(k["x"], csr, hidden, c["dims"], c["Wd"][-1], c["Bd"][-1],
                                                                                 k["root"], "mean", g)
            wrappers["edgeweights backward"] = lambda: ops.nnconv_backward_edgeweights_raw(k["x"], csr, we, k["root"], "mean", g)
        for name, call in wrappers.items():
            # (nnconv_forward_raw has always answered a wrong x dtype with NotImplementedError, the other wrappers with ValueError)
            want = NotImplementedError if (name, operand) == ("forward", "x") else ValueError
            with pytest.raises(want):
                call()
    assert _lib.n_native_calls == calls


# ---------------------------------------------------------------------------------------------------------------------------
# module surface: views as inputs and as parameters, twice (the second call hits the caches built from views)
# ---------------------------------------------------------------------------------------------------------------------------
def _seq(dims, act=torch.nn.ReLU):
    return torch.nn.Sequential(*sum([[torch.nn.Linear(dims[i], dims[i + 1]), act()] for i in range(len(dims) - 1)], [])[:-1])


MODULES = {
    "direct": dict(n=70, e=300, cin=64, cout=64, nn=lambda: _seq([3, 256, 256, 4096]), aggr="mean"),
    "direct_slot_order": dict(n=320, e=33000, cin=64, cout=64, nn=lambda: _seq([3, 256, 256, 4096]), aggr="mean"),
    "max": dict(n=70, e=300, cin=64, cout=64, nn=lambda: _seq([3, 32, 4096]), aggr="max"),
    "general_nn": dict(n=70, e=300, cin=64, cout=64, nn=lambda: _seq([3, 32, 4096], act=torch.nn.Tanh), aggr="mean"),
    # (out_channels 7: the any-width kernels run their dword tiling at every alignment - at a multiple of 4 the offset4 root / bias
    # would move the call from V = 4 to V = 1, the same sums in another order; test_any_width_layouts covers that pair)
    "any_width": dict(n=70, e=300, cin=8, cout=7, nn=lambda: _seq([3, 24, 56]), aggr="add"),
    "bipartite": dict(n=70, e=300, cin=(8, 9), cout=7, nn=lambda: _seq([3, 24, 56]), aggr="mean", n_src=45),
}


def _repoint(conv):
    """Every parameter of the module as an offset4 view of one flat buffer (p.data = flat[o : o + k].view_as(p))."""
    ps = list(conv.parameters())
    total = sum((p.numel() + 3) // 4 * 4 for p in ps) + 8
    raw = torch.zeros(total + 4, device=D)
    lead = (-(raw.data_ptr() // 4)) % 4
    flat, o = raw[lead:], 1
    for p in ps:
        view = flat[o:o + p.numel()].view_as(p)
        view.copy_(p.data)
        p.data = view
        assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        o += (p.numel() + 3) // 4 * 4
    ops.clear_caches()
    return flat


@pytest.mark.parametrize("name", sorted(MODULES))
def test_module_surface_with_views(name):
    m = MODULES[name]
    n, e, n_src = m["n"], m["e"], m.get("n_src")
    g = torch.Generator().manual_seed(99)
    ei = _graph(n, e, g, n_src=n_src).to(D)
    ea = torch.randn(e, 3, generator=g).to(D)
    cin_src = m["cin"][0] if isinstance(m["cin"], tuple) else m["cin"]
    x = torch.randn(n_src or n, cin_src, generator=g).to(D)
    xd = torch.randn(n, m["cin"][1], generator=g).to(D) if n_src else None
    gout = torch.randn(n, m["cout"], generator=g).to(D)
    torch.manual_seed(3)
    conv = gp.NNConv_old(m["cin"], m["cout"], m["nn"](), aggr=m["aggr"]).to(D)
    twin = gp.NNConv_old(m["cin"], m["cout"], m["nn"](), aggr=m["aggr"]).to(D)
    twin.load_state_dict(conv.state_dict())

    def run(model, x_leaf, ea_in):
        outs = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            x_leaf.grad = None
            y = model((x_leaf, xd), ei, ea_in, size=(n_src, n)) if n_src else model(x_leaf, ei, ea_in)
            (y * gout).sum().backward()
            outs.append((y.detach().clone(), x_leaf.grad.detach().clone(), [p.grad.detach().contiguous().clone() for p in model.parameters()]))
        torch.cuda.synchronize()
        return outs

    ops.clear_caches()
    x_dense = x.clone().requires_grad_(True)
    want = run(twin, x_dense, ea.clone())
    # (the second call may take another route than the first - the hidden activations / per-edge weights the first one cached -
    # so call k of the model on views is compared with call k of the dense model)

    flat = _repoint(conv)
    xv, xb = as_layout(x, "row_strided")
    x_view = xv.requires_grad_(True)
    assert not x_view.is_contiguous() and x_view.is_leaf
    eav, eab = as_layout(ea, "row_strided")
    calls = _lib.n_native_calls
    got = run(conv, x_view, eav)
    assert _lib.n_native_calls > calls
    for k, (w, h) in enumerate(zip(want, got)):
        assert _bits_equal(w[0], h[0]), (name, k, "output")
        assert _bits_equal(w[1], h[1]), (name, k, "x.grad")
        for i, (a, b) in enumerate(zip(w[2], h[2])):
            assert _bits_equal(a, b), (name, k, "parameter gradient", i)
    guards_intact(xb)
    guards_intact(eab)
    for p, q in zip(conv.parameters(), twin.parameters()):
        assert _bits_equal(p.data, q.data)                        # the parameters themselves were only read
    del flat
    ops.clear_caches()


# the routes the module reaches only through the policy of hidden_cache: asserted from the deltas of hidden_cache.stats
CACHED = {
    # 33,000 edges on 320 nodes: above hidden_cache.WE_SMALL_EDGES and mean in-degree > 4 - the shared hidden activations
    "shared_h": dict(n=320, e=33000, we=False),
    # 300 edges: the per-edge weights W_e as a shared autograd node (training) and as the inference cache
    "we_cache": dict(n=70, e=300, we=True),
}


@pytest.mark.parametrize("name", sorted(CACHED))
def test_module_cached_routes_with_views(name):
    """A module applied three times per forward (the depth loop of the reference scripts) for two training steps, then four
    inference calls: the applications after the first are served from the hidden activations / per-edge weights that an earlier one
    built FROM VIEWS (cache keys carry the view's strides and storage offset).  Same bits as the dense model, call by call, and the
    same sequence of cache builds and hits."""
    from graph_pde_amd import hidden_cache
    assert hidden_cache.MODE == "auto" and hidden_cache.WE_MODE == "auto"
    m = CACHED[name]
    n, e = m["n"], m["e"]
    g = torch.Generator().manual_seed(7)
    ei = _graph(n, e, g).to(D)
    ea = torch.randn(e, 3, generator=g).to(D)
    x = torch.randn(n, 64, generator=g).to(D)
    gout = torch.randn(n, 64, generator=g).to(D)
    torch.manual_seed(5)
    conv = gp.NNConv_old(64, 64, _seq([3, 256, 256, 4096]), aggr="mean").to(D)
    twin = gp.NNConv_old(64, 64, _seq([3, 256, 256, 4096]), aggr="mean").to(D)
    twin.load_state_dict(conv.state_dict())

    def delta(before):
        return {k: hidden_cache.stats.get(k, 0) - before.get(k, 0) for k in ("hits", "builds", "direct", "we_hits", "we_builds")}

    def run(model, x_leaf, ea_in):
        ops.clear_caches()
        hidden_cache.clear()
        outs, s0 = [], dict(hidden_cache.stats)
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            x_leaf.grad = None
            y = x_leaf
            for _depth in range(3):
                y = torch.tanh(model(y, ei, ea_in))
            (y * gout).sum().backward()
            outs.append([y.detach().clone(), x_leaf.grad.detach().clone()] + [p.grad.detach().contiguous().clone() for p in model.parameters()])
        train = delta(s0)
        s1 = dict(hidden_cache.stats)
        with torch.no_grad():
            for _ in range(4):
                outs.append([model(x_leaf.detach(), ei, ea_in).clone()])
        torch.cuda.synchronize()
        return outs, train, delta(s1)

    want, train_d, infer_d = run(twin, x.clone().requires_grad_(True), ea.clone())
    flat = _repoint(conv)
    xv, xb = as_layout(x, "row_strided")
    eav, eab = as_layout(ea, "row_strided")
    got, train_v, infer_v = run(conv, xv.requires_grad_(True), eav)
    print(name, "training", train_v, "inference", infer_v)
    # the routes were taken - by the model on views exactly as by the dense one
    assert train_v == train_d and infer_v == infer_d, (train_d, train_v, infer_d, infer_v)
    assert train_v["builds"] >= 1 and train_v["hits"] >= 1, train_v           # applications 2.. read the H an earlier one built
    assert infer_v["hits"] + infer_v["we_hits"] >= 1, infer_v
    if m["we"]:
        assert train_v["we_builds"] >= 1 and train_v["we_hits"] >= 1, train_v
        assert infer_v["we_builds"] >= 1 and infer_v["we_hits"] >= 1, infer_v  # the inference W_e cache, keyed on the edge_attr view
    else:
        assert train_v["we_builds"] == train_v["we_hits"] == infer_v["we_builds"] == infer_v["we_hits"] == 0, (train_v, infer_v)
    for k, (w, h) in enumerate(zip(want, got)):
        for i, (a, b) in enumerate(zip(w, h)):
            assert _bits_equal(a, b), (name, "call", k, "tensor", i)
    guards_intact(xb)
    guards_intact(eab)
    del flat
    ops.clear_caches()
    hidden_cache.clear()
