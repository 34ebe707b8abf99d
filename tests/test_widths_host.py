"""CPU tier: NNConv at widths other than 64 -> 64 - everything that can be checked without a GPU.

* the float64 oracle against RECTANGULAR vectors of the reference's own NNConv_old + DenseNet
  (tests/golden/make_golden_widths.py -> nnconv_rect_*.npz): at 64 x 64 a transposed `view(-1, out, in)` would pass, here not;
* the any-width entry points: declared in include/gpde.h, bound by _lib.SIGNATURES, exported by libgpde.so;
* the supported range (ops.width_supported), the module's refusal above it, rectangular `lin.weight` state dicts."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from oracle.nnconv_oracle import nnconv_forward, nnconv_grads, rel_l2
from tests.conftest import GOLDEN, REPO, load_golden
from tests.helpers import any_tilings as at
from tests.test_oracle_golden import load_golden_grads

RECT_CASES = {"nnconv_rect_24x40_mean": (24, 40), "nnconv_rect_40x24_add": (40, 24), "nnconv_rect_1x8_mean": (1, 8)}
ANY_ENTRY_POINTS = ["gpde_nnconv_fwd_edgeweights_any", "gpde_nnconv_bwd_edgeweights_any_workspace_bytes", "gpde_nnconv_bwd_edgeweights_any",
                    "gpde_nnconv_edgeweights_any_plan"]


@pytest.mark.parametrize("name", sorted(RECT_CASES))
def test_oracle_matches_the_reference_at_rectangular_widths(name):
    """Forward in float32 and float64 and every float64 gradient, at the tolerances tests/test_oracle_golden.py holds the 64 x 64
    fixtures to (2e-7 / 1e-13 / 1e-12)."""
    cin, cout = RECT_CASES[name]
    g, r = load_golden(name), load_golden_grads(name)
    assert g["out_f64"].shape == (g["x"].shape[0], cout) and g["weights"][-1].shape[0] == cin * cout
    assert (g["x"].dim() == 1) == (name == "nnconv_rect_1x8_mean")
    args = (g["x"], g["edge_index"], g["edge_attr"], g["weights"], g["biases"], g["root"], g["bias"])
    y32 = nnconv_forward(*args, aggr=g["aggr"], dtype=torch.float32)
    assert rel_l2(y32, g["out_f32"]) <= 2e-7, rel_l2(y32, g["out_f32"])
    y64 = nnconv_forward(*args, aggr=g["aggr"], dtype=torch.float64)
    assert rel_l2(y64, g["out_f64"]) <= 1e-13, rel_l2(y64, g["out_f64"])
    x2 = g["x"].unsqueeze(-1) if g["x"].dim() == 1 else g["x"]
    gx, gW, gb, groot, gbias = nnconv_grads(x2, *args[1:], g["aggr"], r["gout"])
    tol = 1e-12
    assert rel_l2(gx.reshape(r["gx"].shape), r["gx"]) <= tol
    for l in range(len(gW)):
        assert rel_l2(gW[l], r["gW"][l]) <= tol and rel_l2(gb[l], r["gb"][l]) <= tol, l
    assert (groot is None) == (r["groot"] is None) and (gbias is None) == (r["gbias"] is None)
    if groot is not None:
        assert rel_l2(groot, r["groot"]) <= tol
    if gbias is not None:
        assert rel_l2(gbias, r["gbias"]) <= tol


def test_a_transposed_weight_view_fails_the_rectangular_fixture():
    """What the rectangular fixtures are for: view(-1, out, in).transpose would pass at 64 x 64 shapes-wise; here it is wrong."""
    g = load_golden("nnconv_rect_24x40_mean")
    x, ei = g["x"].double(), g["edge_index"]
    h = g["edge_attr"].double()
    for l, (w, b) in enumerate(zip(g["weights"], g["biases"])):
        h = torch.nn.functional.linear(h, w.double(), b.double())
        if l != len(g["weights"]) - 1:
            h = torch.relu(h)
    wrong = h.view(-1, 40, 24).transpose(1, 2)
    m = torch.matmul(x[ei[0]].unsqueeze(1), wrong).squeeze(1)
    out = torch.zeros(x.shape[0], 40, dtype=torch.float64).index_add_(0, ei[1], m)
    out = out / torch.bincount(ei[1], minlength=x.shape[0]).clamp(min=1).double().unsqueeze(1)
    out = out + x @ g["root"].double() + g["bias"].double()
    assert rel_l2(out, g["out_f64"]) > 0.1


def test_fixtures_are_small():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("nnconv_rect_"))
    assert total < (1 << 20), total


def test_any_width_entry_points_are_declared_bound_and_exported():
    protos = _lib.header_prototypes()
    for name in ANY_ENTRY_POINTS:
        assert name in protos, f"{name} is not declared in include/gpde.h"
        assert name in _lib.SIGNATURES, name
    ret, args = protos["gpde_nnconv_fwd_edgeweights_any"]
    assert ret == "int" and len(args) == 15 and args.count("int") == 4              # relu, aggr, in_channels, out_channels
    ret, args = protos["gpde_nnconv_bwd_edgeweights_any_workspace_bytes"]
    assert ret == "size_t" and args == ["int64_t", "int64_t", "int", "int"]
    ret, args = protos["gpde_nnconv_bwd_edgeweights_any"]
    assert ret == "int" and len(args) == 20 and args.count("int") == 3               # aggr, in_channels, out_channels
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(ANY_ENTRY_POINTS) <= syms, sorted(set(ANY_ENTRY_POINTS) - syms)
    src = open(os.path.join(REPO, "include", "gpde.h")).read()
    assert int(re.search(r"#define GPDE_WECONV_ANY_MAX_WIDTH (\d+)", src).group(1)) == _lib.GPDE_WECONV_ANY_MAX_WIDTH == ops.ANY_MAX_WIDTH == 256


def test_workspace_query_and_host_side_validation_need_no_device():
    """The workspace query is host arithmetic; argument checks come before any launch (zero nodes: a valid call, nothing runs)."""
    l = _lib.lib()
    q = l.gpde_nnconv_bwd_edgeweights_any_workspace_bytes
    assert q(10, 30, 24, 40) >= 30 * 24 * 4 + (24 * 40 + 40) * 4
    assert q(0, 0, 1, 1) > 0
    assert q(10, 30, 0, 40) == 0 and q(10, 30, 24, 257) == 0 and q(-1, 30, 24, 40) == 0
    assert q(1 << 20, 1 << 22, 256, 256) >= (1 << 22) * 256 * 4                       # size_t arithmetic: 4 GiB of per-edge rows
    rowptr = (np.zeros(1, dtype=np.int32)).ctypes.data
    fwd = l.gpde_nnconv_fwd_edgeweights_any
    assert fwd(None, 0, None, 0, rowptr, None, None, None, None, 0, _lib.GPDE_AGGR_MEAN, 24, 40, None, None) == _lib.GPDE_OK
    assert fwd(None, 0, None, 0, None, None, None, None, None, 0, _lib.GPDE_AGGR_MEAN, 24, 40, None, None) == -1      # GPDE_EINVAL: no rowptr
    assert fwd(None, -1, None, 0, rowptr, None, None, None, None, 0, _lib.GPDE_AGGR_MEAN, 24, 40, None, None) == -1
    assert fwd(None, 0, None, 0, rowptr, None, None, None, None, 0, 7, 24, 40, None, None) == -1                       # unknown aggr
    for cin, cout in ((0, 8), (8, 0), (257, 8), (8, 257)):
        assert fwd(None, 0, None, 0, rowptr, None, None, None, None, 0, _lib.GPDE_AGGR_ADD, cin, cout, None, None) == -2   # GPDE_EUNSUPPORTED
        assert "256" in l.gpde_last_error().decode()
    bwd = l.gpde_nnconv_bwd_edgeweights_any
    ws = (np.zeros(4096, dtype=np.uint8)).ctypes.data
    ok = (None, 0, None, 0, rowptr, None, None, None, None)
    assert bwd(*ok, _lib.GPDE_AGGR_ADD, 24, 40, None, None, None, None, None, ws, 4096, None) == -3                    # GPDE_EWORKSPACE
    big = int(q(0, 0, 24, 40))
    wsb = (np.zeros(big + 256, dtype=np.uint8)).ctypes.data
    assert bwd(*ok, _lib.GPDE_AGGR_MAX, 24, 40, None, None, None, None, None, wsb, big, None) == -2
    assert "max" in l.gpde_last_error().decode().lower()
    assert bwd(*ok, _lib.GPDE_AGGR_ADD, 300, 40, None, None, None, None, None, wsb, big, None) == -2
    assert "256" in l.gpde_last_error().decode()
    assert bwd(*ok, _lib.GPDE_AGGR_ADD, 24, 40, None, None, None, None, None, None, big, None) == -1                    # no workspace
    assert bwd(*ok, _lib.GPDE_AGGR_ADD, 24, 40, None, None, None, None, None, wsb, big, None) == _lib.GPDE_OK           # zero nodes


def test_supported_range_predicate():
    assert ops.width_supported(64, 64) and ops.width_supported(1, 1) and ops.width_supported(256, 256)
    assert ops.width_supported(3, 5) and ops.width_supported(128, 32)
    assert not ops.width_supported(0, 64) and not ops.width_supported(64, 0)
    assert not ops.width_supported(257, 64) and not ops.width_supported(64, 257) and not ops.width_supported(-3, 8)
    assert not ops.width_supported(2.5, 8) and not ops.width_supported(None, 8)


def test_a_257_wide_module_still_raises_and_names_the_limit():
    """The refusal comes before anything touches a device: it needs none."""
    for cin, cout in ((257, 64), (64, 257), (300, 300)):
        conv = gp.NNConv_old(cin, cout, torch.nn.Linear(3, cin * cout), aggr="mean")
        assert tuple(conv.root.shape) == (cin, cout)
        x = torch.randn(4, cin)
        ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
        ea = torch.randn(3, 3)
        for call in (lambda: conv(x, ei, ea), lambda: conv.propagate(ei, x=x, pseudo=ea), lambda: conv.message(x[ei[0]], ea),
                     lambda: conv.update(torch.zeros(4, cout), x), lambda: conv(x, ei, ea, activation="relu"),
                     lambda: gp.nnconv_group([(conv, x, ei, ea)])):
            with pytest.raises(NotImplementedError, match="256"):
                call()
    # inside the range the width check passes (what follows needs the device)
    gp.NNConv_old(24, 40, torch.nn.Linear(3, 960))._check_width()
    gp.NNConv(1, 1, torch.nn.Linear(3, 1))._check_width()
    gp.NNConv_old(64, 64, torch.nn.Linear(3, 4096))._check_width()


def test_a_rectangular_lin_weight_state_dict_loads_transposed():
    conv = gp.NNConv_old(24, 40, torch.nn.Linear(3, 960), aggr="add")
    sd = conv.state_dict()
    w = torch.randn(40, 24)
    sd_new = {k: v for k, v in sd.items() if k != "root"}
    sd_new["lin.weight"] = w
    conv.load_state_dict(sd_new)
    assert tuple(conv.root.shape) == (24, 40) and torch.equal(conv.root.detach(), w.t())
    assert repr(conv) == "NNConv_old(24, 40)"
    # the module's own format round-trips
    conv2 = gp.NNConv_old(24, 40, torch.nn.Linear(3, 960), aggr="add")
    conv2.load_state_dict(conv.state_dict())
    assert torch.equal(conv2.root.detach(), conv.root.detach())


# ---- the lane tiling of csrc/gpde_weconv_any.hip, through its host query (ops.any_width_plan) -----------------------------------
ANY_XS = 1024        # floats of LDS per wave (gpde_weconv_any.hip)


def test_plan_query_is_declared_with_its_signature():
    ret, args = _lib.header_prototypes()["gpde_nnconv_edgeweights_any_plan"]
    assert ret == "int" and args == ["int", "int", "int", "int", "int32_t*"]


@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
@pytest.mark.parametrize("aligned", [True, False])
def test_every_tiling_fits_the_wave_the_columns_and_the_lds(aligned, aggr):
    """All 256 x 256 widths: the lanes in use fit the wave, 4 column steps of LC lanes cover a row, LC is a power of two (the
    backward's xor shuffles), a pass of x_j rows fits the LDS array, 'max' keeps whole columns in a lane."""
    for cin in range(1, 257):
        for cout in range(1, 257):
            p = ops.any_width_plan(cin, cout, aligned=aligned, aggr=aggr)
            what = (cin, cout, aligned, aggr, p)
            assert p["V"] == (4 if aligned and cout % 4 == 0 else 1), what
            assert min(p.values()) >= 1 and p["lanes"] == p["LC"] * p["R"] * p["ES"] <= 64, what
            assert 4 * p["LC"] >= -(-cout // p["V"]) and (p["V"] == 1 or p["LC"] >= cout // 4), what   # V = 4: one access per lane
            assert p["LC"] & (p["LC"] - 1) == 0, what
            assert p["R"] <= cin, what
            if aggr == "max":
                assert p["R"] == 1, what
            else:
                assert p["B"] in (4, 8) and p["B"] * p["ES"] * cin <= ANY_XS, what
    assert ops.any_width_plan(24, 40, aggr="mean") == ops.any_width_plan(24, 40, aggr="add")


def test_plan_query_rejects_what_the_launchers_reject():
    l = _lib.lib()
    out = (np.zeros(6, dtype=np.int32)).ctypes.data
    for cin, cout in ((0, 8), (8, 0), (257, 8), (8, 257), (-1, 8)):
        assert l.gpde_nnconv_edgeweights_any_plan(cin, cout, 1, _lib.GPDE_AGGR_ADD, out) == -2                      # GPDE_EUNSUPPORTED
        assert "256" in l.gpde_last_error().decode()
        with pytest.raises(NotImplementedError, match="256"):
            ops.any_width_plan(cin, cout)
    assert l.gpde_nnconv_edgeweights_any_plan(8, 8, 1, 7, out) == -1 and l.gpde_nnconv_edgeweights_any_plan(8, 8, 1, 0, None) == -1
    with pytest.raises(NotImplementedError):
        ops.any_width_plan(8, 8, aggr="min")
    assert l.gpde_nnconv_edgeweights_any_plan(256, 256, 1, _lib.GPDE_AGGR_ADD, out) == _lib.GPDE_OK


def test_the_tiling_classes_number_128():
    """What tests/test_gpu_width_tilings.py parametrises over.  Another count: the classifier (tests/helpers/any_tilings.py) or
    the plan changed - either way the GPU tier's cases have to be looked at again."""
    cl = at.classes("add")
    assert len(cl) == at.N_CLASSES == 128, len(cl)
    assert sum(len(v) for v in cl.values()) == 256 * 256
    assert at.classes("mean") == cl
    reps = at.representatives()
    assert len({nm for nm, *_ in reps}) == 128                                       # the names tell the classes apart
    for nm, k, cin, cout in reps:
        assert at.tiling_class(cin, cout, ops.any_width_plan(cin, cout)) == k
    # the `k >= 1` arm of row_load<1> / row_store<1>: a class of its own for every number of column steps
    assert {k[5] for k in cl if k[0] == 1} == {1, 2, 3, 4} and {k[5] for k in cl if k[0] == 4} == {1}
    assert len(at.max_representatives()) == len({(p["V"], p["LC"], p["ES"]) for p in (
        ops.any_width_plan(1, co, aggr="max") for co in range(1, 257))})


def test_ladder_graph_has_the_rows_it_promises():
    g = torch.Generator().manual_seed(1)
    for cin, cout in ((1, 1), (3, 5), (64, 255), (256, 132)):
        plan = ops.any_width_plan(cin, cout)
        ei, n, by_deg = at.ladder_graph(plan, g)
        deg = torch.bincount(ei[1], minlength=n)
        es, eb = plan["ES"], plan["B"] * plan["ES"]
        assert {0, 1, es, es + 1, eb - 1, eb, eb + 1, 2 * eb + 3, 4 * eb + es + 1} <= set(by_deg)
        for d, nodes in by_deg.items():
            assert all(int(deg[i]) == d for i in nodes)
        out_deg = torch.bincount(ei[0], minlength=n)
        assert int(out_deg[0]) == 0 and int(out_deg[1]) >= ei.shape[1] // 8 and int(deg[-3:].sum() + out_deg[-3:].sum()) == 0
        assert int((ei[0] == ei[1]).sum()) >= 1 and ei.shape[1] - torch.unique(ei, dim=1).shape[1] >= 1
        assert not bool((ei[1][1:] >= ei[1][:-1]).all())                              # unsorted
        assert ei.shape[1] <= 24 * eb + 64


@pytest.mark.parametrize("cin,cout", [(1, 1), (64, 255), (256, 132)])
def test_fp32_reference_chain_stays_far_inside_the_row_bars_on_the_ladder(cin, cout):
    """The row-by-row bars of tests/test_gpu_width_tilings.py (forward 1e-5, gradients 2e-5 of max(row norm, rms row norm)) leave
    room for correct fp32 arithmetic: the reference's own fp32 chain (oracle.nnconv_forward, float32) and fp32 autograd of the
    same statement, against float64 on the ladder graph, stay below a fifth of them."""
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    plan = ops.any_width_plan(cin, cout)
    ei, n, _ = at.ladder_graph(plan, g)
    e = ei.shape[1]
    ea = torch.randn(e, 4, generator=g)
    wl, bl = torch.randn(cin * cout, 4, generator=g) / (2 * cin ** 0.5), torch.randn(cin * cout, generator=g) / (2 * cin ** 0.5)
    x, _, root, bias, _, gout = at.draw_inputs(n, e, cin, cout, g)
    for aggr in ("add", "mean"):
        w = torch.nn.functional.linear(ea, wl, bl)                                   # the fp32 W_e both sides see
        y32 = nnconv_forward(x, ei, ea, [wl], [bl], root, bias, aggr=aggr, dtype=torch.float32)
        leaves64 = [t.double().requires_grad_(True) for t in (x, w, root, bias)]
        ref = at.reference64(leaves64[0], ei, leaves64[1], leaves64[2], leaves64[3], aggr)
        (ref * gout.double()).sum().backward()
        leaves32 = [t.clone().requires_grad_(True) for t in (x, w, root, bias)]
        (at.reference64(leaves32[0], ei, leaves32[1], leaves32[2], leaves32[3], aggr) * gout).sum().backward()
        figs = {"out": at.worst_row(y32, ref), "dW_e": at.worst_row(leaves32[1].grad, leaves64[1].grad),
                "dx": at.worst_row(leaves32[0].grad, leaves64[0].grad)}
        print(f"[ladder fp32 chain] {cin}->{cout} {aggr}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
        assert figs["out"] <= 2e-6 and figs["dW_e"] <= 4e-6 and figs["dx"] <= 4e-6, figs
