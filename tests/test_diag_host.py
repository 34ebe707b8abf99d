"""The diagonal-kernel operator without a GPU: the plan query the GPU tier builds its graphs from, the C entry points' argument
validation (before any device call), the module surface of NNConvDiag / NNConvGaussian, the shim, and the float64 helper against the
fixtures made by the reference's own classes (tests/golden/make_golden_diag.py)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from graph_pde_amd.message_passing import MessagePassing
from tests.helpers import diag_oracle as do

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(REPO, "graph-pde_amd", "shims")
EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("aligned", [True, False])
def test_plan_invariants_at_every_width(aligned):
    for w in range(1, ops.ANY_MAX_WIDTH + 1):
        p = ops.diag_plan(w, aligned=aligned)
        assert p["lanes"] == p["LC"] * p["ES"] <= 64 and p["active_lanes"] <= p["lanes"], (w, p)
        assert p["LC"] & (p["LC"] - 1) == 0 and p["LC"] >= 1, (w, p)
        assert p["V"] in (1, 4) and (p["V"] == 1 or (w % 4 == 0 and aligned)), (w, p)
        assert p["V"] == (4 if (w % 4 == 0 and aligned) else 1), (w, p)
        assert p["consecutive"] == (1 if w % 4 == 0 else 0), (w, p)
        assert p["LC"] * p["per_lane"] >= w and 1 <= p["per_lane"] <= 4, (w, p)         # every channel has a lane
        assert p["pass_edges"] % p["ES"] == 0 and p["chain_edges"] % p["pass_edges"] == 0, (w, p)
        assert p["lanes"] * 8 * 4 <= p["lds_bytes"] <= 64 * 1024, (w, p)                 # the slots' sums (8 floats per lane) fit the LDS
        assert p == ops.diag_plan(w, aligned=aligned, aggr="max") == ops.diag_plan(w, aligned=aligned, aggr="mean")
        # the tiling and the summation order depend on the width alone: alignment changes V, nothing else
        q = ops.diag_plan(w, aligned=not aligned)
        assert {k: v for k, v in p.items() if k != "V"} == {k: v for k, v in q.items() if k != "V"}, (w, p, q)
    assert ops.diag_plan(32)["active_lanes"] == 64 and ops.diag_plan(8)["active_lanes"] == 64      # narrow widths fill the wave
    assert ops.diag_plan(64)["ES"] == 4 and ops.diag_plan(256)["ES"] == 1


def test_plan_refusals():
    for w in (0, -1, 257):
        with pytest.raises(NotImplementedError, match="width"):
            ops.diag_plan(w)
    with pytest.raises(NotImplementedError):
        ops.diag_plan(8, aggr="min")
    l = _lib.lib()
    assert l.gpde_diagconv_plan(8, 1, 0, None) == EINVAL and b"gpde_diagconv_plan" in l.gpde_last_error()
    out = (ctypes.c_int32 * 10)()
    assert l.gpde_diagconv_plan(8, 1, 7, out) == EINVAL and b"aggr" in l.gpde_last_error()


def test_entry_points_validate_on_the_host():
    l = _lib.lib()
    buf, other = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 16)
    # gpde_diagconv_fwd(x_src, n_src, x_dst, n_dst, k, n_edges, rowptr, src, root, bias, residual, relu, aggr, width, in_dst, out, stream)
    fwd = l.gpde_diagconv_fwd
    assert fwd(None, 4, None, 4, None, 8, None, None, None, None, None, 0, 0, 8, 8, None, None) == EINVAL
    assert b"gpde_diagconv_fwd" in l.gpde_last_error() and b"null" in l.gpde_last_error()
    assert fwd(buf, 4, buf, 4, buf, 8, buf, None, None, None, None, 0, 0, 8, 8, other, None) == EINVAL        # edges without src
    assert fwd(buf, 4, buf, 4, buf, 8, buf, buf, None, None, None, 0, 5, 8, 8, other, None) == EINVAL and b"unknown aggr" in l.gpde_last_error()
    assert fwd(buf, -1, buf, 4, buf, 8, buf, buf, None, None, None, 0, 0, 8, 8, other, None) == EINVAL
    assert fwd(buf, 0, buf, 4, buf, 8, buf, buf, None, None, None, 0, 0, 8, 8, other, None) == EINVAL and b"without sources" in l.gpde_last_error()
    assert fwd(buf, 4, None, 4, buf, 8, buf, buf, buf, None, None, 0, 0, 8, 8, other, None) == EINVAL and b"root without x_dst" in l.gpde_last_error()
    assert fwd(buf, 4, buf, 4, buf, 8, buf, buf, None, None, other, 0, 0, 8, 8, other, None) == EINVAL and b"residual aliases out" in l.gpde_last_error()
    assert fwd(buf, 4, buf, 4, other, 8, other, other, None, None, None, 0, 0, 8, 8, buf, None) == EINVAL and b"overlaps x_src" in l.gpde_last_error()
    for w in (0, 257, -4):
        assert fwd(buf, 4, buf, 4, buf, 8, buf, buf, None, None, None, 0, 0, w, 8, other, None) == EUNSUPPORTED and b"width" in l.gpde_last_error()
    for cind in (0, 257):
        assert fwd(buf, 4, buf, 4, buf, 8, buf, buf, None, None, None, 0, 0, 8, cind, other, None) == EUNSUPPORTED and b"in_dst" in l.gpde_last_error()
    assert fwd(None, 0, None, 0, None, 0, buf, None, None, None, None, 0, 0, 8, 8, None, None) == 0          # no node: a valid call
    # gpde_diagconv_bwd(x_src, n_src, x_dst, n_dst, k, n_edges, rowptr, src, dst, src_rowptr, src_slots, root, aggr, width, in_dst, grad_out,
    #                   grad_x_src, grad_x_dst, grad_k, grad_root, grad_bias, ws, ws_bytes, stream)
    bwd = l.gpde_diagconv_bwd
    big = 1 << 16
    assert l.gpde_diagconv_bwd_workspace_bytes(4, 8, 8) > 0 and l.gpde_diagconv_bwd_workspace_bytes(4, 300, 8) == 0
    assert l.gpde_diagconv_bwd_workspace_bytes(-1, 8, 8) == 0 and l.gpde_diagconv_bwd_workspace_bytes(4, 8, 0) == 0
    assert bwd(buf, 4, buf, 4, buf, 8, None, buf, buf, buf, buf, None, 0, 8, 8, buf, buf, None, buf, None, None, buf, big, None) == EINVAL
    assert b"gpde_diagconv_bwd" in l.gpde_last_error()
    assert bwd(buf, 4, buf, 4, buf, 8, buf, buf, buf, None, None, None, 0, 8, 8, buf, other, None, None, None, None, buf, big, None) == EINVAL
    assert b"gpde_csr_source_order" in l.gpde_last_error() and b"never by atomics" in l.gpde_last_error()
    assert bwd(buf, 4, buf, 4, buf, 8, buf, buf, None, buf, buf, None, 0, 8, 8, buf, other, None, None, None, None, buf, big, None) == EINVAL   # no dst
    assert bwd(buf, 4, None, 4, buf, 8, buf, buf, buf, buf, buf, None, 0, 8, 8, buf, None, None, None, other, None, buf, big, None) == EINVAL
    assert b"without x_dst" in l.gpde_last_error()
    assert bwd(buf, 4, buf, 4, buf, 8, buf, buf, buf, buf, buf, None, 2, 8, 8, buf, other, None, None, None, None, buf, big, None) == EUNSUPPORTED
    assert b"GPDE_AGGR_ADD and GPDE_AGGR_MEAN" in l.gpde_last_error()
    assert bwd(buf, 4, buf, 4, buf, 8, buf, buf, buf, buf, buf, None, 9, 8, 8, buf, other, None, None, None, None, buf, big, None) == EINVAL
    assert bwd(buf, 4, buf, 4, buf, 8, buf, buf, buf, buf, buf, None, 0, 257, 8, buf, other, None, None, None, None, buf, big, None) == EUNSUPPORTED
    assert bwd(buf, 4, buf, 4, buf, 8, buf, buf, buf, buf, buf, None, 0, 8, 8, buf, other, None, None, None, None, buf, 16, None) == -3
    assert b"workspace" in l.gpde_last_error()
    assert bwd(buf, 4, buf, 4, buf, 8, buf, buf, buf, buf, buf, None, 0, 8, 8, buf, other, None, buf, None, None, buf, big, None) == EINVAL
    assert b"grad_k aliases k" in l.gpde_last_error()


def _lin(w, k0=3):
    return torch.nn.Sequential(torch.nn.Linear(k0, 16), torch.nn.ReLU(), torch.nn.Linear(16, w))


@pytest.mark.parametrize("cls", [gp.NNConvDiag, gp.NNConvGaussian])
def test_module_surface(cls):
    torch.manual_seed(0)
    conv = cls(24, 24, _lin(24), aggr="mean")
    assert isinstance(conv, MessagePassing) and isinstance(conv, torch.nn.Module)
    assert tuple(conv.root.shape) == (24, 24) and tuple(conv.bias.shape) == (24,)
    bound = 1 / math.sqrt(24)
    root, bias = conv.root.detach(), conv.bias.detach()
    assert float(root.abs().max()) <= bound and float(bias.abs().max()) <= bound and float(root.abs().max()) > bound / 2
    assert list(conv.state_dict()) == ["root", "bias", "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]     # the reference's keys
    assert repr(conv) == f"{cls.__name__}(24, 24)" and conv.aggr == "mean" and conv.in_channels == 24 and conv.out_channels == 24
    nr = cls(8, 8, _lin(8), root_weight=False, bias=False)
    assert nr.root is None and nr.bias is None and list(nr.state_dict()) == ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]
    pair = cls((8, 5), 8, _lin(8), flow="target_to_source")
    assert tuple(pair.root.shape) == (5, 8) and float(pair.root.detach().abs().max()) <= 1 / math.sqrt(8) and pair.flow == "target_to_source"
    before = conv.root.clone()
    conv.reset_parameters()
    assert not torch.equal(before, conv.root)
    with pytest.raises(ValueError, match="in_channels == out_channels"):
        cls(8, 16, _lin(16))
    with pytest.raises(ValueError, match="in_channels == out_channels"):
        cls((5, 8), 8, _lin(8))
    with pytest.raises(NotImplementedError, match="nn must be a torch.nn.Module"):
        cls(1, 1, None)
    with pytest.raises(NotImplementedError, match="nn must be a torch.nn.Module"):
        cls(8, 8, lambda t: t)
    with pytest.raises(NotImplementedError, match="widths 1 .. 256"):
        cls(300, 300, _lin(300))
    with pytest.raises(ValueError, match="aggr"):
        cls(8, 8, _lin(8), aggr="min")
    with pytest.raises(ValueError, match="flow"):
        cls(8, 8, _lin(8), flow="sideways")


def test_wrong_kernel_shape_and_refused_calls():
    """Raised before any device is looked at."""
    x, ei, ea = torch.randn(6, 8), torch.tensor([[0, 1, 2], [1, 2, 3]]), torch.rand(3, 3) + 0.5
    with pytest.raises(ValueError, match=r"nn_conv.py:84"):
        gp.NNConvDiag(8, 8, _lin(9)).message(x[ei[0]], ea)
    with pytest.raises(ValueError, match=r"nn_conv.py:175-180"):
        gp.NNConvGaussian(8, 8, torch.nn.Linear(1, 9)).message(x[ei[0]], ea)
    assert tuple(gp.NNConvGaussian(8, 8, torch.nn.Linear(1, 8)).message(x[ei[0]], ea).shape) == (3, 8)
    conv = gp.NNConvDiag((8, 5), 8, _lin(8), aggr="max")
    with pytest.raises(NotImplementedError, match="aggr='max' with a gradient on a call between two node sets"):
        conv((x, torch.randn(4, 5)), ei, ea, size=(6, 4))
    with pytest.raises(NotImplementedError, match="NodeAttr"):
        conv((x, torch.randn(4, 5)), ei, ops.NodeAttr(torch.randn(6, 3), [(0, 0), (1, 1), (0, 2)]), size=(6, 4))
    with pytest.raises(ValueError, match="activation"):
        conv(x, ei, ea, activation="gelu")
    with pytest.raises(ValueError, match=r"x must be \[N, 8\]"):
        gp.NNConvDiag(8, 8, _lin(8))(torch.randn(6, 9), ei, ea)


def test_the_shim_names_the_diagonal_classes():
    code = ("import nn_conv, graph_pde_amd, torch_geometric.nn as tgnn\n"
            "assert nn_conv.NNConv is graph_pde_amd.NNConvDiag and nn_conv.NNConv_Gaussian is graph_pde_amd.NNConvGaussian\n"
            "assert nn_conv.ECConv is nn_conv.NNConv and nn_conv.NNConv_old is graph_pde_amd.NNConv_old\n"
            "assert tgnn.NNConv is graph_pde_amd.NNConv and issubclass(tgnn.NNConv, graph_pde_amd.NNConv_old)\n"
            "assert not issubclass(nn_conv.NNConv, graph_pde_amd.NNConv_old)\nprint('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd="/tmp", env=dict(os.environ, PYTHONPATH=SHIMS), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("name", ["diag_w8", "diag_gauss_w64"])
def test_the_float64_helper_reproduces_the_reference(name):
    g = do.load_golden(name)
    assert g["x"].shape[0] == 16 and os.path.getsize(os.path.join(do.GOLDEN, name + ".npz")) < 64 * 1024
    x = g["x"].double()
    out = do.diag_reference(x, x, g["edge_index"], do.golden_kernel(g, torch.float64), g["root"].double(), g["bias"].double(), g["aggr"])
    scale = float(g["out_f64"].abs().max())
    assert float((out - g["out_f64"]).abs().max()) <= 1e-12 * scale
    assert float((g["out_f32"].double() - g["out_f64"]).abs().max()) <= 1e-5 * scale        # the reference's own float32 run
    if name == "diag_gauss_w64":
        assert float((g["edge_attr"][:, 1] * g["edge_attr"][:, 2]).abs().min()) >= 0.25
