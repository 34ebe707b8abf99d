"""GCNConv without a GPU: the float64 checker against a graph worked by hand, the module's construction surface and host path,
the shim, the C entry points' argument validation and the plan query the GPU tier takes its tiling classes from."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops
from tests.helpers import gcn_oracle as go

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(REPO, "graph-pde_amd", "shims")


def test_oracle_reproduces_a_graph_worked_by_hand():
    """4 nodes, edges 0->1, 2->1, 1->2, 3->3 (w = 0.5), 3->3 (w = 4): node 3 has two self loops, the later one (w = 4) is its self
    weight; nodes 0, 1, 2 get a self loop of weight 1.  deg = [1, 3, 2, 4]; dinv = [1, 1/sqrt 3, 1/sqrt 2, 1/2].
      coef(0->1) = 1 * 1/sqrt 3, coef(2->1) = 1/sqrt 2 * 1/sqrt 3 = 1/sqrt 6, coef(1->2) = 1/sqrt 6, both self-loop edges 0
      self_coef = [1, 1/3, 1/2, 4 * 1/4 = 1]
    x = [1, 2, 3, 4] (one channel), W = [[2]], bias = [1]:
      agg = [1, 1/sqrt 3 + 3/sqrt 6 + 2/3, 2/sqrt 6 + 3/2, 4];   out = 2 agg + 1"""
    ei = torch.tensor([[0, 2, 1, 3, 3], [1, 1, 2, 3, 3]])
    ew = torch.tensor([1.0, 1.0, 1.0, 0.5, 4.0])
    coef, selfc = go.coefficients(ei, 4, ew)
    s3, s6 = math.sqrt(3.0), math.sqrt(6.0)
    assert coef.tolist() == pytest.approx([1 / s3, 1 / s6, 1 / s6, 0.0, 0.0], rel=1e-15)
    assert selfc.tolist() == pytest.approx([1.0, 1 / 3, 0.5, 1.0], rel=1e-15)
    x = torch.tensor([[1.0], [2.0], [3.0], [4.0]], dtype=torch.float64)
    out = go.forward(x, ei, torch.tensor([[2.0]], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64), edge_weight=ew)
    agg = [1.0, 1 / s3 + 3 / s6 + 2 / 3, 2 / s6 + 1.5, 4.0]
    assert out.view(-1).tolist() == pytest.approx([2 * a + 1 for a in agg], rel=1e-15)
    # improved: the fill is 2 where there is no self-loop edge; node 3 keeps 4
    _, selfc2 = go.coefficients(ei, 4, ew, improved=True)
    assert selfc2.tolist() == pytest.approx([2 / 2, 2 / 4, 2 / 3, 4 / 4], rel=1e-15)
    # no self loops added: self-loop edges are ordinary edges, deg = in-weights [0, 2, 1, 4.5]
    coef3, selfc3 = go.coefficients(ei, 4, ew, add_self_loops=False)
    assert selfc3.tolist() == [0.0] * 4 and coef3.tolist() == pytest.approx([0.0, 1 / math.sqrt(2), 1 / math.sqrt(2), 0.5 / 4.5, 4 / 4.5], rel=1e-15)
    coef4, selfc4 = go.coefficients(ei, 4, ew, normalize=False)
    assert coef4.tolist() == ew.tolist() and selfc4.tolist() == [0.0] * 4


def test_construction_surface():
    conv = gp.GCNConv(128, 128)
    assert isinstance(conv, gp.message_passing.MessagePassing)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {"weight": (128, 128), "bias": (128,)}
    assert gp.GCNConv(3, 5, bias=False).bias is None and tuple(gp.GCNConv(3, 5).weight.shape) == (3, 5)
    bound = math.sqrt(6.0 / (3 + 200))
    c = gp.GCNConv(3, 200)
    assert float(c.weight.detach().abs().max()) <= bound and float(c.weight.detach().abs().max()) > 0.8 * bound and float(c.bias.detach().abs().max()) == 0.0
    w0 = c.weight.detach().clone()
    with torch.no_grad():
        c.bias.fill_(3.0)
    c.reset_parameters()
    assert not torch.equal(c.weight, w0) and float(c.bias.detach().abs().max()) == 0.0
    # the newer layout: lin.weight [out, in]
    lw, b = torch.randn(200, 3), torch.randn(200)
    c.load_state_dict({"lin.weight": lw, "bias": b})
    assert torch.equal(c.weight, lw.t()) and torch.equal(c.bias, b)
    c.load_state_dict({"weight": lw.t().contiguous() * 2, "bias": b})
    assert torch.equal(c.weight, lw.t() * 2)
    with pytest.raises(NotImplementedError, match="improved must be True or False"):
        gp.GCNConv(1, 1, None)
    for kw in ("cached", "bias", "normalize", "add_self_loops"):
        with pytest.raises(NotImplementedError, match=f"{kw} must be True or False"):
            gp.GCNConv(1, 1, **{kw: 1})
    for i, o in ((0, 4), (4, 0), (257, 4), (4, 257)):
        with pytest.raises(ValueError):
            gp.GCNConv(i, o)
    assert gp.GCNConv(256, 1) is not None and gp.GCNConv(1, 256) is not None


def test_the_shim_exports_the_class():
    code = ("from torch_geometric.nn import GCNConv\nimport graph_pde_amd\nassert GCNConv is graph_pde_amd.GCNConv\n"
            "c = GCNConv(4, 6)\nprint('ok', tuple(c.weight.shape))")
    r = subprocess.run([sys.executable, "-c", code], cwd="/tmp", env=dict(os.environ, PYTHONPATH=SHIMS), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok (4, 6)" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("graph", ["ladder", "selfloops"])
@pytest.mark.parametrize("kw", [dict(), dict(improved=True), dict(normalize=False), dict(add_self_loops=False)], ids=str)
@pytest.mark.parametrize("weighted", [False, True])
def test_host_path_equals_the_oracle(graph, kw, weighted):
    torch.manual_seed(11)
    ei, n = getattr(go, graph)()
    ew = go.weights_for(ei) if weighted else None
    conv = gp.GCNConv(5, 7, **kw)
    with torch.no_grad():
        conv.bias.uniform_(-1, 1)
    x = torch.randn(n, 5, requires_grad=True)
    y = conv(x, ei, ew)
    g = torch.randn(n, 7)
    y.backward(g)
    ref, gx, gw, gb = go.gradients(x, ei, conv.weight, conv.bias, g, edge_weight=ew, **kw)
    for name, a, b in (("out", y, ref), ("grad_x", x.grad, gx), ("grad_weight", conv.weight.grad, gw), ("grad_bias", conv.bias.grad, gb)):
        assert go.rel_l2(a, b) <= 1e-6, (name, go.rel_l2(a, b))


def test_host_path_module_options():
    torch.manual_seed(12)
    ei, n = go.directed()
    x = torch.randn(n)                                      # one-dimensional x is [N, 1]
    c = gp.GCNConv(1, 3)
    assert torch.equal(c(x, ei), c(x.view(-1, 1), ei))
    t2s = gp.GCNConv(1, 3, flow="target_to_source")
    t2s.load_state_dict(c.state_dict())
    assert torch.equal(t2s(x, ei), c(x, ei.flip(0)))
    assert not torch.equal(t2s(x, ei), c(x, ei))           # the graph is directed: the flow matters
    cached = gp.GCNConv(1, 3, cached=True)
    cached.load_state_dict(c.state_dict())
    first = cached(x, ei)
    assert torch.equal(cached(x, ei.flip(0)), first) and not torch.equal(c(x, ei.flip(0)), first)
    with pytest.raises(NotImplementedError, match="edge_weight"):
        c(x, ei, torch.ones(ei.size(1), requires_grad=True))
    with pytest.raises(ValueError):
        c(torch.randn(n, 2), ei)


def _header():
    return open(os.path.join(REPO, "include", "gpde.h")).read()


def test_flag_values_match_the_header():
    hdr = _header()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"(GPDE_GCN_\w+)\s*=\s*(\d+)", hdr)}
    assert (vals["GPDE_GCN_ADD_SELF_LOOPS"], vals["GPDE_GCN_IMPROVED"], vals["GPDE_GCN_NORMALIZE"], vals["GPDE_GCN_RELU"]) == \
        (ops.GCN_ADD_SELF_LOOPS, ops.GCN_IMPROVED, ops.GCN_NORMALIZE, ops.GCN_RELU)
    assert ops.gcn_flags() == ops.GCN_ADD_SELF_LOOPS | ops.GCN_NORMALIZE and ops.gcn_flags(True, False, False) == ops.GCN_IMPROVED


def test_entry_points_validate_on_the_host():
    l = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    # gpde_gcn_norm(rowptr, src, perm, edge_weight, n_nodes, n_edges, flags, coef, self_coef, ws, ws_bytes, stream)
    assert l.gpde_gcn_norm(None, None, None, None, 4, 8, 5, None, None, None, 0, None) == -1 and b"gpde_gcn_norm" in l.gpde_last_error()
    assert l.gpde_gcn_norm(buf, buf, None, buf, 4, 8, 5, buf, buf, buf, 4096, None) == -1          # edge_weight without perm
    assert l.gpde_gcn_norm(buf, buf, buf, None, 4, 8, 64, buf, buf, buf, 4096, None) == -1 and b"flags" in l.gpde_last_error()
    assert l.gpde_gcn_norm(buf, buf, buf, None, -1, 8, 5, buf, buf, buf, 4096, None) == -1
    assert l.gpde_gcn_norm(buf, buf, buf, None, 4, 8, 5, buf, buf, None, 0, None) == -1            # no workspace
    assert l.gpde_gcn_norm(None, None, None, None, 0, 0, 5, None, None, None, 0, None) == 0        # no nodes: no pointer is read
    assert l.gpde_gcn_norm(None, None, None, None, 0, 3, 5, None, None, None, 0, None) == -1       # edges without nodes
    assert l.gpde_gcn_norm_workspace_bytes(1000, 5000) >= 12000 and l.gpde_gcn_norm_workspace_bytes(-1, 0) == 0
    # gpde_gcn_fwd(x, n_nodes, n_edges, rowptr, src, coef, self_coef, W, bias, in, out, flags, out, agg_out, stream)
    assert l.gpde_gcn_fwd(None, 4, 8, None, None, None, None, None, None, 8, 8, 0, None, None, None) == -1
    assert b"gpde_gcn_fwd" in l.gpde_last_error()
    for cin, cout in ((0, 8), (8, 0), (257, 8), (8, 257), (-3, 8)):
        assert l.gpde_gcn_fwd(buf, 4, 8, buf, buf, buf, buf, buf, buf, cin, cout, 0, buf, None, None) == -1
        assert b"widths" in l.gpde_last_error()
    assert l.gpde_gcn_fwd(buf, 4, 8, buf, buf, buf, buf, None, buf, 8, 9, 0, buf, None, None) == -1 and b"W == NULL" in l.gpde_last_error()
    assert l.gpde_gcn_fwd(buf, 4, 8, buf, buf, buf, buf, buf, buf, 8, 8, 2, buf, None, None) == -1 and b"flags" in l.gpde_last_error()
    assert l.gpde_gcn_fwd(buf, 4, 8, buf, None, None, buf, buf, buf, 8, 8, 0, buf, None, None) == -1      # edges without src / coef
    x = ctypes.create_string_buffer(4096)
    assert l.gpde_gcn_fwd(x, 4, 8, buf, buf, buf, buf, buf, buf, 8, 8, 0, x, None, None) == -1 and b"overlap" in l.gpde_last_error()
    # as gpde_hidden_fwd: a call without work returns GPDE_OK before any pointer is looked at
    assert l.gpde_gcn_fwd(None, 0, 0, None, None, None, None, None, None, 8, 8, 0, None, None, None) == 0
    assert l.gpde_gcn_fwd(None, 0, 5, None, None, None, None, None, None, 8, 8, 0, None, None, None) == -1
    assert l.gpde_gcn_plan(8, 8, None) == -1


@functools.lru_cache(maxsize=None)
def plan_classes():
    """One (in, out) pair per tiling class gpde_gcn_plan reports over 1 .. 256 x 1 .. 256: (channel passes per lane, column blocks
    per wave, K tail, column tail) - the first pair found of each.  tests/test_gpu_gcn.py iterates over this list."""
    seen = {}
    for cin in range(1, 257):
        for cout in range(1, 257):
            p = ops.gcn_plan(cin, cout)
            seen.setdefault((p["passes"], p["col_blocks_per_wave"], p["k_tail"], p["col_tail"]), (cin, cout))
    return seen


def test_plan_answers_for_every_width():
    for cin in range(1, 257):
        for cout in (1, 31, 32, 33, 128, 129, 256):
            p = ops.gcn_plan(cin, cout)
            assert p["rows"] == 64 and p["kstride"] >= cin + (cin & 1) and p["kstride"] % 64 == 2
            assert p["passes"] == -(-cin // 64) and p["col_blocks"] == -(-cout // 32) and p["col_blocks_per_wave"] == -(-p["col_blocks"] // 4)
            assert p["k_tail"] == cin % 2 and p["col_tail"] == (1 if cout % 32 else 0) and p["lds_bytes"] == 64 * p["kstride"] * 4
            assert p["lds_bytes"] <= 160 * 1024
    cls = plan_classes()
    assert len(cls) == 4 * 2 * 2 * 2, sorted(cls)
    for bad in ((0, 1), (1, 0), (257, 1), (1, 257)):
        with pytest.raises(_lib.GpdeError):
            ops.gcn_plan(*bad)
    assert ops.GCN_ROUTES == ("aggregate_first", "aggregate_mm", "transform_first")
    assert ops.gcn_route(3, 5) == "aggregate_mm" and ops.gcn_route(128, 128) == "transform_first" and ops.gcn_route(256, 130) == "transform_first"


def test_norm_refuses_what_it_does_not_cover():
    z = torch.zeros(0, dtype=torch.int32)
    rect = ops.Csr(4, 0, torch.zeros(5, dtype=torch.int32), z, z, z, n_src_nodes=3)
    with pytest.raises(ValueError, match="one node set"):
        ops.gcn_norm(rect)
    with pytest.raises(TypeError):
        ops.gcn_norm(torch.zeros(2, 3, dtype=torch.int64))
    sq = ops.Csr(4, 0, torch.zeros(5, dtype=torch.int32), z, z, z)
    with pytest.raises(NotImplementedError, match="edge_weight"):
        ops.gcn_norm(sq, torch.ones(0, requires_grad=True))
