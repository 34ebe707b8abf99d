"""GPU tier: the K-loop schedule of the one-wave-per-SIMD fused kernel (csrc/gpde_fused_f16v6.hip, "what rides in the gap
behind MFMA n").  A schedule edit fails in four ways: a converted operand overwritten before its last reader or read
before its writer; a ring slot refilled or read early; a counted vmcnt wait retiring the wrong loads; the wrap from a
tile's last chunk into the next tile's first.  None of them shows in the arithmetic of one chunk, so the cases here vary
what the schedule depends on:

    kernel MLP            K1P / 32   mod 3 (ring slots)
    [6, 256, 256, 4096]       8         2      fewest chunks: 6 peeled + 2 steady
    [6, 288, 256, 4096]       9         0      odd: the store variant only (see below)
    [6, 320, 128, 4096]      10         1
    [6, 384, 256, 4096]      12         0
    [6, 1024, 1024, 4096]    32                the headline widths

(the slot a tile starts in rotates from tile to tile, hence the three residues; the forward entry gives this kernel even
chunk counts only - choose_fused in csrc/gpde_api.hip asks for the 8-wave kernel's support first - so at nine chunks the
forward runs the fp32 kernel and only the store variant, which has no such condition, runs the schedule; twelve chunks
carry residue 0 into the aggregation kernel), on skewed graphs of 33,000 - 40,000 edges
(at or above the 32,768-edge switch: the default precision picks this kernel, blocks hold many tiles, tiles span many
nodes and nodes many tiles).  Every case: the float64 oracle (1e-5 relative L2, the project's bar) and the 8-wave kernel
(5e-7: same products, different tile alignment), then bit reproducibility of the aggregation kernel and of the store
variant under memory pressure (tests/test_gpu_repeat.py: a cold-cache DMA piece or side load that a wrong wait lets
through shows as a result that differs from the first call)."""
import functools

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, rel_l2
from tests.test_gpu_parity import run_native
from tests.test_gpu_repeat import _repeat
from tests.test_gpu_v6 import _graph, _mlp
from tests.test_gpu_v6_layout import _root_bias, _segment_graph

pytestmark = pytest.mark.gpu
TOL = 1e-5
V6 = "f16split_agg16"       # forces this kernel below 32,768 edges
ODD = ("chunks9",)          # the forward entry does not run this kernel at an odd chunk count

CASES = {
    # name: dims, n, e, precision
    "chunks8": ([6, 256, 256, 4096], 700, 36000, "f16split"),
    "chunks9": ([6, 288, 256, 4096], 800, 34000, "f16split"),
    "chunks10": ([6, 320, 128, 4096], 900, 38000, "f16split"),
    "chunks12": ([6, 384, 256, 4096], 800, 35000, "f16split"),
    "chunks32": ([6, 1024, 1024, 4096], 300, 6000, V6),
    # fewer edges than two tiles: waves without a tile, and waves whose only tile is partial - a first chunk that no
    # earlier chunk wrapped into
    "tiny12": ([6, 384, 256, 4096], 50, 130, V6),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the float64 reference of a case: computed once, shared by the tests below, never modified."""
    dims, n, e, prec = CASES[name]
    ws_, bs_ = _mlp(dims, 11)
    x, ei, ea = _graph(n, e, dims[0], 12, skew=True)
    root, bias = _root_bias(13)
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    return dims, prec, x, ei, ea, ws_, bs_, root, bias, y64


def _device_case(name):
    dims, prec, x, ei, ea, ws_, bs_, root, bias, _ = _case(name)
    d = torch.device("cuda:0")
    wd, bd = [w.to(d) for w in ws_], [b.to(d) for b in bs_]
    pm = ops.pack_mlp(wd, bd)
    csr = ops.build_csr(ei.to(d), x.shape[0])
    if name not in ODD:
        assert ops.fused_kernel_name(x.shape[0], ei.shape[1], pm, prec) == "gpde_fused_f16v6_kernel"
    return d, prec, x.to(d), csr, ea.to(d), pm, wd, bd, root.to(d), bias.to(d)


@pytest.mark.parametrize("name", list(CASES))
def test_kloop_matches_oracle_and_8wave(name):
    dims, prec, x, ei, ea, ws_, bs_, root, bias, y64 = _case(name)
    d = torch.device("cuda:0")
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    if name not in ODD:
        assert ops.fused_kernel_name(x.shape[0], ei.shape[1], pm, prec) == "gpde_fused_f16v6_kernel"
    y6 = run_native(x, ei, ea, ws_, bs_, root, bias, "mean", precision=prec)
    y3 = run_native(x, ei, ea, ws_, bs_, root, bias, "mean", precision="f16split_8wave")
    assert torch.isfinite(y6).all()
    e6, e63 = rel_l2(y6, y64), rel_l2(y6, y3)
    print(f"{name}: rel-L2 vs float64 {e6:.3e}, vs the 8-wave kernel {e63:.3e}")
    assert e6 <= TOL, (name, e6)
    assert e63 <= 5e-7, (name, e63)


@pytest.mark.parametrize("name", ["chunks8", "chunks9", "chunks10", "chunks12", "chunks32"])
def test_aggregation_kernel_is_reproducible_under_memory_pressure(name):
    d, prec, x, csr, ea, pm, _, _, root, bias = _device_case(name)
    _repeat(lambda: ops.nnconv_forward_raw(x, csr, ea, pm, root, bias, "mean", precision=prec), d, 20)


@pytest.mark.parametrize("name", ["chunks8", "chunks9", "chunks10", "chunks12", "chunks32"])
def test_store_variant_is_reproducible_under_memory_pressure(name):
    """ops.hidden_forward_raw: the kernel's store variant (the backward's recompute of H_2), static edge ranges."""
    d, _, _, csr, ea, pm, wd, bd, _, _ = _device_case(name)
    assert pm.dims[1] > 7 * 32                # >= 8 k1 chunks: the store entry takes this kernel at any edge count
    _repeat(lambda: ops.hidden_forward_raw(csr, ea, pm, wd[:-1] + [None], bd[:-1] + [None], "f16split"), d, 20)


def test_node_table_equals_tensor_bitwise_at_twelve_chunks():
    """The node-table instantiations share the schedule but carry one more side load in a tile's first chunk (source and
    destination ids): the graph of tests/test_gpu_v6_layout.py (segment boundaries at every offset) at K1P = 384, ring residue
    0.  (At nine chunks the node-table forward is refused as unsupported: it exists on the f16-split kernels only, and
    those take even chunk counts.)"""
    x, ei, ea, pos, a = _segment_graph()
    d = torch.device("cuda:0")
    ws_, bs_ = _mlp([6, 384, 256, 4096], 1)
    root, bias = _root_bias(3)
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    assert ops.fused_kernel_name(x.shape[0], ei.shape[1], pm, V6) == "gpde_fused_f16v6_kernel"
    csr = ops.build_csr(ei.to(d), x.shape[0])
    na = gp.NodeAttr.darcy(pos.to(d), a.to(d))
    assert torch.equal(na.materialize(ei.to(d)).cpu(), ea)
    y_t = ops.nnconv_forward_raw(x.to(d), csr, ea.to(d), pm, root.to(d), bias.to(d), "mean", precision=V6)
    y_n = ops.nnconv_forward_nodeattr_raw(x.to(d), csr, na, pm, root.to(d), bias.to(d), "mean", precision=V6)
    torch.cuda.synchronize()
    assert torch.equal(y_t, y_n), rel_l2(y_n.cpu(), y_t.cpu())
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    assert rel_l2(y_n.cpu(), y64) <= TOL
