"""GPU tier: the operand layouts of the one-wave-per-SIMD fused kernel on v_mfma_f32_16x16x32_f16
(csrc/gpde_fused_f16v6.hip): a lane owns 4 consecutive edges of a 16-edge block and one hidden column of a
16-column block; H1 comes from ONE K = 32 MFMA whose lane groups carry the three split terms; the aggregation
covers a 32-edge half with one K = 32 MFMA.  What can go wrong with that is positional - a segment boundary at
some offset inside a tile, a partial 16-edge block, the bias slot in some attribute position, a ragged width -
so the graphs here are small and built to hit every position, and every case is compared with the float64
oracle (bars of tests/test_gpu_v6.py: 1e-5 relative L2, 4 x the fp32 kernel's error + 2e-7) and with the
8-wave kernel (5e-7).  The small graphs force the kernel with precision="f16split_agg16"."""
import functools

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, rel_l2
from tests.test_gpu_parity import run_native

pytestmark = pytest.mark.gpu
TOL = 1e-5
V6 = "f16split_agg16"


def _mlp(dims, seed):
    torch.manual_seed(seed)
    layers = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
    return [l.weight.detach() for l in layers], [l.bias.detach() for l in layers]


def _root_bias(seed):
    torch.manual_seed(seed)
    return torch.randn(64, 64) / 8, torch.randn(64) / 8


def _check(name, x, ei, ea, dims, seed=1, rows=False):
    """The new kernel against float64, the fp32 kernel's own error and the 8-wave kernel; returns (y, y64)."""
    ws_, bs_ = _mlp(dims, seed)
    root, bias = _root_bias(seed + 2)
    d = torch.device("cuda:0")
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    assert ops.fused_kernel_name(x.shape[0], ei.shape[1], pm, V6) == "gpde_fused_f16v6_kernel"
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    y6 = run_native(x, ei, ea, ws_, bs_, root, bias, "mean", precision=V6)
    y3 = run_native(x, ei, ea, ws_, bs_, root, bias, "mean", precision="f16split_8wave")
    y32 = run_native(x, ei, ea, ws_, bs_, root, bias, "mean", precision="f32")
    assert torch.isfinite(y6).all()
    e6, e32 = rel_l2(y6, y64), rel_l2(y32, y64)
    assert e6 <= TOL and e6 <= 4 * e32 + 2e-7, (name, e6, e32)
    assert rel_l2(y6, y3) <= 5e-7, (name, rel_l2(y6, y3))
    if rows:
        # every output row on its own.  A row's error is bounded relative to the size of the terms that were summed, not of
        # what is left after they cancel: the scale is the row's norm, floored by the median row norm.  An edge added to the
        # wrong row, or dropped, moves a row by >= 1 / 700 of a term (the largest in-degree here) - two orders above the bar
        nr = y64.norm(dim=1)
        scale = torch.maximum(nr, nr.median())
        err = ((y6.double() - y64).norm(dim=1) / scale)
        assert err.max().item() <= TOL, (name, int(err.argmax()), err.max().item())
    return y6, y64


@functools.lru_cache(maxsize=None)
def _segment_graph():
    """284 nodes whose in-degrees run over 0, 1, ..., 70 (four of each, shuffled) and one node of 700 in-edges: every node
    boundary falls on every offset modulo 16 and 32 inside a 64-edge tile, tiles hold 1 to 64 segments, one node spans
    11 tiles.  The attributes come from node data, so that the node-table kernel can run on the same graph."""
    g = torch.Generator().manual_seed(41)
    deg = torch.tensor(list(range(71)) * 4 + [700])
    deg = deg[torch.randperm(deg.numel(), generator=g)]
    n = deg.numel()
    dst = torch.repeat_interleave(torch.arange(n), deg)
    dst = dst[torch.randperm(dst.numel(), generator=g)]            # the CSR build sorts them back; perm is non-trivial
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    ei = torch.stack([src, dst])
    pos = torch.rand(n, 2, generator=g)
    a = torch.rand(n, generator=g) * 8 + 4
    na_cpu = gp.NodeAttr.darcy(pos, a)
    ea = na_cpu.materialize(ei)
    x = torch.randn(n, 64, generator=g)
    return x, ei, ea, pos, a


def test_segment_boundaries_at_every_offset():
    x, ei, ea, _, _ = _segment_graph()
    assert ei.shape[1] == 4 * 2485 + 700
    _check("segments", x, ei, ea, [6, 256, 256, 4096], rows=True)


def _ragged_graph(n, e, k0, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(n, generator=g) ** 4
    w[: n // 6] = 0
    dst = torch.multinomial(w, e, replacement=True, generator=g)
    src = torch.randint(0, n, (e,), generator=g)
    return torch.randn(n, 64, generator=g), torch.stack([src, dst]), torch.randn(e, k0, generator=g)


@pytest.mark.parametrize("rem", [1, 15, 16, 17, 33, 63])
def test_partial_last_tile_and_partial_16_edge_block(rem):
    x, ei, ea = _ragged_graph(60, 64 * 9 + rem, 6, 50 + rem)
    _check(f"rem{rem}", x, ei, ea, [6, 256, 256, 4096], rows=True)


@pytest.mark.parametrize("k0", [1, 3, 6, 7])
def test_attribute_slots_and_the_bias_slot(k0):
    """The bias slot sits at position k0 of the 8 slots of a lane group; the slots behind it and lane group 3 are zero."""
    x, ei, ea = _ragged_graph(90, 1500 + k0, k0, 60 + k0)
    _check(f"k0_{k0}", x, ei, ea, [k0, 256, 256, 4096], seed=7)


@pytest.mark.parametrize("dims,e", [([6, 250, 130, 4096], 5000), ([6, 1024, 1024, 4096], 3000)],
                         ids=["k250_k130", "k1024"])
def test_ragged_and_headline_widths(dims, e):
    """K1P = 256 with 6 padded rows / K2P = 256 with 126 padded columns (two column slices); the headline MLP."""
    x, ei, ea = _ragged_graph(250, e, 6, 70)
    _check("widths", x, ei, ea, dims, seed=9)


def _hidden_check(name, ei, ea, n, dims, seed):
    """ops.hidden_forward_raw (the store variant): every [slot][k2] entry against float64, hmax = max of the stored rows.
    Bar per entry: 1e-5 of the sum of the absolute terms of that entry, |b2| + sum_k |W2[c][k]| H1[k] - the forward error
    bound of a dot product is relative to that sum, not to what is left of it (the split drops lo x lo, 2^-22 per term,
    fp32 accumulation adds k1 x 2^-24)."""
    ws_, bs_ = _mlp(dims, seed)
    d = torch.device("cuda:0")
    csr = ops.build_csr(ei.to(d), n)
    wd, bd = [w.to(d) for w in ws_], [b.to(d) for b in bs_]
    pm = ops.pack_mlp(wd, bd)
    H, hmax = ops.hidden_forward_raw(csr, ea.to(d), pm, wd[:-1] + [None], bd[:-1] + [None], "f16split")
    torch.cuda.synchronize()
    assert hmax is not None and H.shape[0] == ei.shape[1]
    eas = ea[csr.perm.long().cpu()].double()
    h1 = torch.relu(eas @ ws_[0].double().T + bs_[0].double())
    pre = h1 @ ws_[1].double().T + bs_[1].double()
    mag = h1 @ ws_[1].double().abs().T + bs_[1].double().abs()
    k2 = dims[2]
    Hc = H.cpu().double()
    err = ((Hc[:, :k2] - torch.relu(pre)).abs() / mag)
    assert err.max().item() <= TOL, (name, err.max().item())
    assert rel_l2(Hc[:, :k2], torch.relu(pre)) <= TOL
    assert hmax.item() == H.max().item(), (name, hmax.item(), H.max().item())


def test_store_variant_on_the_segment_graph():
    x, ei, ea, _, _ = _segment_graph()
    _hidden_check("segments", ei, ea, x.shape[0], [6, 256, 256, 4096], 1)


def test_store_variant_with_three_attribute_slots():
    x, ei, ea = _ragged_graph(90, 1503, 3, 63)
    _hidden_check("k0_3", ei, ea, 90, [3, 256, 256, 4096], 7)


def test_node_table_equals_tensor_bitwise_on_the_segment_graph():
    x, ei, ea, pos, a = _segment_graph()
    d = torch.device("cuda:0")
    ws_, bs_ = _mlp([6, 256, 256, 4096], 1)
    root, bias = _root_bias(3)
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    csr = ops.build_csr(ei.to(d), x.shape[0])
    na = gp.NodeAttr.darcy(pos.to(d), a.to(d))
    assert torch.equal(na.materialize(ei.to(d)).cpu(), ea)
    y_t = ops.nnconv_forward_raw(x.to(d), csr, ea.to(d), pm, root.to(d), bias.to(d), "mean", precision=V6)
    y_n = ops.nnconv_forward_nodeattr_raw(x.to(d), csr, na, pm, root.to(d), bias.to(d), "mean", precision=V6)
    torch.cuda.synchronize()
    assert torch.equal(y_t, y_n), rel_l2(y_n.cpu(), y_t.cpu())
