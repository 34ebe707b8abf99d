"""GPU tier: the attribute operand image of the one-wave-per-SIMD fused kernel (csrc/gpde_prep.hip k_attr_image,
gpde_fused_f16v6_kernel<0, ASRC_IMAGE>).  The image variant fetches per tile what the other variants form in their tile
prologue, and produces the next tile's first H1 and operands in its last chunk; every accumulator receives the same
products in the same order, so its output is the other path's byte for byte.  Which path runs is a matter of the
workspace: with the image's bytes (ops.workspace_bytes counts them from 32,768 edges on) the plan takes the image,
without them - or under "f16split_noimage" - it is the plan and the kernel of before.  What can go wrong is a tile
boundary (a block that ends inside a tile, a next tile in another block, no next tile, a wave's first tile), a staged
row read before its DMA has landed, the bias slot's position, and the un-scale of edges whose bound leaves the
exponent range."""
import functools

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, rel_l2
from tests.test_gpu_repeat import _repeat
from tests.test_gpu_v6 import _graph, _mlp
from tests.test_gpu_v6_kloop import CASES
from tests.test_gpu_v6_layout import _ragged_graph, _root_bias, _segment_graph

pytestmark = pytest.mark.gpu
TOL = 1e-5
V6 = "f16split_agg16"
FORWARD_CASES = ["chunks8", "chunks10", "chunks12", "chunks32", "tiny12"]       # the CASES that reach the forward entry


def _image_bytes(e):
    """The image's part of the workspace: constant record, hi plane, lo plane, isc - each aligned to 256 bytes."""
    al = lambda v: (v + 255) // 256 * 256
    return 256 + 2 * al(16 * e) + al(4 * e)


@pytest.fixture
def static16(monkeypatch):
    """Static per-wave ranges on graphs below 32,768 edges: the two flags together have no name of their own."""
    from graph_pde_amd import _lib
    monkeypatch.setitem(ops._PRECISION, "f16split_agg16_static", _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_AGG_F16 | _lib.GPDE_FWD_STATIC_RANGES)
    return "f16split_agg16_static"


def _route(csr, pm, prec, ws_bytes):
    """ops.forward_route of the raw forward call: NNConvFunction sends graphs of low mean in-degree to another operator
    altogether (route "per_edge"); ops.nnconv_forward_raw, which runs here, does not - then the library's queries directly."""
    r = ops.forward_route(csr, pm, "mean", precision=prec, ws_bytes=ws_bytes)
    if r["association"] == "node":
        return r
    import ctypes
    from graph_pde_amd import _lib
    nch = ctypes.c_int32()
    img = _lib.lib().gpde_nnconv_fwd_attr_image(csr.n_nodes, csr.n_edges, len(pm.dims) - 1, pm.dims_c, ops._PRECISION[prec], ws_bytes,
                                                ctypes.byref(nch))
    assert img >= 0, img
    return {"kernel": ops.fused_kernel_name(csr.n_nodes, csr.n_edges, pm, prec), "attr_image": img == 1, "n_chunks": nch.value}


def _both(x, ei, ea, ws_, bs_, root, bias, prec, na=None):
    """The forward on the image path and on the per-tile prologue, told apart by the workspace alone (same flags, same
    plan otherwise); returns (y_image, y_prologue, device inputs)."""
    d = torch.device("cuda:0")
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    n, e = x.shape[0], ei.shape[1]
    csr = ops.build_csr(ei.to(d), n)
    base = ops.workspace_bytes(n, e, pm) - (_image_bytes(e) if e >= 32768 else 0)     # the workspace without the image
    r_img = _route(csr, pm, prec, base + _image_bytes(e))
    r_pro = _route(csr, pm, prec, base)
    assert r_img["kernel"] == r_pro["kernel"] == "gpde_fused_f16v6_kernel", (r_img, r_pro)
    assert r_img["attr_image"] is True and r_pro["attr_image"] is False, (r_img, r_pro)
    assert r_img["n_chunks"] == r_pro["n_chunks"] == 1
    xd, ead = x.to(d), ea.to(d)
    rd, bd = (None if root is None else root.to(d)), (None if bias is None else bias.to(d))
    out = []
    for nbytes in (base + _image_bytes(e), base):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
        if na is None:
            out.append(ops.nnconv_forward_raw(xd, csr, ead, pm, rd, bd, "mean", ws=ws, precision=prec))
        else:
            out.append(ops.nnconv_forward_nodeattr_raw(xd, csr, na, pm, rd, bd, "mean", ws=ws, precision=prec))
    torch.cuda.synchronize()
    return out[0], out[1], (xd, csr, ead, pm, rd, bd)


@functools.lru_cache(maxsize=None)
def _case(name):
    dims, n, e, prec = CASES[name]
    ws_, bs_ = _mlp(dims, 11)
    x, ei, ea = _graph(n, e, dims[0], 12, skew=True)
    root, bias = _root_bias(13)
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    return prec, x, ei, ea, ws_, bs_, root, bias, y64


@pytest.mark.parametrize("static", [False, True], ids=["queue", "static"])
@pytest.mark.parametrize("name", FORWARD_CASES)
def test_image_path_equals_prologue_path_bitwise_and_meets_the_float64_bar(name, static, static16):
    prec, x, ei, ea, ws_, bs_, root, bias, y64 = _case(name)
    if static:
        prec = static16 if prec == V6 else "f16split_static"
    y_i, y_p, (xd, csr, ead, pm, rd, bd) = _both(x, ei, ea, ws_, bs_, root, bias, prec)
    assert torch.equal(y_i, y_p), (name, prec, rel_l2(y_i.cpu(), y_p.cpu()))
    err = rel_l2(y_i.cpu(), y64)
    print(f"{name} {prec}: image path rel-L2 vs float64 {err:.3e}")
    assert torch.isfinite(y_i).all() and err <= TOL, (name, prec, err)
    if prec == "f16split":
        # the flag that forces the per-tile prologue at the full workspace
        assert ops.forward_route(csr, pm, "mean", precision="f16split_noimage")["attr_image"] is False
        y_f = ops.nnconv_forward_raw(xd, csr, ead, pm, rd, bd, "mean", precision="f16split_noimage")
        assert torch.equal(y_i, y_f), (name, rel_l2(y_i.cpu(), y_f.cpu()))


def _boundary_graph(e, big, seed):
    """`e` edges on rows of in-degree 1 - 3 and, if `big`, one row of `big` in-edges in their middle: node-aligned queue
    blocks then end anywhere inside a 64-edge tile, and a wave's next tile starts in another block.  (More than four edges
    per node on average: with fewer, and 4096 edges or more, the library takes the per-edge last layer, not this kernel.)"""
    g = torch.Generator().manual_seed(seed)
    deg, left = [], e - big
    while left > 0:
        k = min(int(torch.randint(1, 4, (1,), generator=g)), left)
        deg.append(k)
        left -= k
    if big:
        deg.insert(len(deg) // 2, big)
    deg = torch.tensor(deg)
    n = deg.numel() + 3                                              # three rows without in-edges at the end
    dst = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    src = torch.randint(0, n, (e,), generator=g)
    p = torch.randperm(e, generator=g)
    return torch.randn(n, 64, generator=g), torch.stack([src[p], dst[p]]), torch.randn(e, 6, generator=g)


@pytest.mark.parametrize("e,big", [(64 * 120 + 1, 4200), (65, 0), (63, 0), (150, 70)],
                         ids=["E7681_long_row", "E65", "E63", "fewer_tiles_than_waves"])
def test_tile_boundaries(e, big, static16):
    x, ei, ea = _boundary_graph(e, big, 100 + e)
    assert ei.shape[1] == e
    ws_, bs_ = _mlp([6, 256, 256, 4096], 21)
    root, bias = _root_bias(22)
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    for prec in (V6, static16):
        y_i, y_p, _ = _both(x, ei, ea, ws_, bs_, root, bias, prec)
        assert torch.equal(y_i, y_p), (e, prec, rel_l2(y_i.cpu(), y_p.cpu()))
        assert rel_l2(y_i.cpu(), y64) <= TOL, (e, prec, rel_l2(y_i.cpu(), y64))


@pytest.mark.parametrize("k0", [1, 3, 6, 7])
def test_bias_slot_position(k0):
    x, ei, ea = _ragged_graph(90, 1500 + k0, k0, 60 + k0)
    ws_, bs_ = _mlp([k0, 256, 256, 4096], 7)
    root, bias = _root_bias(9)
    y_i, y_p, _ = _both(x, ei, ea, ws_, bs_, root, bias, V6)
    assert torch.equal(y_i, y_p), (k0, rel_l2(y_i.cpu(), y_p.cpu()))
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    assert rel_l2(y_i.cpu(), y64) <= TOL, (k0, rel_l2(y_i.cpu(), y64))


@pytest.mark.parametrize("huge,zero_b1", [(False, False), (False, True), (True, False)], ids=["small_b1", "small_b1_zero", "huge"])
def test_attribute_rows_of_extreme_magnitude_inside_one_tile(huge, zero_b1):
    """Rows of magnitude 1e-30 and all-zero rows among ordinary ones, within one 64-edge tile; with b1 = 0 the bound of an
    all-zero row is 0: the branch that leaves the edge unscaled (isc = 1).  "huge" adds rows of magnitude 1e+30: the hidden
    layer's global scale then leaves the float range on either path (zeros and non-finite values), so that case compares
    the two paths' bit patterns and nothing else."""
    x, ei, ea = _ragged_graph(40, 300, 6, 77)
    ea = ea.clone()
    ea[5:9] *= 1e-30
    ea[40:44] = 0.0
    ea[64 + 7] = 0.0
    if huge:
        ea[20:23] *= 1e30
    ws_, bs_ = _mlp([6, 256, 256, 4096], 31)
    if zero_b1:
        bs_ = [torch.zeros_like(bs_[0])] + list(bs_[1:])
    y_i, y_p, _ = _both(x, ei, ea, ws_, bs_, None, None, V6)
    assert torch.equal(y_i.view(torch.int32), y_p.view(torch.int32))
    if not huge:
        y64 = nnconv_forward(x, ei, ea, ws_, bs_, None, None, aggr="mean", dtype=torch.float64)
        assert torch.isfinite(y_i).all() and rel_l2(y_i.cpu(), y64) <= TOL, rel_l2(y_i.cpu(), y64)


def test_node_table_equals_tensor_bitwise_through_the_image():
    x, ei, ea, pos, a = _segment_graph()
    d = torch.device("cuda:0")
    ws_, bs_ = _mlp([6, 384, 256, 4096], 1)
    root, bias = _root_bias(3)
    na = gp.NodeAttr.darcy(pos.to(d), a.to(d))
    assert torch.equal(na.materialize(ei.to(d)).cpu(), ea)
    y_t, y_tp, _ = _both(x, ei, ea, ws_, bs_, root, bias, V6)
    y_n, y_np, _ = _both(x, ei, ea, ws_, bs_, root, bias, V6, na=na)
    assert torch.equal(y_t, y_tp) and torch.equal(y_n, y_np)
    assert torch.equal(y_t, y_n), rel_l2(y_n.cpu(), y_t.cpu())
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    assert rel_l2(y_n.cpu(), y64) <= TOL


def test_reduced_workspace_runs_without_the_image_and_gives_the_same_bytes():
    """A workspace for 2/5 of the nodes' Z: the plan drops the image and chunks the nodes.  Every row has 64 in-edges, so
    every chunk and every queue block starts on a tile boundary of the one-chunk run and the two runs form the same tiles:
    the same bytes (on a ragged graph chunking moves the tile alignment, tests/test_gpu_v6.py)."""
    g = torch.Generator().manual_seed(5)
    n, deg = 640, 64
    dst = torch.repeat_interleave(torch.arange(n), deg)
    e = dst.numel()
    p = torch.randperm(e, generator=g)
    ei = torch.stack([torch.randint(0, n, (e,), generator=g)[p], dst[p]])
    ea, x = torch.randn(e, 6, generator=g), torch.randn(n, 64, generator=g)
    dims = [6, 256, 256, 4096]
    ws_, bs_ = _mlp(dims, 41)
    root, bias = _root_bias(42)
    d = torch.device("cuda:0")
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    csr = ops.build_csr(ei.to(d), n)
    full = ops.workspace_bytes(n, e, pm)
    small = full - (n - n * 2 // 5) * 64 * ops.hidden_width(pm.dims) * 4
    r_full = ops.forward_route(csr, pm, "mean", precision="f16split", ws_bytes=full)
    r_small = ops.forward_route(csr, pm, "mean", precision="f16split", ws_bytes=small)
    assert r_full["attr_image"] is True and r_full["n_chunks"] == 1, r_full
    assert r_small["attr_image"] is False and r_small["n_chunks"] >= 2, r_small
    assert ops.launch_plan(n, e, pm, small)["n_chunks"] == r_small["n_chunks"]
    args = (x.to(d), csr, ea.to(d), pm, root.to(d), bias.to(d), "mean")
    y_full = ops.nnconv_forward_raw(*args, ws=torch.empty(full, dtype=torch.uint8, device=d), precision="f16split")
    y_small = ops.nnconv_forward_raw(*args, ws=torch.empty(small, dtype=torch.uint8, device=d), precision="f16split")
    torch.cuda.synchronize()
    assert torch.equal(y_full, y_small), rel_l2(y_small.cpu(), y_full.cpu())


@pytest.mark.parametrize("name", ["chunks8", "chunks32"])
def test_image_path_is_reproducible_under_memory_pressure(name):
    """A staged image row or isc read before its DMA has landed shows as a result that differs from the first call."""
    prec, x, ei, ea, ws_, bs_, root, bias, _ = _case(name)
    d = torch.device("cuda:0")
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    n, e = x.shape[0], ei.shape[1]
    csr = ops.build_csr(ei.to(d), n)
    nbytes = ops.workspace_bytes(n, e, pm) + (0 if e >= 32768 else _image_bytes(e))
    assert ops.forward_route(csr, pm, "mean", precision=prec, ws_bytes=nbytes)["attr_image"] is True
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    xd, ead, rd, bd = x.to(d), ea.to(d), root.to(d), bias.to(d)
    _repeat(lambda: ops.nnconv_forward_raw(xd, csr, ead, pm, rd, bd, "mean", ws=ws, precision=prec), d, 20)
