"""GPU tier: the tied accumulators of the image variant of the one-wave-per-SIMD fused kernel (csrc/gpde_fused_f16v6.hip,
gpde_fused_f16v6_kernel<0, ASRC_IMAGE>; DESIGN.md §3d, "Tied accumulators").  Its hidden-layer product MFMAs are asm
statements whose accumulator is C and D at once, and a tile's first product into each accumulator takes the constant 0
as C (nothing zeroes the accumulators any more).  The per-tile-prologue variant of the same library ("f16split_noimage",
or a workspace without the image) keeps builtin MFMAs and its zeroing, and receives the same products in the same order:
the two paths give the same bytes, and torch.equal between them is the test; the float64 oracle at the tier's 1e-5 comes
on top.

What the change can break, and the case that shows it:
  * a product left out of, or added twice to, an accumulator at some chunk count: k1 / 32 = 8, 10, 12 (the ring's three
    residues; at 8 every chunk but two is peeled) and 36 (the LDS limit), k2 = 128 (one column slice) and 256;
  * a stale accumulator (a first product that adds to what the tile before left): a wave that runs many consecutive
    tiles (rows of 2,048 and more in-edges), waves with one tile, fewer tiles than waves - the other waves of those
    workgroups run whole rounds without a tile beside waves that have one - and a block that ends inside a tile (63 and
    65 edges in the last row), under the block queue and under static ranges.  (A wave that has run out of tiles never
    draws a block again in this kernel: "no tile, then a tile" does not occur inside one launch, the next launch starts
    from fresh registers.)
  * an accumulator read before its last product has landed (the asm MFMAs carry no compiler-made wait states): rows of
    magnitude 1e-30 and 1e+30 and all-zero rows (with b1 = 0 the un-scaled edge, isc = 1) next to ordinary ones - a value
    read early is then wrong by orders of magnitude; three calls bitwise equal, and one under a 1 GiB fill on a second
    stream;
  * the un-scale, now without its zero writes, between the masks and flushes of half tiles that span several rows:
    in-degrees 5 - 40.
Every graph of the first three groups has just over 32,768 edges (the size from which the default precision takes this
kernel with the image); the one-tile cases are smaller by nature and force the kernel as tests/test_gpu_v6_resident.py does."""
import functools

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, rel_l2
from tests.helpers.magnitude_classes import class_rows
from tests.test_gpu_v6 import _mlp
from tests.test_gpu_v6_image import V6, _both, _route
from tests.test_gpu_v6_layout import _hidden_check, _root_bias, _segment_graph
from tests.test_gpu_v6_resident import _image_call, _rows_graph

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture
def static16(monkeypatch):
    """Static per-wave ranges on graphs below 32,768 edges (as in tests/test_gpu_v6_image.py)."""
    from graph_pde_amd import _lib
    monkeypatch.setitem(ops._PRECISION, "f16split_agg16_static", _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_AGG_F16 | _lib.GPDE_FWD_STATIC_RANGES)
    return "f16split_agg16_static"


def _fill_rows(total, lo, hi, g):
    """In-degrees drawn from lo .. hi that sum to `total` exactly."""
    rows = []
    while total > 0:
        k = min(int(torch.randint(lo, hi + 1, (1,), generator=g)), total)
        rows.append(k)
        total -= k
    return rows


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(x, edge_index, edge_attr); every graph has 32,768 + a few hundred edges."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name in ("long_rows_63", "long_rows_65"):
        # three rows of 2,048 - 2,600 in-edges among short ones (a wave walks 32 - 41 consecutive tiles of one row), the
        # last row of 63 / 65 edges: the last block ends one edge short of / one edge into a tile
        fill = _fill_rows(32768 + 300 - 2048 - 2300 - 2600, 5, 40, g)
        third = len(fill) // 3
        rows = fill[:third] + [2048] + fill[third:2 * third] + [2300, 2600] + fill[2 * third:] + [int(name[-2:])]
    elif name == "short_rows":
        rows = _fill_rows(32768 + 200, 5, 40, g)                   # every 32-edge half spans one to six rows
    else:
        raise KeyError(name)
    x, ei, ea = _rows_graph(rows, int(g.initial_seed()))
    assert 32768 < ei.shape[1] <= 33500
    return x, ei, ea


@functools.lru_cache(maxsize=None)
def _case(graph, k1, k2, attrs="randn", zero_b1=False):
    """Inputs and the float64 reference of a case: computed once, never modified."""
    x, ei, ea = _graph(graph)
    if attrs != "randn":
        # rows of four magnitude classes, neighbours in the edge list (and, the CSR order being a shuffle of it, mixed
        # inside every tile): 1e-30, ordinary, ordinary or 1e+30, all-zero
        g = torch.Generator().manual_seed(7)
        factors = {"small": (1e-30, 1.0, 1.0, 0.0), "huge": (1e-30, 1.0, 1e30, 0.0)}[attrs]
        ea = class_rows(torch.arange(ei.shape[1]) % 4, 6, factors, g)
    ws_, bs_ = _mlp([6, k1, k2, 4096], 71)
    if zero_b1:
        bs_ = [torch.zeros_like(bs_[0])] + list(bs_[1:])
    root, bias = _root_bias(72)
    y64 = None
    if attrs != "huge":
        y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    return x, ei, ea, ws_, bs_, root, bias, y64


def _check(case, prec, what, calls=3, no_image=False):
    """image path == prologue path bitwise; the float64 bar where the case has a reference (the "huge" rows leave the
    float range on either path: bit patterns only); `calls` calls of the image path bitwise equal."""
    x, ei, ea, ws_, bs_, root, bias, y64 = case
    y_i, y_p, dev = _both(x, ei, ea, ws_, bs_, root, bias, prec)      # asserts the kernel and which path took the image
    assert torch.equal(y_i.view(torch.int32), y_p.view(torch.int32)), (what, prec, rel_l2(y_i.cpu(), y_p.cpu()))
    if y64 is not None:
        err = rel_l2(y_i.cpu(), y64)
        print(f"{what} {prec}: image path rel-L2 vs float64 {err:.3e}")
        assert torch.isfinite(y_i).all() and err <= TOL, (what, prec, err)
    for rep in range(calls - 1):
        y_r = _image_call(dev, ei.shape[1], prec)
        assert torch.equal(y_r.view(torch.int32), y_i.view(torch.int32)), (what, prec, rep)
    if no_image:                                                       # the flag that forces the prologue at the full workspace
        xd, csr, ead, pm, rd, bd = dev
        r = _route(csr, pm, "f16split_noimage", ops.workspace_bytes(xd.shape[0], ei.shape[1], pm))
        assert r["kernel"] == "gpde_fused_f16v6_kernel" and r["attr_image"] is False, r
        y_f = ops.nnconv_forward_raw(xd, csr, ead, pm, rd, bd, "mean", precision="f16split_noimage")
        assert torch.equal(y_f.view(torch.int32), y_i.view(torch.int32)), (what, "f16split_noimage")
    return y_i, dev


@pytest.mark.parametrize("k1,k2", [(256, 256), (320, 256), (384, 256), (256, 128), (320, 128), (384, 128), (1152, 256)],
                         ids=lambda v: str(v))
def test_chunk_counts_and_column_slices(k1, k2):
    _check(_case("long_rows_63", k1, k2), "f16split", f"k1={k1} k2={k2}", no_image=True)


@pytest.mark.parametrize("prec", ["f16split", "f16split_static"], ids=["queue", "static"])
@pytest.mark.parametrize("graph", ["long_rows_63", "long_rows_65"])
def test_a_wave_that_runs_many_consecutive_tiles_and_a_block_that_ends_inside_a_tile(graph, prec):
    _check(_case(graph, 256, 256), prec, graph, no_image=prec == "f16split")


ONE_TILE = {
    "one_tile": [64],                          # one wave has one tile, every other wave of its workgroup none
    "three_tiles": [64, 64, 64],               # fewer tiles than waves: one tile each for three waves
    "last_63": [64, 64, 63],
    "last_65": [64, 64, 65],                   # a fourth tile of one edge
    "five_one_edge_rows_then_a_tile": [1, 1, 1, 1, 1, 59, 64],
}


@pytest.mark.parametrize("name", list(ONE_TILE))
def test_waves_with_one_tile_beside_waves_without(name, static16):
    x, ei, ea = _rows_graph(ONE_TILE[name], 5)
    ws_, bs_ = _mlp([6, 256, 256, 4096], 71)
    root, bias = _root_bias(72)
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    for prec in (V6, static16):                                        # queue blocks and static per-wave ranges
        _check((x, ei, ea, ws_, bs_, root, bias, y64), prec, name)


@pytest.mark.parametrize("attrs,zero_b1", [("small", False), ("small", True), ("huge", False)],
                         ids=["small", "small_b1_zero", "huge"])
@pytest.mark.parametrize("prec", ["f16split", "f16split_static"], ids=["queue", "static"])
def test_rows_of_extreme_magnitude_show_an_accumulator_read_too_early(attrs, zero_b1, prec):
    _check(_case("long_rows_63", 256, 256, attrs, zero_b1), prec, f"{attrs} b1=0:{zero_b1}")


def test_extreme_rows_are_reproducible_while_a_fill_runs_on_a_second_stream():
    """A 1 GiB fill on a second stream competes for memory bandwidth while the kernel runs: the ring pieces and staged
    rows land late, the barriers close late, and an accumulator is still read only behind its last product."""
    case = _case("long_rows_63", 256, 256, "small", True)
    y_i, dev = _check(case, "f16split", "small b1=0", calls=1)
    d = y_i.device
    junk = torch.empty(256 << 20, device=d)                            # 1 GiB
    side = torch.cuda.Stream(device=d)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        junk.fill_(0.5)
    y_r = _image_call(dev, case[1].shape[1], "f16split")               # synchronises the device: the fill has ended too
    assert torch.equal(y_r.view(torch.int32), y_i.view(torch.int32)), rel_l2(y_r.cpu(), y_i.cpu())


@pytest.mark.parametrize("prec", ["f16split", "f16split_static"], ids=["queue", "static"])
def test_half_tiles_that_span_several_rows(prec):
    x, ei, ea, ws_, bs_, root, bias, y64 = case = _case("short_rows", 256, 256)
    y_i, _ = _check(case, prec, "short_rows", no_image=prec == "f16split")
    # every output row on its own (an edge un-scaled with its neighbour's factor, or flushed into the wrong row, moves one
    # row): error relative to the row's norm, floored by the median row norm
    nr = y64.norm(dim=1)
    err = (y_i.cpu().double() - y64).norm(dim=1) / torch.maximum(nr, nr.median())
    assert err.max().item() <= TOL, (int(err.argmax()), err.max().item())


def test_node_table_attributes_equal_tensor_attributes_bitwise():
    x, ei, ea, pos, a = _segment_graph()
    d = torch.device("cuda:0")
    ws_, bs_ = _mlp([6, 256, 256, 4096], 1)
    root, bias = _root_bias(3)
    na = gp.NodeAttr.darcy(pos.to(d), a.to(d))
    assert torch.equal(na.materialize(ei.to(d)).cpu(), ea)
    y_t, y_tp, _ = _both(x, ei, ea, ws_, bs_, root, bias, V6)
    y_n, y_np, _ = _both(x, ei, ea, ws_, bs_, root, bias, V6, na=na)
    assert torch.equal(y_t, y_tp) and torch.equal(y_n, y_np)
    assert torch.equal(y_t, y_n), rel_l2(y_n.cpu(), y_t.cpu())
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    assert rel_l2(y_n.cpu(), y64) <= TOL


def test_store_variant_is_unchanged_against_the_oracle():
    """gpde_hidden_fwd (the <1, tensor> instantiation: builtin MFMAs, its own epilogue) on a graph of this file."""
    x, ei, ea = _graph("long_rows_63")
    _hidden_check("long_rows_63", ei, ea, x.shape[0], [6, 256, 256, 4096], 71)
