"""GPU tier: the resident W2 fragment sets of the image variant of the one-wave-per-SIMD fused kernel
(csrc/gpde_fused_f16v6.hip, gpde_fused_f16v6_kernel<0, ASRC_IMAGE>).  The image variant keeps four fragment sets and reads
every W2 fragment from the LDS ring once per chunk, the next chunk's sets from the next ring slot while the current chunk
still runs; the per-tile-prologue variant of the same library keeps two sets and the schedule of before.  MFMA order and
operands are the same, so the two paths give the same bytes (tests/test_gpu_v6_image.py compares them on its own cases).
What a resident set can break is a set read from a slot whose pieces have not landed or that is already being refilled
(the three ring residues, the longest ring walk), a set carried into a chunk it does not belong to (the tile's first and
last chunk, a wave's first tile, a tile without a successor) and the column slice's base.  W2 is random in every case, so
every (chunk, column block) fragment is distinct.  Every case: image path == prologue path bitwise, rel-L2 against the
float64 oracle within the tier's 1e-5, and three calls of the image path bitwise equal (a set read before its slot
landed differs from run to run)."""
import functools

import pytest
import torch

from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, rel_l2
from tests.test_gpu_v6 import _graph, _mlp
from tests.test_gpu_v6_image import V6, _both, _boundary_graph, _image_bytes, _route
from tests.test_gpu_v6_layout import _root_bias

pytestmark = pytest.mark.gpu
TOL = 1e-5

SHAPES = {
    # name: dims, n, e - graphs of 32,768 - 40,000 edges: the default precision takes this kernel with the image
    "chunks8": ([6, 256, 256, 4096], 700, 36000),        # k1 / 32 = 8, 10, 12: the three ring residues
    "chunks10": ([6, 320, 256, 4096], 900, 38000),
    "chunks12": ([6, 384, 256, 4096], 800, 35000),
    "chunks36": ([6, 1152, 256, 4096], 600, 33000),      # the image variant's largest k1: LDS at its limit
    "one_slice": ([6, 256, 128, 4096], 650, 34000),      # k2 = 128: one column slice
    "ragged_slices": ([6, 256, 200, 4096], 750, 37000),  # k2 = 200: two slices, the second ragged
    "eight_slices": ([6, 256, 1024, 4096], 500, 32768),  # k2 = 1024
}


@pytest.fixture
def static16(monkeypatch):
    """Static per-wave ranges on graphs below 32,768 edges (as in tests/test_gpu_v6_image.py)."""
    from graph_pde_amd import _lib
    monkeypatch.setitem(ops._PRECISION, "f16split_agg16_static", _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_AGG_F16 | _lib.GPDE_FWD_STATIC_RANGES)
    return "f16split_agg16_static"


@functools.lru_cache(maxsize=None)
def _shape_case(name):
    """Inputs and the float64 reference of a case: computed once, never modified."""
    dims, n, e = SHAPES[name]
    ws_, bs_ = _mlp(dims, 51)
    x, ei, ea = _graph(n, e, dims[0], 52, skew=True)
    root, bias = _root_bias(53)
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    return x, ei, ea, ws_, bs_, root, bias, y64


def _image_call(dev_inputs, e, prec):
    """The image path again, on the device inputs _both returned (its workspace rule)."""
    xd, csr, ead, pm, rd, bd = dev_inputs
    nbytes = ops.workspace_bytes(xd.shape[0], e, pm) + (0 if e >= 32768 else _image_bytes(e))
    assert _route(csr, pm, prec, nbytes)["attr_image"] is True
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
    y = ops.nnconv_forward_raw(xd, csr, ead, pm, rd, bd, "mean", ws=ws, precision=prec)
    torch.cuda.synchronize()
    return y


def _check(x, ei, ea, ws_, bs_, root, bias, y64, prec, what):
    y_i, y_p, dev = _both(x, ei, ea, ws_, bs_, root, bias, prec)       # asserts the kernel and which path took the image
    assert torch.equal(y_i, y_p), (what, prec, rel_l2(y_i.cpu(), y_p.cpu()))
    err = rel_l2(y_i.cpu(), y64)
    print(f"{what} {prec}: image path rel-L2 vs float64 {err:.3e}")
    assert torch.isfinite(y_i).all() and err <= TOL, (what, prec, err)
    for rep in range(2):                                               # with y_i: three calls of the image path
        y_r = _image_call(dev, ei.shape[1], prec)
        assert torch.equal(y_r, y_i), (what, prec, rep, rel_l2(y_r.cpu(), y_i.cpu()))
    return y_i, dev


@pytest.mark.parametrize("name", list(SHAPES))
def test_chunk_counts_and_column_slices(name):
    x, ei, ea, ws_, bs_, root, bias, y64 = _shape_case(name)
    assert 32768 <= ei.shape[1] <= 40000
    _check(x, ei, ea, ws_, bs_, root, bias, y64, "f16split", name)


def test_the_forward_entry_gives_this_kernel_no_odd_chunk_count():
    """Nine chunks (k1 = 288): the forward entry asks for the 8-wave kernel's support first, which wants an even chunk count,
    so the resident sets never run at an odd one - asserted, not assumed."""
    d = torch.device("cuda:0")
    ws_, bs_ = _mlp([6, 288, 256, 4096], 51)
    pm = ops.pack_mlp([w.to(d) for w in ws_], [b.to(d) for b in bs_])
    for prec in ("f16split", V6):
        assert ops.fused_kernel_name(800, 34000, pm, prec) != "gpde_fused_f16v6_kernel"


def _rows_graph(rows, seed):
    """Destination rows of the given in-degrees, in order (node-aligned ranges and blocks then hold whole rows)."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor(rows)
    n, e = deg.numel() + 2, int(deg.sum())
    dst = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    src = torch.randint(0, n, (e,), generator=g)
    p = torch.randperm(e, generator=g)
    return torch.randn(n, 64, generator=g), torch.stack([src[p], dst[p]]), torch.randn(e, 6, generator=g)


TILES = {
    # a wave's first tile forms its own operands and reads its own sets (cold start); a tile without a successor reads none
    "one_tile": lambda: _rows_graph([64], 1),                        # cold start, then the last chunk with no next tile
    "two_tiles": lambda: _rows_graph([128], 2),                      # one row: one wave owns both tiles in either mode
    "three_tiles": lambda: _rows_graph([64, 64, 64], 3),             # fewer tiles than waves
    "partial_tiles": lambda: _rows_graph([70, 5, 100], 4),
    "blocks_end_inside_tiles": lambda: _boundary_graph(64 * 70 + 13, 4130, 5),
}


@pytest.mark.parametrize("name", list(TILES))
def test_tiles_per_wave(name, static16):
    x, ei, ea = TILES[name]()
    ws_, bs_ = _mlp([6, 256, 256, 4096], 61)
    root, bias = _root_bias(62)
    y64 = nnconv_forward(x, ei, ea, ws_, bs_, root, bias, aggr="mean", dtype=torch.float64)
    for prec in (V6, static16):                                        # queue blocks and static per-wave ranges
        _check(x, ei, ea, ws_, bs_, root, bias, y64, prec, name)


def test_image_path_is_reproducible_while_a_fill_runs_on_a_second_stream():
    """A 1 GiB fill on a second stream competes for memory bandwidth while the kernel runs: a ring piece that lands late must
    still be waited for before its set is read."""
    x, ei, ea, ws_, bs_, root, bias, y64 = _shape_case("chunks12")
    y_i, dev = _check(x, ei, ea, ws_, bs_, root, bias, y64, "f16split", "chunks12")
    d = y_i.device
    junk = torch.empty(256 << 20, device=d)                            # 1 GiB
    side = torch.cuda.Stream(device=d)
    torch.cuda.synchronize()
    for val in (0.5, float("nan"), -3.0e38):
        with torch.cuda.stream(side):
            junk.fill_(val)
        y_r = _image_call(dev, ei.shape[1], "f16split")                # synchronises the device: the fill has ended too
        assert torch.equal(y_r, y_i), (val, rel_l2(y_r.cpu(), y_i.cpu()))
