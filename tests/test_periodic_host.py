"""CPU tier: the host side of the periodic (torus) radius graphs - argument validation of the three gpde_radius_csr_periodic_*
entry points before any device call, the workspace query, the ValueErrors of the `period=` keywords of ops, and the fairness of
the inputs the GPU tier runs (tests/helpers/periodic_oracle.py).  Needs libgpde.so, no device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from graph_pde_amd import _lib, ops
from tests.helpers import periodic_oracle as po

EINVAL = -1
D2 = ctypes.c_double * 2
LO, HI, ORG, PER = D2(0.0, 0.0), D2(1.0, 1.0), D2(0.0, 0.0), D2(1.0, 1.0)
BUF = ctypes.create_string_buffer(256)        # stands for every device pointer: validation must return before any is read

# (dim, r, flags, origin, period): each invalid argument of the issue's list, one at a time
INVALID = {
    "dim 0": (0, 0.1, 0, ORG, PER),
    "dim 4": (4, 0.1, 0, ORG, PER),
    "negative period": (2, 0.1, 0, ORG, D2(1.0, -1.0)),
    "2r == period": (2, 0.5, 0, ORG, PER),
    "2r > period": (2, 0.3, 0, ORG, D2(1.0, 0.5)),
    "r == 0": (2, 0.0, 0, ORG, PER),
    "r < 0": (2, -0.1, 0, ORG, PER),
    "reference ties": (2, 0.1, 1, ORG, PER),
}


def _count(dim, r, flags, org, per):
    return _lib.lib().gpde_radius_csr_periodic_count(BUF, 5, BUF, 5, dim, r, flags, LO, HI, org, per, BUF, BUF, 1 << 20, None)


def _fill(dim, r, flags, org, per, geom=None):
    return _lib.lib().gpde_radius_csr_periodic_fill(BUF, 5, BUF, 5, dim, r, flags, LO, HI, org, per, BUF, BUF, BUF, geom, 3, BUF, 1 << 20, None)


def _ws(n, dim, r, org, per, lo=LO, hi=HI):
    return int(_lib.lib().gpde_radius_csr_periodic_workspace_bytes(n, dim, r, lo, hi, org, per))


@pytest.mark.parametrize("what", sorted(INVALID))
def test_entry_points_reject_invalid_arguments_before_any_device_call(what):
    dim, r, flags, org, per = INVALID[what]
    assert _count(dim, r, flags, org, per) == EINVAL, what
    assert _lib.lib().gpde_last_error() != b""
    assert _fill(dim, r, flags, org, per) == EINVAL, what
    assert _fill(dim, r, flags, org, per, geom=BUF) == EINVAL, what
    if flags == 0:                                    # the query takes no flags: it sees every other argument
        assert _ws(5, dim, r, org, per) == 0, what
        assert _lib.lib().gpde_last_error() != b""


def test_error_messages_name_the_argument():
    l = _lib.lib()
    assert _count(*INVALID["2r == period"]) == EINVAL and b"period[0]" in l.gpde_last_error()
    assert _count(*INVALID["reference ties"]) == EINVAL and b"REFERENCE_TIES" in l.gpde_last_error()
    assert _count(*INVALID["dim 4"]) == EINVAL and b"dim" in l.gpde_last_error()
    assert l.gpde_radius_csr_periodic_count(BUF, 5, BUF, 5, 2, 0.1, 0, LO, HI, None, PER, BUF, BUF, 1 << 20, None) == EINVAL      # no origin
    assert l.gpde_radius_csr_periodic_count(None, 5, BUF, 5, 2, 0.1, 0, LO, HI, ORG, PER, BUF, BUF, 1 << 20, None) == EINVAL     # no positions
    assert l.gpde_radius_csr_periodic_count(BUF, 5, BUF, 5, 2, 0.1, 0, None, None, ORG, D2(1.0, 0.0), BUF, BUF, 1 << 20, None) == EINVAL   # open axis, no bounds
    assert b"lo / hi" in l.gpde_last_error()
    assert l.gpde_radius_csr_periodic_count(BUF, 5, BUF, 5, 2, 0.1, 0, LO, HI, ORG, PER, BUF, BUF, 16, None) == -3                # workspace too small


def test_workspace_query():
    sizes = [_ws(n, 2, 0.1, ORG, PER) for n in (0, 1, 10, 1000, 58081, 1 << 20)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]      # monotone in n
    # the reduced source positions are kept next to the open builder's cell structure
    assert sizes[4] >= 58081 * (4 * 4 + 2 * 8)
    assert _ws(1000, 2, 0.1, ORG, PER, lo=None, hi=None) == sizes[3] > 0                     # bounds are read on open axes only
    assert _ws(1000, 2, 0.1, ORG, D2(1.0, 0.0), lo=None, hi=None) == 0
    assert _ws(1000, 2, 0.1, ORG, D2(1.0, 0.0)) > 0                                          # a mixed box
    assert 0 < _ws(10, 2, 1e-9, ORG, PER) < (1 << 28)                                        # an absurdly fine grid is coarsened
    assert _ws(-1, 2, 0.1, ORG, PER) == 0


def test_header_declares_the_additions():
    protos = _lib.header_prototypes()
    for twin in ("workspace_bytes", "count", "fill"):
        new, old = protos[f"gpde_radius_csr_periodic_{twin}"][1], protos[f"gpde_radius_csr_{twin}"][1]
        assert len(new) == len(old) + (3 if twin == "fill" else 2), twin                     # + origin, period (+ geom)
        assert new.count("const double*") == old.count("const double*") + 2
    assert "float*" in protos["gpde_radius_csr_periodic_fill"][1]
    assert _lib.lib().gpde_version() == _lib.GPDE_VERSION == 101                             # additions leave the version alone


def test_ops_refuses_on_the_host():
    pos = torch.rand(20, 2, dtype=torch.float64)                  # CPU tensors: every refusal below comes before the device is asked for
    for fn in (ops.radius_csr_raw, ops.radius_csr, ops.radius_in_degrees, ops.radius_graph):
        with pytest.raises(ValueError, match="ALIAS of the grid"):
            fn(pos, 0.1, reference_ties=True, period=1.0)
        with pytest.raises(ValueError, match=r"2 r = 1\.0 >= period\[1\]"):
            fn(pos, 0.5, period=(2.0, 1.0))
        with pytest.raises(ValueError, match="3 entries for positions of dimension 2"):
            fn(pos, 0.1, period=(1.0, 1.0, 1.0))
        with pytest.raises(ValueError, match="origin has 1 entries"):
            fn(pos, 0.1, period=1.0, origin=[0.0])
        with pytest.raises(ValueError, match="must be >= 0"):
            fn(pos, 0.1, period=(1.0, -1.0))
    with pytest.raises(ValueError, match="ALIAS of the grid"):
        ops.multilevel_radius_graphs([pos, pos[:5]], [0.1, 0.1], [0.1], reference_ties=True, period=1.0)
    with pytest.raises(ValueError, match="reference_ties must be False"):
        ops.radius_csr(pos, 0.1, reference_ties=True, return_geometry=True)
    with pytest.raises(RuntimeError, match="pos is on cpu"):      # a valid periodic call on CPU tensors gets as far as the device check
        ops.radius_csr(pos, 0.1, period=1.0)


def test_period_and_origin_spellings():
    assert ops.periodic_box(2.0, None, 3, 0.5) == ([2.0, 2.0, 2.0], [0.0, 0.0, 0.0])
    assert ops.periodic_box((1.0, None, 0), (-0.3, 0.7, None), 3, 0.2) == ([1.0, 0.0, 0.0], [-0.3, 0.7, 0.0])
    assert ops.periodic_box(torch.tensor([1.0, 2.0]), 0.5, 2, 0.2) == ([1.0, 2.0], [0.5, 0.5])
    assert ops.periodic_box(0, None, 1, 5.0) == ([0.0], [0.0])                 # every axis open: no bound on r
    for fn in (ops.radius_csr_raw, ops.radius_csr, ops.radius_in_degrees, ops.radius_graph, ops.multilevel_radius_graphs):
        p = inspect.signature(fn).parameters
        assert p["period"].default is None and p["origin"].default is None, fn.__name__
    assert inspect.signature(ops.radius_csr).parameters["return_geometry"].default is False


@pytest.mark.parametrize("name", sorted(po.CASES))
def test_gpu_tier_inputs_are_fair(name):
    """No pair of any input of the GPU tier lies within 1e-12 r^2 of the threshold (periodic_edges asserts it), 2 r < period, and the
    case exercises what it is there for."""
    c = po.CASES[name]()
    ei, disp, norm = po.periodic_edges(c["xs"], c["r"], c["period"], xd=c.get("xd"))
    assert ei.shape[0] == 2 and disp.shape == (ei.shape[1], np.asarray(c["xs"]).shape[1]) and (norm <= c["r"]).all()
    L = po.per_axis(c["period"], disp.shape[1])
    if name != "1d_one_point":
        wrapped = np.abs(c["xs"][ei[0]] - (c["xs"] if "xd" not in c else c["xd"])[ei[1]] - disp).max(axis=0)
        assert (wrapped[L > 0] > 0.5 * L[L > 0]).all(), "no edge crosses the seam"
    if name.startswith("2d_nc"):
        assert int(np.floor(1.0 / c["r"])) == int(name[5:])
    if name == "long_row":
        assert (np.bincount(ei[1], minlength=3) == 5000).all()


def test_the_lattice_inputs_are_fair():
    lat = po.lattice16()
    ei, disp, _ = po.periodic_edges(lat, 0.2, 1.0)
    assert ei.shape[1] == 256 * 37                                 # a^2 + b^2 <= 10.24 lattice steps: 37 offsets, every node alike
    assert np.array_equal(disp * 16.0, np.round(disp * 16.0))     # dyadic: exact
    levels, radii_inner, radii_inter = po.nested_levels_1d()
    for p, r in zip(levels, radii_inner):
        po.periodic_edges(p, r, 1.0)
    for l, r in enumerate(radii_inter):
        po.periodic_edges(levels[l], r, 1.0, xd=levels[l + 1])
    box = 0.25 + 0.5 * np.random.default_rng(31).random((200, 2))
    assert np.array_equal(po.periodic_edges(box, 0.2, 4.0)[0], po.periodic_edges(box, 0.2, 0.0)[0])
