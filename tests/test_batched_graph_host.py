"""CPU tier: the host side of the batched radius graphs - every ValueError of ops.radius_csr_batched / radius_graph_batched on
CPU tensors before the device is asked for, ops.ptr_from_batch, the host-only planning entry point
(gpde_radius_csr_batched_plan: per-graph grids, cell bases, the cap), the refusals of the three entry points, and the
concatenate-and-offset assembly the GPU tier compares against (tests/helpers/batched_graphs.py), pinned on the oracle and the
reference generator's own graphs.  Needs libgpde.so, no device."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from graph_pde_amd import _lib, ops, synth
from oracle import radius_oracle
from tests.conftest import GOLDEN
from tests.helpers import batched_graphs as bg

EINVAL, EWORKSPACE = -1, -3
BUF = ctypes.create_string_buffer(4096)       # stands for every device pointer: validation must return before any is read
REC = np.dtype([("lo", "<f8", 3), ("inv", "<f8", 3), ("r2", "<f8"), ("d2_max", "<f8"), ("nc", "<i4", 3), ("cell_base", "<i4"),
                ("src_begin", "<i4"), ("src_end", "<i4"), ("dst_begin", "<i4"), ("dst_end", "<i4")])
CAP = 1 << 24


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _f64(*v):
    return (ctypes.c_double * len(v))(*v)


def _plan(bounds, ptr, radii, dim, ptr_dst=None, want_table=True):
    """(rc, records, n_cells, ws_bytes) of gpde_radius_csr_batched_plan on plain host arrays."""
    b = len(ptr) - 1
    bounds = np.ascontiguousarray(bounds, dtype=np.float64)
    table = np.zeros(max(b, 1), dtype=REC)
    n_cells, ws = ctypes.c_int64(-1), ctypes.c_size_t(0)
    rc = _lib.lib().gpde_radius_csr_batched_plan(bounds.ctypes.data if bounds.size else None, _i64(*ptr), None if ptr_dst is None else _i64(*ptr_dst),
                                                 _f64(*radii) if len(radii) else None, b, dim, table.ctypes.data if want_table else None,
                                                 ctypes.byref(n_cells), ctypes.byref(ws))
    return rc, table[:b], int(n_cells.value), int(ws.value)


def test_record_size_and_version():
    assert REC.itemsize == _lib.GPDE_RADIUS_BATCHED_REC_BYTES == 96
    header = open(_lib.HEADER_PATH).read()
    assert "GPDE_RADIUS_BATCHED_REC_BYTES = 96" in header
    assert "#define GPDE_VERSION 101" in " ".join(header.split())          # entry points are only added
    assert _lib.lib().gpde_version() == _lib.GPDE_VERSION == 101
    protos = _lib.header_prototypes()
    for name in ("plan", "count", "fill"):
        assert f"gpde_radius_csr_batched_{name}" in protos


# ---- the planning entry point -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,r,lo,hi,n", [(2, 0.1, (0.0, 0.0), (1.0, 1.0), 58081), (1, 0.011, (-1.0,), (2.0,), 4000),
                                           (3, 0.16, (0.0, 0.5, -2.0), (1.0, 0.75, 3.0), 2500), (2, 1e-9, (0.0, 0.0), (1.0, 1.0), 10)])
def test_plan_of_one_graph_is_the_grid_of_the_open_builder(dim, r, lo, hi, n):
    """B = 1: the cell counts follow make_grid's rule (cells of edge 1.0001 r, doubled while more than 2^24 of them) and the
    workspace is what gpde_radius_csr_workspace_bytes answers for that graph."""
    rc, rec, n_cells, ws = _plan([lo, hi], [0, n], [r], dim)
    assert rc == 0
    cs = r * 1.0001
    while math.prod(int(math.floor((h - l) / cs)) + 1 for l, h in zip(lo, hi)) > CAP:
        cs *= 2.0
    nc = [int(math.floor((h - l) / cs)) + 1 for l, h in zip(lo, hi)] + [1] * (3 - dim)
    assert rec["nc"][0].tolist() == nc and n_cells == math.prod(nc) <= CAP
    assert rec["lo"][0].tolist() == list(lo) + [0.0] * (3 - dim)
    assert rec["inv"][0].tolist() == [1.0 / cs] * dim + [0.0] * (3 - dim)
    assert rec["r2"][0] == r * r and abs(rec["d2_max"][0] - r * r) <= 4 * np.spacing(r * r)
    assert math.sqrt(rec["d2_max"][0]) <= r < math.sqrt(np.nextafter(rec["d2_max"][0], np.inf))
    assert (rec["cell_base"][0], rec["src_begin"][0], rec["src_end"][0], rec["dst_begin"][0], rec["dst_end"][0]) == (0, 0, n, 0, n)
    assert ws == int(_lib.lib().gpde_radius_csr_workspace_bytes(n, dim, r, _f64(*lo), _f64(*hi))) > 0
    assert _plan([lo, hi], [0, n], [r], dim, want_table=False)[2:] == (n_cells, ws)       # a query writes no table


def test_plan_lays_graphs_out_by_cell_base_with_their_own_grids():
    bounds = [[(0.0, 0.0), (1.0, 1.0)], [(100.0, 100.0), (100.001, 100.001)], [(5.0, 5.0), (5.0, 5.0)], [(np.inf, np.inf), (-np.inf, -np.inf)],
              [(0.0, -1.0), (2.0, 1.0)]]
    ptr, ptr_dst, radii = [0, 10, 30, 35, 35, 60], [0, 4, 4, 9, 20, 21], [0.05, 0.3, 0.11, 0.2, 0.5]
    rc, rec, n_cells, ws = _plan(bounds, ptr, radii, 2, ptr_dst=ptr_dst)
    assert rc == 0
    want_nc = [[20, 20, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [4, 4, 1]]      # floor(ext / (1.0001 r)) + 1; coincident / no sources: one cell
    assert rec["nc"].tolist() == want_nc
    cells = [a * b * c for a, b, c in want_nc]
    assert rec["cell_base"].tolist() == np.concatenate([[0], np.cumsum(cells)[:-1]]).tolist() and n_cells == sum(cells)
    assert rec["src_begin"].tolist() == ptr[:-1] and rec["src_end"].tolist() == ptr[1:]
    assert rec["dst_begin"].tolist() == ptr_dst[:-1] and rec["dst_end"].tolist() == ptr_dst[1:]
    assert rec["lo"][1].tolist() == [100.0, 100.0, 0.0] and rec["lo"][3].tolist() == [0.0, 0.0, 0.0] and rec["inv"][3].tolist() == [0.0] * 3
    assert rec["r2"].tolist() == [r * r for r in radii]
    # one point set: ptr_dst NULL = ptr_src
    rec1 = _plan(bounds, ptr, radii, 2)[1]
    assert rec1["dst_begin"].tolist() == ptr[:-1] and rec1["dst_end"].tolist() == ptr[1:]
    # the workspace holds four uint32 arrays over all sources and the start array over all cells
    assert ws >= 4 * 4 * 60 + 4 * (n_cells + 1)


def test_plan_coarsens_every_graph_when_the_summed_cells_exceed_the_cap():
    r = 1.0 / 4000.5 / 1.0001                              # 4001 x 4001 = 16.0 M cells per graph: under the cap alone
    unit = [(0.0, 0.0), (1.0, 1.0)]
    rc, rec, n_cells, _ = _plan([unit], [0, 5], [r], 2)
    assert rc == 0 and rec["nc"][0].tolist() == [4001, 4001, 1] and n_cells == 4001 * 4001 <= CAP
    rc, rec, n_cells, ws = _plan([unit] * 4, [0, 5, 10, 15, 20], [r] * 4, 2)
    assert rc == 0 and n_cells <= CAP
    assert rec["nc"].tolist() == [[2001, 2001, 1]] * 4 and n_cells == 4 * 2001 * 2001          # every cell edge doubled once
    assert rec["inv"][0][0] == 1.0 / (2.0 * r * 1.0001)
    assert rec["cell_base"].tolist() == [k * 2001 * 2001 for k in range(4)]
    assert rec["r2"].tolist() == [r * r] * 4                                                    # the radius itself is untouched
    assert ws < (1 << 28)
    # graphs of unequal radii: all are coarsened together, deterministically
    rc, rec, n_cells, _ = _plan([unit] * 3, [0, 5, 10, 15], [r, r, 0.5], 2)
    assert rc == 0 and rec["nc"].tolist() == [[2001, 2001, 1], [2001, 2001, 1], [1, 1, 1]] and n_cells == 2 * 2001 * 2001 + 1


def test_plan_of_empty_batches():
    rc, rec, n_cells, ws = _plan(np.zeros((0, 2, 2)), [0], [], 2)
    assert (rc, len(rec), n_cells) == (0, 0, 0) and ws > 0
    rc, rec, n_cells, ws = _plan(np.full((3, 2, 1), np.nan), [0, 0, 0, 0], [0.1, 0.2, 0.3], 1)      # all graphs empty: bounds unread
    assert rc == 0 and n_cells == 3 and rec["nc"].tolist() == [[1, 1, 1]] * 3 and rec["cell_base"].tolist() == [0, 1, 2]


PLAN_INVALID = {
    "dim 0": (dict(dim=0), b"dim"),
    "dim 4": (dict(dim=4), b"dim"),
    "r zero": (dict(radii=[0.1, 0.0]), b"r[1]"),
    "r negative": (dict(radii=[-0.1, 0.1]), b"r[0]"),
    "r inf": (dict(radii=[0.1, math.inf]), b"r[1]"),
    "r nan": (dict(radii=[math.nan, 0.1]), b"r[0]"),
    "ptr start": (dict(ptr=[1, 5, 9]), b"ptr_src[0]"),
    "ptr decreases": (dict(ptr=[0, 9, 5]), b"decreases"),
    "ptr_dst decreases": (dict(ptr_dst=[0, 9, 5]), b"ptr_dst"),
    "ptr too long": (dict(ptr=[0, 5, 1 << 31]), b"2^31"),
}


@pytest.mark.parametrize("what", sorted(PLAN_INVALID))
def test_plan_refuses_with_a_text(what):
    kw, text = PLAN_INVALID[what]
    args = dict(bounds=[[(0.0, 0.0), (1.0, 1.0)]] * 2, ptr=[0, 5, 9], radii=[0.1, 0.1], dim=2)
    args.update(kw)
    assert _plan(**args)[0] == EINVAL, what
    assert text in _lib.lib().gpde_last_error(), (what, _lib.lib().gpde_last_error())


def test_plan_refuses_null_arrays_and_negative_batches():
    l = _lib.lib()
    nc, ws = ctypes.c_int64(0), ctypes.c_size_t(0)
    ok = (BUF, _i64(0, 5), None, _f64(0.1), 1, 2, None, ctypes.byref(nc), ctypes.byref(ws))
    for k in (0, 1, 3, 7, 8):                             # bounds, ptr_src, r, n_cells, ws_bytes
        a = list(ok)
        a[k] = None
        assert l.gpde_radius_csr_batched_plan(*a) == EINVAL, k
        assert l.gpde_last_error() != b""
    a = list(ok)
    a[4] = -1
    assert l.gpde_radius_csr_batched_plan(*a) == EINVAL and b"n_graphs" in l.gpde_last_error()


# ---- count / fill: refusals before any device call ------------------------------------------------------------------------------
def _count(ns=9, nd=9, dim=2, flags=0, ptr=(0, 5, 9), ptr_dst=(0, 5, 9), b=2, table=BUF, n_cells=2, deg=BUF, ws=BUF, ws_bytes=1 << 20, ps=BUF, pd=BUF):
    return _lib.lib().gpde_radius_csr_batched_count(ps, ns, pd, nd, dim, flags, None if ptr is None else _i64(*ptr),
                                                    None if ptr_dst is None else _i64(*ptr_dst), b, table, n_cells, deg, ws, ws_bytes, None)


def _fill(ns=9, nd=9, dim=2, flags=0, ptr=(0, 5, 9), ptr_dst=(0, 5, 9), b=2, table=BUF, n_cells=2, rowptr=BUF, src=BUF, dst=BUF, e=3, ws=BUF,
          ws_bytes=1 << 20, ps=BUF, pd=BUF):
    return _lib.lib().gpde_radius_csr_batched_fill(ps, ns, pd, nd, dim, flags, None if ptr is None else _i64(*ptr),
                                                   None if ptr_dst is None else _i64(*ptr_dst), b, table, n_cells, rowptr, src, dst, e, ws, ws_bytes, None)


CALL_INVALID = {
    "dim 0": (dict(dim=0), b"dim"),
    "dim 4": (dict(dim=4), b"dim"),
    "flags": (dict(flags=2), b"flags"),
    "n_graphs negative": (dict(b=-1), b"n_graphs"),
    "ptr null": (dict(ptr=None), b"ptr_src"),
    "ptr_dst null": (dict(ptr_dst=None), b"ptr_dst"),
    "ptr start": (dict(ptr=(1, 5, 9)), b"ptr_src[0]"),
    "ptr decreases": (dict(ptr=(0, 6, 5), ns=5), b"decreases"),
    "ptr end": (dict(ptr=(0, 5, 8)), b"ends at 8"),
    "ptr_dst end": (dict(ptr_dst=(0, 5, 10)), b"ptr_dst ends at 10"),
    "too many points": (dict(ns=1 << 31), b"2^31"),
    "no positions": (dict(ps=None), b"pos_src"),
    "one point set, two ptr": (dict(ptr_dst=(0, 4, 9)), b"one point set"),
    "no table": (dict(table=None), b"table"),
    "n_cells": (dict(n_cells=1), b"n_cells"),
    "no workspace": (dict(ws=None), b"ws"),
}


@pytest.mark.parametrize("what", sorted(CALL_INVALID))
def test_count_and_fill_refuse_before_any_device_call(what):
    kw, text = CALL_INVALID[what]
    for fn in (_count, _fill):
        assert fn(**kw) == EINVAL, (what, fn.__name__)
        assert text in _lib.lib().gpde_last_error(), (what, _lib.lib().gpde_last_error())


def test_count_and_fill_further_refusals_and_empty_calls():
    l = _lib.lib()
    assert _count(deg=None) == EINVAL and b"deg" in l.gpde_last_error()
    assert _fill(rowptr=None) == EINVAL and _fill(src=None) == EINVAL and _fill(e=-1) == EINVAL
    assert _count(ws_bytes=16) == EWORKSPACE and _fill(ws_bytes=16) == EWORKSPACE and b"workspace" in l.gpde_last_error()
    # B = 0 and zero points are valid calls: nothing is launched, nothing is read
    assert _count(ns=0, nd=0, ptr=(0,), ptr_dst=(0,), b=0, table=None, n_cells=0, deg=None, ps=None, pd=None) == 0
    assert _fill(ns=0, nd=0, ptr=(0,), ptr_dst=(0,), b=0, table=None, n_cells=0, src=None, dst=None, e=0, ps=None, pd=None) == 0
    assert _count(ns=0, nd=0, ptr=(0, 0, 0), ptr_dst=(0, 0, 0), deg=None, ps=None, pd=None) == 0        # all graphs empty
    assert _count(ns=9, nd=0, ptr_dst=(0, 0, 0), deg=None, pd=None) == 0                                 # sources, no destinations


# ---- ops: ptr_from_batch ---------------------------------------------------------------------------------------------------------
def test_ptr_from_batch():
    t = torch.tensor
    assert ops.ptr_from_batch(t([0, 0, 0, 1, 3, 3])).tolist() == [0, 3, 4, 4, 6]                       # graph 2 has no points
    assert ops.ptr_from_batch(t([0, 0, 0, 1, 3, 3]), n_graphs=6).tolist() == [0, 3, 4, 4, 6, 6, 6]
    assert ops.ptr_from_batch(t([2, 2], dtype=torch.int32)).tolist() == [0, 0, 0, 2]
    assert ops.ptr_from_batch(t([], dtype=torch.int64)).tolist() == [0]
    assert ops.ptr_from_batch(t([], dtype=torch.int64), n_graphs=3).tolist() == [0, 0, 0, 0]
    p = ops.ptr_from_batch(t([0, 1, 1]))
    assert p.dtype == torch.int64 and p.shape == (3,)
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 9, size=50)
    batch = torch.from_numpy(np.repeat(np.arange(50), counts))
    assert ops.ptr_from_batch(batch, n_graphs=50).tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    with pytest.raises(ValueError, match="not sorted"):
        ops.ptr_from_batch(t([0, 1, 0]))
    with pytest.raises(ValueError, match="negative"):
        ops.ptr_from_batch(t([-1, 0]))
    with pytest.raises(ValueError, match="n_graphs = 2"):
        ops.ptr_from_batch(t([0, 2]), n_graphs=2)
    with pytest.raises(ValueError, match="1-D integer"):
        ops.ptr_from_batch(t([0.0, 1.0]))
    with pytest.raises(ValueError, match="1-D integer"):
        ops.ptr_from_batch(t([[0, 1]]))


# ---- ops: every argument error on CPU tensors, before the device check ----------------------------------------------------------
@pytest.mark.parametrize("fn", [ops.radius_csr_batched, ops.radius_graph_batched], ids=["csr", "graph"])
def test_ops_refuse_on_the_host(fn):
    pos, q = torch.rand(20, 2, dtype=torch.float64), torch.rand(8, 2, dtype=torch.float64)      # CPU tensors
    ptr, ptr_q = torch.tensor([0, 5, 20]), torch.tensor([0, 8, 8])
    bad = [
        (dict(ptr=torch.tensor([[0, 5, 20]])), "1-D integer"),                                   # the ptr shape ...
        (dict(ptr=torch.tensor([], dtype=torch.int64)), "1-D integer"),
        (dict(ptr=torch.tensor([0.0, 5.0, 20.0])), "1-D integer"),
        (dict(ptr=[1, 5, 20]), "must start at 0"),                                               # ... its start ...
        (dict(ptr=[0, 5, 19]), "ends at 19, the position array has 20"),                         # ... its end ...
        (dict(ptr=[0, 25, 20]), "ptr decreases"),                                                # ... its monotonicity
        (dict(r=[0.1]), "r has 1 entries for 2 graphs"),                                         # the length of r
        (dict(r=torch.tensor([0.1, 0.2, 0.3])), "r has 3 entries for 2 graphs"),
        (dict(r=0.0), "must be positive"), (dict(r=-1.0), "must be positive"),                   # a non-positive r
        (dict(r=[0.1, 0.0]), r"r\[1\] = 0.0 must be positive"), (dict(r=float("inf")), "finite"),
        (dict(r=[float("nan"), 0.1]), r"r\[0\]"),
        (dict(pos_dst=torch.rand(8, 3, dtype=torch.float64), ptr_dst=ptr_q), "same dimension"),  # a dimension mismatch
        (dict(pos=torch.rand(20, 4, dtype=torch.float64)), "dimension 4"),
        (dict(ptr_dst=ptr_q), "ptr_dst given without pos_dst"),
        (dict(pos_dst=q), "pos_dst given without ptr_dst"),
        (dict(pos_dst=q, ptr_dst=[0, 8]), "ptr_dst divides pos_dst into 1 graphs, ptr divides pos into 2"),
        (dict(pos_dst=q, ptr_dst=[0, 3, 7]), "ptr_dst ends at 7"),
        (dict(period=1.0), "period= has no batched form"),                                       # out of scope, said so
        (dict(origin=0.0), "origin= has no batched form"),
        (dict(return_geometry=True), "single-graph forms"),
    ]
    for kw, text in bad:
        a = dict(pos=pos, ptr=ptr, r=0.1)
        a.update(kw)
        p, pt, r = a.pop("pos"), a.pop("ptr"), a.pop("r")
        with pytest.raises(ValueError, match=text):
            fn(p, pt, r, **a)
    with pytest.raises(TypeError, match="unexpected keyword"):
        fn(pos, ptr, 0.1, radius=0.2)
    for a in (dict(), dict(pos_dst=q, ptr_dst=ptr_q), dict(reference_ties=True)):
        with pytest.raises(RuntimeError, match="pos is on cpu"):      # a valid call on CPU tensors gets as far as the device check
            fn(pos, ptr, [0.1, 0.2], **a)
    with pytest.raises(RuntimeError, match="pos is on cpu"):
        fn(torch.rand(20, dtype=torch.float64), [0, 5, 20], 0.1)      # 1-D positions, ptr as a list


def test_batched_plan_wrapper_matches_the_entry_point():
    bounds = np.array([[(0.0, 0.0), (1.0, 1.0)], [(2.0, 2.0), (2.5, 3.0)]])
    ptr = torch.tensor([0, 7, 19])
    table, n_cells, ws = ops.batched_plan(torch.from_numpy(bounds), ptr, None, [0.2, 0.1], 2)
    rc, rec, n_cells2, ws2 = _plan(bounds, [0, 7, 19], [0.2, 0.1], 2)
    assert rc == 0 and (n_cells, ws) == (n_cells2, ws2)
    assert table.dtype == torch.uint8 and table.numel() == 2 * 96 and table.numpy().tobytes() == rec.tobytes()


# ---- the assembly the GPU tier compares against, pinned on code that is not under test ---------------------------------------------
def test_assembly_reproduces_the_reference_generators_multilevel_graphs():
    """tests/golden/mgkn_graphs_s20.npz is RandomMultiMeshGenerator's own output: its inner graphs are a batch of three self
    graphs with their own radii, its down graphs a batch of two graphs between two point sets.  Oracle per level + the
    concatenate-and-offset assembly must give the fixture's edge_index and per-level ranges."""
    g = np.load(os.path.join(GOLDEN, "mgkn_graphs_s20.npz"))
    m = [int(v) for v in g["m"]]
    lattice = synth.lattice_positions(int(g["s"])).double().numpy()
    levels = [lattice[g[f"idx{l}"]] for l in range(len(m))]
    pos, ptr = bg.concat_sets(levels)
    assert ptr.tolist() == np.concatenate([[0], np.cumsum(m)]).tolist()
    lists = bg.oracle_edge_lists(pos, ptr, g["radii_inner"], reference_ties=True)
    ei, edge_ptr = bg.assemble_edge_index(lists, ptr)
    assert np.array_equal(ei, g["edge_index"])
    assert edge_ptr.tolist() == [0] + [int(hi) for _, hi in g["range"]] and [int(lo) for lo, _ in g["range"]] == edge_ptr[:-1].tolist()
    # the CSR assembly is the stable sort by destination of that list
    rowptr, src, dst, edge_ptr2 = bg.oracle_csr(pos, ptr, g["radii_inner"], reference_ties=True)
    want = bg.csr_of_edges(g["edge_index"], int(ptr[-1]))
    assert np.array_equal(rowptr, want[0]) and np.array_equal(src, want[1]) and np.array_equal(dst, want[2])
    assert np.array_equal(edge_ptr2, edge_ptr) and np.array_equal(edge_ptr2, rowptr[ptr])
    # two point sets: sources = levels 0, 1, destinations = levels 1, 2; the fixture numbers all levels in one range
    ps, ptr_s = bg.concat_sets(levels[:-1])
    pd, ptr_d = bg.concat_sets(levels[1:])
    down = bg.oracle_edge_lists(ps, ptr_s, g["radii_inter"], pd, ptr_d, reference_ties=True)
    ei_d, edge_ptr_d = bg.assemble_edge_index(down, ptr_s, ptr_d)
    assert edge_ptr_d.tolist() == [0] + [int(hi) for _, hi in g["range_down"]]
    ei_d[1] += m[0]                                         # destination ids of the batch start at 0, the fixture's after level 0
    assert np.array_equal(ei_d, g["edge_index_down"])


def test_assembly_on_a_hand_made_batch():
    """Three graphs on a line, the middle one empty: ids, rows and edge_ptr by hand."""
    pos, ptr = bg.concat_sets([[[0.0], [1.0], [1.5]], np.zeros((0, 1)), [[0.0], [0.4]]])
    assert ptr.tolist() == [0, 3, 3, 5]
    rowptr, src, dst, edge_ptr = bg.oracle_csr(pos, ptr, [0.6, 9.0, 0.5])
    assert rowptr.tolist() == [0, 1, 3, 5, 7, 9] and edge_ptr.tolist() == [0, 5, 5, 9]
    assert src.tolist() == [0, 1, 2, 1, 2, 3, 4, 3, 4] and dst.tolist() == [0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert np.array_equal(edge_ptr, rowptr[ptr])
    ei, edge_ptr2 = bg.assemble_edge_index(bg.oracle_edge_lists(pos, ptr, [0.6, 9.0, 0.5]), ptr)
    assert ei.tolist() == [[0, 1, 1, 2, 2, 3, 3, 4, 4], [0, 1, 2, 1, 2, 3, 4, 3, 4]] and edge_ptr2.tolist() == [0, 5, 5, 9]
    # the whole batch as ONE point set would join graph 0 and graph 2 (both hold the point 0.0): the assembly does not
    assert radius_oracle.radius_edges(pos, 0.6, reference_ties=False).shape[1] > ei.shape[1]


def test_gpu_tier_inputs_are_what_they_are_meant_to_be():
    pos, ptr = bg.unit_box_batch()
    assert ptr.tolist() == [0, 37, 37, 38, 102, 232] and pos.min() >= 0.0 and pos.max() <= 1.0
    rowptr, src, dst, edge_ptr = bg.oracle_csr(pos, ptr, [0.2] * 5)
    whole = radius_oracle.radius_edges(pos, 0.2, reference_ties=False)
    assert whole.shape[1] > 2 * len(src)                    # most pairs within r belong to different graphs: a leak would show
