"""Host tier of the batched and the periodic k-nearest-neighbour graphs (graph_pde_amd.neighbor_graph: knn_csr_batched /
knn_graph_batched, knn_csr(period=...); gpde_knn_csr_batched*, gpde_knn_csr_periodic*): the ABI additions, every
refusal that needs no device, the k_eff / edge_ptr / rowptr arithmetic of a batch, the plan call on host values, and the oracles
of the GPU tier on inputs whose answer is known by hand."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, neighbor_graph as ng, ops
from tests.helpers import batched_graphs as bg
from tests.helpers import knn_arms_oracle as ao
from tests.helpers import knn_oracle as ko

ENTRY_POINTS = ("gpde_knn_csr_batched_plan", "gpde_knn_csr_batched", "gpde_knn_csr_periodic_workspace_bytes", "gpde_knn_csr_periodic")

REC = np.dtype([("lo", "<f8", 3), ("inv", "<f8", 3), ("h", "<f8"), ("mag", "<f8", 3), ("nc", "<i4", 3), ("cell_base", "<i4"),
                ("src_begin", "<i4"), ("src_end", "<i4"), ("dst_begin", "<i4"), ("dst_end", "<i4"), ("k_eff", "<i4"), ("edge_base", "<i4"),
                ("n_rings", "<i4"), ("pad", "<i4")])


def test_the_entry_points_are_in_the_header_the_binding_and_the_library():
    protos = _lib.header_prototypes()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ENTRY_POINTS:
        assert name in protos and name in _lib.SIGNATURES and name in exported, name
        assert hasattr(_lib.lib(), name)
    assert protos["gpde_knn_csr_batched_plan"] == ("int", ["const double*", "const int64_t*", "const int64_t*", "int64_t", "int", "int64_t", "int",
                                                           "double", "void*", "int64_t*", "size_t*", "int64_t*"])
    assert protos["gpde_knn_csr_batched"][1] == ["const double*", "int64_t", "const double*", "int64_t", "int", "int64_t", "int", "const int64_t*",
                                                 "const int64_t*", "int64_t", "const void*", "int64_t", "int32_t*", "int32_t*", "int32_t*", "float*",
                                                 "int64_t", "void*", "size_t", "void*"]
    assert protos["gpde_knn_csr_periodic_workspace_bytes"] == ("size_t", ["int64_t", "int64_t", "int", "int64_t", "double", "const double*",
                                                                          "const double*", "const double*", "const double*"])
    assert protos["gpde_knn_csr_periodic"][1] == ["const double*", "int64_t", "const double*", "int64_t", "int", "int64_t", "int", "double",
                                                  "const double*", "const double*", "const double*", "const double*", "int32_t*", "int32_t*",
                                                  "int32_t*", "float*", "void*", "size_t", "void*"]
    header = open(_lib.HEADER_PATH).read()
    assert "GPDE_KNN_BATCHED_REC_BYTES = 128" in header and REC.itemsize == _lib.GPDE_KNN_BATCHED_REC_BYTES == 128
    assert _lib.lib().gpde_version() == 101


def test_the_builders_are_module_functions():
    for name in ("knn_csr_batched", "knn_graph_batched"):
        assert callable(getattr(gp.neighbor_graph, name)) and not hasattr(ops, name)
    import inspect
    for fn in (ng.knn_csr, ng.knn_graph):
        assert {"period", "origin"} <= set(inspect.signature(fn).parameters)


# ---- Python refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", (ng.knn_csr, ng.knn_graph), ids=lambda f: f.__name__)
def test_periodic_value_errors_are_raised_without_a_device(fn):
    pos = torch.rand(10, 2, dtype=torch.float64)                     # CPU tensors: a refusal never reaches the device
    nan, inf = float("nan"), float("inf")
    for period in (-1.0, nan, inf, (1.0, -0.5), (1.0, nan), (1.0,), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="period"):
            fn(pos, 3, period=period)
    for origin in (nan, inf, (0.0, -inf), (0.0,)):
        with pytest.raises(ValueError, match="origin"):
            fn(pos, 3, period=1.0, origin=origin)
    with pytest.raises(ValueError, match="k must be"):
        fn(pos, 0, period=1.0)
    with pytest.raises(ValueError, match="loop=True with pos_dst"):
        fn(pos, 3, pos_dst=torch.rand(4, 2), loop=True, period=1.0)
    with pytest.raises(ValueError, match="bounds"):
        fn(pos, 3, period=(1.0, 0.0), bounds=(1.0, 0.0))
    # everything in order: the refusal of a CPU tensor, in the other builders' words
    for kw in (dict(period=1.0), dict(period=(1.0, None)), dict(period=(0.0, 2.0), origin=(3.0, -1.0)), dict(period=1.0, loop=True),
               dict(period=torch.tensor([1.0, 1.5])), dict(period=0.0), dict(period=1.0, pos_dst=torch.rand(4, 2, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="no CPU / composite fallback exists by design"):
            fn(pos, 3, **kw)


@pytest.mark.parametrize("fn", (ng.knn_csr_batched, ng.knn_graph_batched), ids=lambda f: f.__name__)
def test_batched_value_errors_are_raised_without_a_device(fn):
    pos, ptr = torch.rand(10, 2, dtype=torch.float64), [0, 4, 10]
    pd = torch.rand(6, 2, dtype=torch.float64)
    for k in (0, -1, 257, 2.0, None, True):
        with pytest.raises(ValueError, match="k must be"):
            fn(pos, ptr, k)
    with pytest.raises(ValueError, match="loop"):
        fn(pos, ptr, 3, loop=1)
    with pytest.raises(ValueError, match="cell_size"):
        fn(pos, ptr, 3, cell_size=0.0)
    with pytest.raises(ValueError, match="ptr_dst given without pos_dst"):
        fn(pos, ptr, 3, ptr_dst=[0, 3, 6])
    with pytest.raises(ValueError, match="pos_dst given without ptr_dst"):
        fn(pos, ptr, 3, pos_dst=pd)
    with pytest.raises(ValueError, match="loop=True with pos_dst"):
        fn(pos, ptr, 3, pos_dst=pd, ptr_dst=[0, 3, 6], loop=True)
    with pytest.raises(ValueError, match="same dimension"):
        fn(pos, ptr, 3, pos_dst=torch.rand(6, 3), ptr_dst=[0, 3, 6])
    with pytest.raises(ValueError, match="dim"):
        fn(torch.rand(10, 4), ptr, 3)
    for bad, what in (([1, 4, 10], "start at 0"), ([0, 6, 4, 10], "decreases"), ([0, 4, 9], "ends at"), ([0.0, 10.0], "integer"), ([], "integer")):
        with pytest.raises(ValueError, match=what):
            fn(pos, bad, 3)
    with pytest.raises(ValueError, match="graphs"):
        fn(pos, ptr, 3, pos_dst=pd, ptr_dst=[0, 6])
    for name in ("period", "origin"):
        with pytest.raises(ValueError, match=f"{name}= has no batched form"):
            fn(pos, ptr, 3, **{name: 1.0})
    with pytest.raises(TypeError, match="unexpected keyword"):
        fn(pos, ptr, 3, radius=1.0)
    nan = float("nan")
    for bounds in (np.zeros((2, 2, 3)), np.zeros((3, 2, 2)), [[[0.0, 0.0], [1.0, nan]], [[0.0, 0.0], [1.0, 1.0]]],
                   [[[0.0, 0.0], [1.0, 1.0]], [[0.5, 0.0], [0.0, 1.0]]], "box"):
        with pytest.raises(ValueError, match="bounds"):
            fn(pos, ptr, 3, bounds=bounds)
    with pytest.raises(ValueError, match="int32 CSR"):
        fn(torch.empty((1 << 24, 2), dtype=torch.float64, device="meta"), [0, 1 << 23, 1 << 24], 256)
    for kw in (dict(), dict(loop=True), dict(bounds=np.tile(np.array([[0.0, 0.0], [1.0, 1.0]]), (2, 1, 1))), dict(cell_size=0.1),
               dict(pos_dst=pd, ptr_dst=[0, 3, 6])):
        with pytest.raises(RuntimeError, match="no CPU / composite fallback exists by design"):
            fn(pos, ptr, 3, **kw)
    # the box of a graph WITHOUT sources is not read
    with pytest.raises(RuntimeError, match="no CPU / composite fallback"):
        fn(pos, [0, 0, 10], 3, bounds=[[[nan, nan], [nan, nan]], [[0.0, 0.0], [1.0, 1.0]]])


# ---- the arithmetic of a batch -----------------------------------------------------------------------------------------------------
def test_k_eff_edge_ptr_and_rowptr_arithmetic():
    ptr = torch.tensor([0, 37, 37, 38, 102, 232])
    ptr_dst = torch.tensor([0, 20, 25, 25, 89, 96])
    for k in (1, 5, 36, 37, 64, 200):
        for one, loop in ((True, False), (True, True), (False, False)):
            ke, edge_ptr = ng.batch_slots(ptr, None if one else ptr_dst, k, one, loop)
            assert ke.tolist() == ao.batch_k_eff(ptr.numpy(), k, one, loop) and min(ke.tolist()) >= 0
            nd = (ptr if one else ptr_dst).diff()
            assert edge_ptr.dtype == torch.int64 and edge_ptr.tolist() == [0] + torch.cumsum(nd * ke, 0).tolist()
    assert ng.batch_slots(ptr, None, 5, True, False)[0].tolist() == [5, 0, 0, 5, 5]           # the one-point graph has no neighbour
    assert ng.batch_slots(ptr, None, 5, True, True)[0].tolist() == [5, 0, 1, 5, 5]
    # the oracle's batch: rowptr[i] = edge_ptr[b] + (i - ptr_dst[b]) * k_eff[b], edge_ptr = rowptr[ptr_dst]
    for name, k, loop in (("unit_box", 37, False), ("unit_box", 37, True), ("two_sets", 64, False), ("b0", 3, False)):
        c = ao.BATCHES[name]()
        rowptr, src, dst, edge_ptr = ao.batched(c["pos"], c["ptr"], k, c.get("pos_dst"), c.get("ptr_dst"), loop)
        pd = c.get("ptr_dst", c["ptr"])
        ke, ep = ng.batch_slots(torch.from_numpy(c["ptr"]), torch.from_numpy(c["ptr_dst"]) if "ptr_dst" in c else None, k, "pos_dst" not in c, loop)
        assert np.array_equal(edge_ptr, ep.numpy()) and np.array_equal(edge_ptr, rowptr[pd])
        for b in range(len(pd) - 1):
            i = np.arange(pd[b], pd[b + 1])
            assert np.array_equal(rowptr[i], edge_ptr[b] + (i - pd[b]) * int(ke[b]))
            s = src[edge_ptr[b]:edge_ptr[b + 1]]
            assert ((s >= c["ptr"][b]) & (s < c["ptr"][b + 1])).all()


def _plan(bounds, ptr, ptr_dst, k, loop, cell, dim, table=True):
    l = _lib.lib()
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    b = len(ptr) - 1
    bounds = np.ascontiguousarray(bounds, dtype=np.float64)
    pd = None if ptr_dst is None else np.ascontiguousarray(ptr_dst, dtype=np.int64)
    tab = np.zeros(max(b, 1), dtype=REC)
    n_cells, nbytes, n_edges = ctypes.c_int64(-1), ctypes.c_size_t(0), ctypes.c_int64(-1)
    rc = l.gpde_knn_csr_batched_plan(bounds.ctypes.data if bounds.size else None, ptr.ctypes.data, None if pd is None else pd.ctypes.data, b, dim, k,
                                     loop, cell, tab.ctypes.data if table else None, ctypes.byref(n_cells), ctypes.byref(nbytes), ctypes.byref(n_edges))
    return rc, tab[:b], n_cells.value, nbytes.value, n_edges.value


def test_the_plan_on_host_values():
    c = ao.BATCHES["unit_box"]()
    bounds = ao.batch_bounds(c)
    rc, tab, n_cells, nbytes, e = _plan(bounds, c["ptr"], None, 5, 0, 0.0, 2)
    assert rc == 0 and nbytes > 0 and e == 5 * (37 + 64 + 130)
    assert tab["k_eff"].tolist() == [5, 0, 0, 5, 5] and tab["edge_base"].tolist() == [0, 185, 185, 185, 505]
    assert tab["src_begin"].tolist() == c["ptr"][:-1].tolist() and tab["dst_end"].tolist() == c["ptr"][1:].tolist()
    cells = tab["nc"].prod(axis=1)
    assert n_cells == cells.sum() and tab["cell_base"].tolist() == [0] + np.cumsum(cells)[:-1].tolist()
    assert cells[1] == 1 and cells[2] == 1                            # no sources / one point: one cell
    assert (tab["n_rings"] == tab["nc"].max(axis=1)).all() and cells[4] > 1
    # identical records from a second call, and the same numbers from a query without a table
    rc2, tab2, n2, b2, e2 = _plan(bounds, c["ptr"], None, 5, 0, 0.0, 2)
    assert rc2 == 0 and tab2.tobytes() == tab.tobytes() and (n2, b2, e2) == (n_cells, nbytes, e)
    assert _plan(bounds, c["ptr"], None, 5, 0, 0.0, 2, table=False)[2:] == (n_cells, nbytes, e)
    # loop = 1 and two point sets
    assert _plan(bounds, c["ptr"], None, 5, 1, 0.0, 2)[1]["k_eff"].tolist() == [5, 0, 1, 5, 5]
    t = ao.BATCHES["two_sets"]()
    rc, tab, _, _, e = _plan(ao.batch_bounds(t), t["ptr"], t["ptr_dst"], 64, 1, 0.0, 2)
    assert rc == 0 and tab["k_eff"].tolist() == [37, 0, 1, 64, 64] and e == 20 * 37 + 0 + 0 + 64 * 64 + 7 * 64
    # the cell-count cap: an absurdly fine edge is doubled, for every graph, until the sum fits 2^24
    rc, tab, n_cells, nbytes, _ = _plan(bounds, c["ptr"], None, 5, 0, 1e-9, 2)
    assert rc == 0 and n_cells <= 1 << 24 and nbytes < 1 << 28
    h = tab["h"][[0, 3, 4]]
    assert (h == h[0]).all() and np.log2(h[0] / 1e-9) == round(np.log2(h[0] / 1e-9)) and h[0] > 1e-9
    # coincident points: one cell; a graph without sources: its box is not read; B = 0
    rc, tab, n_cells, _, e = _plan(np.array([[[0.5, 0.5], [0.5, 0.5]], [[np.nan, 0.0], [np.inf, -1.0]]]), [0, 9, 9], [0, 9, 13], 3, 1, 0.0, 2)
    assert rc == 0 and n_cells == 2 and tab["k_eff"].tolist() == [3, 0] and e == 27
    assert _plan(np.zeros((0, 2, 2)), [0], None, 3, 0, 0.0, 2)[2:] == (0, _plan(np.zeros((0, 2, 2)), [0], None, 3, 0, 0.0, 2)[3], 0)


def test_the_library_refuses_a_bad_batch_before_any_device_call():
    l = _lib.lib()
    c = ao.BATCHES["unit_box"]()
    bounds = ao.batch_bounds(c)
    nan, inf = float("nan"), float("inf")
    ok = dict(bounds=bounds, ptr=c["ptr"], ptr_dst=None, k=5, loop=0, cell=0.0, dim=2)
    bad_box = bounds.copy(); bad_box[3, 1, 0] = nan
    empty_box = bounds.copy(); empty_box[0, 0, 1] = 2.0
    for bad in (dict(k=0), dict(k=257), dict(loop=2), dict(loop=-1), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(cell=1e-320),
                dict(ptr=[1, 5]), dict(ptr=[0, 5, 3]), dict(ptr=[0, 1 << 31]), dict(ptr_dst=[0, 5, 3, 9, 9, 9]), dict(bounds=bad_box),
                dict(bounds=empty_box), dict(bounds=np.zeros(0)), dict(ptr=[0, 300, 300 + (1 << 24)], bounds=bounds[:2], k=256)):
        v = dict(ok); v.update(bad)
        assert _plan(**v)[0] == -1, bad
        assert l.gpde_last_error(), bad
    assert _plan(**dict(ok, dim=0))[0] == -2 and _plan(**dict(ok, dim=4))[0] == -2                # GPDE_EUNSUPPORTED
    ptr = np.ascontiguousarray(c["ptr"])
    out = ctypes.c_int64(0)
    sz = ctypes.c_size_t(0)
    assert l.gpde_knn_csr_batched_plan(bounds.ctypes.data, None, None, 5, 2, 5, 0, 0.0, None, ctypes.byref(out), ctypes.byref(sz), ctypes.byref(out)) == -1
    assert l.gpde_knn_csr_batched_plan(bounds.ctypes.data, ptr.ctypes.data, None, 5, 2, 5, 0, 0.0, None, None, ctypes.byref(sz), ctypes.byref(out)) == -1
    assert l.gpde_knn_csr_batched_plan(bounds.ctypes.data, ptr.ctypes.data, None, -1, 2, 5, 0, 0.0, None, ctypes.byref(out), ctypes.byref(sz), ctypes.byref(out)) == -1

    # gpde_knn_csr_batched: a fake non-null "device" address is never dereferenced - every call below returns before a device call
    P, n = 0x1000, int(ptr[-1])
    e5 = 5 * (37 + 64 + 130)
    pd2 = np.ascontiguousarray([0, 20, 25, 25, 89, 96], dtype=np.int64)

    def run(ps=P, ns=n, pd=P, nd=n, dim=2, k=5, loop=0, p_src=ptr, p_dst=None, b=5, table=P, n_cells=100, rowptr=P, src=P, dst=P, e=e5, w=P, wb=1 << 24):
        p_src = None if p_src is None else np.ascontiguousarray(p_src, dtype=np.int64)
        p_dst = None if p_dst is None else np.ascontiguousarray(p_dst, dtype=np.int64)
        return l.gpde_knn_csr_batched(ps, ns, pd, nd, dim, k, loop, None if p_src is None else p_src.ctypes.data,
                                      None if p_dst is None else p_dst.ctypes.data, b, table, n_cells, rowptr, src, dst, None, e, w, wb, None)

    for bad in (dict(ps=None), dict(pd=None), dict(ns=-1), dict(nd=1 << 31), dict(k=0), dict(k=257), dict(loop=2), dict(p_src=None), dict(ns=n + 1, pd=0x2000, loop=1),
                dict(p_src=[0, 5, 3, n, n, n]), dict(p_src=[1, 5, 7, n, n, n]), dict(p_dst=pd2), dict(pd=0x2000, nd=96, p_dst=pd2, loop=0), dict(b=-1),
                dict(table=None), dict(n_cells=3), dict(rowptr=None), dict(src=None), dict(dst=None), dict(w=None), dict(e=e5 + 1), dict(e=-1)):
        assert run(**bad) == -1, bad
        assert l.gpde_last_error(), bad
    assert run(dim=0) == -2 and run(dim=4) == -2
    assert run(wb=16) == -3                                          # GPDE_EWORKSPACE
    assert run(pd=0x2000, nd=96, p_dst=pd2, loop=1, e=20 * 5 + 5 * 0 + 0 + 64 * 5 + 7 * 5, wb=16) == -3     # two point sets in order: only the workspace is short


def test_the_library_refuses_a_bad_torus_before_any_device_call():
    l = _lib.lib()
    D = ctypes.c_double * 2
    nan, inf = float("nan"), float("inf")
    lo, hi, org, per = D(0.0, 0.0), D(1.0, 1.0), D(0.0, 0.0), D(1.0, 1.0)
    q = l.gpde_knn_csr_periodic_workspace_bytes
    assert q(58081, 58081, 2, 16, 0.0, None, None, org, per) > 4 * 4 * 58081           # every axis periodic: no box is read
    assert q(100, 100, 2, 16, 0.0, None, None, None, per) > 0                           # origin NULL: 0
    assert q(100, 100, 2, 16, 0.0, lo, hi, org, D(1.0, 0.0)) > 0
    assert q(100, 100, 2, 16, 1e-12, None, None, org, per) < 1 << 28                    # an absurdly fine grid is coarsened
    assert q(0, 0, 1, 1, 0.0, None, None, org, per) > 0
    for bad in (dict(per=None), dict(per=D(-1.0, 1.0)), dict(per=D(1.0, nan)), dict(per=D(inf, 1.0)), dict(per=D(1e-320, 1.0)), dict(org=D(nan, 0.0)),
                dict(org=D(0.0, inf)), dict(per=D(1.0, 0.0)), dict(per=D(0.0, 1.0), lo=D(2.0, 0.0), hi=hi), dict(per=D(0.0, 0.0), lo=lo), dict(k=0),
                dict(k=257), dict(ns=-1), dict(nd=1 << 31), dict(cell=-1.0), dict(cell=nan), dict(nd=1 << 24, k=256, ns=300)):
        v = dict(ns=100, nd=100, dim=2, k=16, cell=0.0, lo=None, hi=None, org=org, per=per)
        v.update(bad)
        assert q(v["ns"], v["nd"], v["dim"], v["k"], v["cell"], v["lo"], v["hi"], v["org"], v["per"]) == 0, bad
        assert l.gpde_last_error(), bad
    P = 0x1000

    def knn(ps=P, ns=8, pd=0x2000, nd=8, dim=2, k=3, loop=0, cell=0.0, lo=None, hi=None, org=org, per=per, rowptr=P, src=P, dst=P, w=P, wb=1 << 20):
        return l.gpde_knn_csr_periodic(ps, ns, pd, nd, dim, k, loop, cell, lo, hi, org, per, rowptr, src, dst, None, w, wb, None)

    for bad in (dict(ps=None), dict(pd=None), dict(ns=-1), dict(nd=1 << 31), dict(k=0), dict(k=257), dict(loop=2), dict(loop=-1), dict(cell=-1.0),
                dict(cell=inf), dict(per=None), dict(per=D(-1.0, 1.0)), dict(per=D(nan, 1.0)), dict(per=D(1.0, inf)), dict(org=D(0.0, nan)),
                dict(per=D(1.0, 0.0)), dict(per=D(1.0, 0.0), lo=lo, hi=D(1.0, nan)), dict(rowptr=None), dict(src=None), dict(dst=None), dict(w=None),
                dict(nd=1 << 24, k=256, ns=300)):
        assert knn(**bad) == -1, bad
        assert l.gpde_last_error(), bad
    assert knn(dim=0) == -2 and knn(dim=4) == -2
    assert knn(wb=16) == -3
    assert knn(per=D(-1.0, 1.0)) == -1 and b"period" in l.gpde_last_error()


# ---- the oracles on inputs known by hand ---------------------------------------------------------------------------------------------
def test_the_periodic_oracle_on_inputs_known_by_hand():
    x = ao.ring8()
    rows = lambda k, loop=False, **kw: ao.periodic(x, k, 1.0, loop=loop, **kw)[1].reshape(8, -1).tolist()
    assert rows(2) == [sorted(((i - 1) % 8, (i + 1) % 8)) for i in range(8)]              # i +- 1, across the seam
    assert rows(1) == [[min((i - 1) % 8, (i + 1) % 8)] for i in range(8)]                # the tie goes to the smaller id
    assert rows(3, True) == [sorted(((i - 1) % 8, i, (i + 1) % 8)) for i in range(8)]
    assert rows(7) == [[j for j in range(8) if j != i] for i in range(8)] == rows(12)    # every source once, however large k is
    # the antipode lies at exactly half a period, whichever way round: one candidate, one edge
    assert ao.periodic(x, 8, 1.0, loop=True)[1].reshape(8, 8).tolist() == [list(range(8))] * 8
    # the same ring many periods away, and with an open axis in front
    far = x + np.array([3.0, -2.0, 0.0, 7.0, -5.0, 1.0, 0.0, 2.0])[:, None]
    assert ao.periodic(far, 2, 1.0)[1].reshape(8, 2).tolist() == rows(2)
    xy = np.concatenate([np.zeros((8, 1)), x], axis=1)
    assert ao.periodic(xy, 2, (0.0, 1.0))[1].reshape(8, 2).tolist() == rows(2)
    assert ao.periodic(x, 2, 0.0)[1].reshape(8, 2)[0].tolist() == [1, 2] and ko.oracle(x, 2)[1].reshape(8, 2)[0].tolist() == [1, 2]
    # geometry: source minus target at the minimum image
    rp, s, d = ao.periodic(x, 2, 1.0)
    g = ao.periodic_geometry(x, None, s, d, 1.0)
    assert g.dtype == np.float32 and g.shape == (16, 2) and g[:2].tolist() == [[0.125, 0.125], [-0.125, 0.125]]
    # two point sets
    rp, s, d = ao.periodic(x, 2, 1.0, xd=np.array([[0.99], [0.51]]))
    assert s.tolist() == [0, 7, 4, 5] and rp.tolist() == [0, 2, 4]
    for name in ("1d_64", "two_sets"):
        from tests.helpers import periodic_oracle as po
        c = po.CASES[name]()
        assert ao.periodic_ks(c) == ([1, 8, 64, 67] if name == "1d_64" else [1, 8, 64, 150, 153]) and len(ao.periodic_cells(c)) == 6
    assert np.abs(ao.outside_scaled()["xs"]).max() > 3e6


def test_the_batched_oracle_is_the_per_graph_oracle_with_offsets():
    c = ao.BATCHES["lattices"]()
    rowptr, src, dst, edge_ptr = ao.batched(c["pos"], c["ptr"], 4)
    assert edge_ptr.tolist() == [0, 324, 648, 972] and rowptr.tolist() == list(range(0, 973, 4))
    for b in range(3):
        assert src.reshape(243, 4)[81 * b + 40].tolist() == [81 * b + j for j in (31, 39, 41, 49)]
    one = ko.oracle(ko.lattice9(), 4)
    assert np.array_equal(src[:324], one[1]) and np.array_equal(src[324:648] - 81, ko.oracle(ko.lattice9((0.1, 0.3)), 4)[1])
    assert {n: len(ao.batch_cells(m())) for n, m in ao.BATCHES.items()} == {n: 3 for n in ao.BATCHES}
    assert ao.batch_bounds(ao.BATCHES["two_sets"]()).shape == (5, 2, 2)
