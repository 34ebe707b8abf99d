"""GPU tier of the batched and the periodic k-nearest-neighbour graphs (graph_pde_amd.neighbor_graph: knn_csr_batched /
knn_graph_batched, knn_csr(period=...); csrc/gpde_knn_arms.hip).

Every comparison of graphs is torch.equal against tests/helpers/knn_arms_oracle.py, numpy float64 that never calls the code under
test: no case is excluded, no fairness filter, no tolerance - kernel and oracle evaluate the same float64 formula.  A batch is
also compared with a loop over the open knn_csr with offsets; every case runs under every cell edge and must give the same bits."""
import functools

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import neighbor_graph as ng, ops
from tests.helpers import batched_graphs as bg
from tests.helpers import knn_arms_oracle as ao
from tests.helpers import knn_oracle as ko
from tests.helpers import periodic_oracle as po

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


def _same(a, b):
    return torch.equal(a.rowptr, b.rowptr) and torch.equal(a.src, b.src) and torch.equal(a.dst, b.dst)


def _assert_csr(csr, rowptr, src, dst):
    assert csr.n_nodes == len(rowptr) - 1 and csr.n_edges == len(src)
    assert csr.rowptr.dtype == csr.src.dtype == csr.dst.dtype == csr.perm.dtype == torch.int32
    assert torch.equal(csr.rowptr.cpu().long(), torch.from_numpy(rowptr))
    assert torch.equal(csr.src.cpu().long(), torch.from_numpy(src))
    assert torch.equal(csr.dst.cpu().long(), torch.from_numpy(dst))
    assert torch.equal(csr.perm.cpu().long(), torch.arange(len(src)))


def _net(k0, hidden, out):
    return torch.nn.Sequential(torch.nn.Linear(k0, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, out))


def _train_step(conv, x, graph, ea, g):
    conv.zero_grad()
    xs = x.clone().requires_grad_(True)
    y = conv(xs, graph, ea)
    (y * g).sum().backward()
    return [y.detach(), xs.grad.clone()] + [p.grad.clone() for p in conv.parameters()]


def _module_agrees(csr, pos, seed):
    """NNConv_old(64, 64): output and gradients on the Csr are those on its edge_index."""
    d, n = pos.device, csr.n_nodes
    torch.manual_seed(seed)
    conv = gp.NNConv_old(64, 64, _net(2 * pos.size(1), 32, 64 * 64), aggr="mean").to(d)
    x, g = torch.randn(n, 64, device=d), torch.randn(n, 64, device=d)
    ei = csr.edge_index
    ea = torch.cat([pos[ei[0]], pos[ei[1]]], dim=1).float()
    a, b = _train_step(conv, x, csr, ea, g), _train_step(conv, x, ei, ea, g)
    assert len(a) == len(b) >= 4
    for i, (u, v) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v), i


# ---- batches ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(name):
    return ao.BATCHES[name]()


@functools.lru_cache(maxsize=None)
def _batch_oracle(name, k, loop):
    c = _batch(name)
    rowptr, src, dst, edge_ptr = ao.batched(c["pos"], c["ptr"], k, c.get("pos_dst"), c.get("ptr_dst"), loop)
    dim = c["pos"].shape[1]
    geom = ko.geometry(c["pos"], c.get("pos_dst"), src, dst) if len(src) else np.zeros((0, dim + 1), dtype=np.float32)
    return rowptr, src, dst, edge_ptr, geom.reshape(len(src), dim + 1)


def _batch_kw(c, d, cell=None, bounds=False):
    kw = {}
    if "pos_dst" in c:
        kw.update(pos_dst=_t(c["pos_dst"], d), ptr_dst=torch.from_numpy(c["ptr_dst"]))
    if cell is not None:
        kw["cell_size"] = cell
    if bounds:
        kw["bounds"] = ao.batch_bounds(c)
    return kw


def _loop_over_knn_csr(c, d, k, loop):
    """The existing single-graph builder, one call per graph, concatenated with the graphs' offsets (device tensors)."""
    ptr, pd = c["ptr"], c.get("ptr_dst", c["ptr"])
    rowptr, src, dst, geom, off = [torch.zeros(1, dtype=torch.int32, device=d)], [], [], [], 0
    for b in range(len(ptr) - 1):
        ps = _t(c["pos"][ptr[b]:ptr[b + 1]], d)
        pdst = _t(c["pos_dst"][pd[b]:pd[b + 1]], d) if "pos_dst" in c else None
        csr, g = ng.knn_csr(ps, k, pos_dst=pdst, loop=loop, return_geometry=True)
        rowptr.append(csr.rowptr[1:] + off)
        src.append(csr.src + int(ptr[b]))
        dst.append(csr.dst + int(pd[b]))
        geom.append(g)
        off += csr.n_edges
    dim = c["pos"].shape[1]
    cat = lambda parts, empty: torch.cat(parts) if parts else empty
    return (torch.cat(rowptr), cat(src, torch.zeros(0, dtype=torch.int32, device=d)), cat(dst, torch.zeros(0, dtype=torch.int32, device=d)),
            cat(geom, torch.zeros(0, dim + 1, device=d)))


BATCH_PARAMS = [(name, k, loop) for name, make in ao.BATCHES.items() for c in (make(),) for k in c["ks"] for loop in c["loops"]]


@pytest.mark.parametrize("name,k,loop", BATCH_PARAMS)
def test_a_batch_is_its_graphs_concatenated_bit_for_bit(name, k, loop):
    d = _dev()
    c = _batch(name)
    pos, ptr = _t(c["pos"], d), torch.from_numpy(c["ptr"])
    rowptr, src, dst, edge_ptr, geom = _batch_oracle(name, k, loop)
    one = "pos_dst" not in c
    ke = ao.batch_k_eff(c["ptr"], k, one, loop)
    lrow, lsrc, ldst, lgeom = _loop_over_knn_csr(c, d, k, loop)
    for cell in ao.batch_cells(c):
        for bounds in (False, True):
            csr, ep, g = ng.knn_csr_batched(pos, ptr, k, loop=loop, return_geometry=True, **_batch_kw(c, d, cell, bounds))
            _assert_csr(csr, rowptr, src, dst)
            assert csr.n_src_nodes == (None if one else len(c["pos"])) and csr.max_in_degree == (max(ke, default=0) if len(src) else 0)
            assert ep.dtype == torch.int64 and torch.equal(ep.cpu(), torch.from_numpy(edge_ptr))
            assert torch.equal(ep, csr.rowptr.long()[torch.from_numpy(c.get("ptr_dst", c["ptr"])).to(d)])
            assert g.dtype == torch.float32 and torch.equal(g.cpu(), torch.from_numpy(geom))
            # the loop over the open builder
            assert torch.equal(csr.rowptr, lrow) and torch.equal(csr.src, lsrc) and torch.equal(csr.dst, ldst) and torch.equal(g, lgeom)
    # the source-major edge list: the collated per-graph knn_graph lists
    ei, ep = ng.knn_graph_batched(pos, ptr, k, loop=loop, **_batch_kw(c, d))
    pd = c.get("ptr_dst", c["ptr"])
    lists = []
    for b in range(len(c["ptr"]) - 1):
        ps = _t(c["pos"][c["ptr"][b]:c["ptr"][b + 1]], d)
        pdst = _t(c["pos_dst"][pd[b]:pd[b + 1]], d) if not one else None
        lists.append(ng.knn_graph(ps, k, pos_dst=pdst, loop=loop).cpu().numpy())
    want, want_ptr = bg.assemble_edge_index(lists, c["ptr"], c.get("ptr_dst"))
    assert ei.dtype == torch.int64 and torch.equal(ei.cpu(), torch.from_numpy(want)) and torch.equal(ep.cpu(), torch.from_numpy(want_ptr))


def test_one_graph_is_knn_csr():
    d = _dev()
    c = _batch("b1")
    pos = _t(c["pos"], d)
    for k, loop in ((16, False), (200, True)):
        ref, gref = ng.knn_csr(pos, k, loop=loop, return_geometry=True)
        csr, ep, g = ng.knn_csr_batched(pos, [0, 130], k, loop=loop, return_geometry=True)
        assert _same(csr, ref) and torch.equal(g, gref) and ep.tolist() == [0, ref.n_edges] and csr.max_in_degree == ref.max_in_degree


def test_no_graphs_and_graphs_without_edges():
    d = _dev()
    none = torch.zeros(0, 2, device=d, dtype=torch.float64)
    for kw in (dict(), dict(bounds=np.zeros((0, 2, 2)))):
        csr, ep, g = ng.knn_csr_batched(none, [0], 3, return_geometry=True, **kw)
        assert csr.n_nodes == 0 and csr.n_edges == 0 and ep.tolist() == [0] and tuple(g.shape) == (0, 3) and csr.rowptr.tolist() == [0]
        ei, ep = ng.knn_graph_batched(none, [0], 3, **kw)
        assert tuple(ei.shape) == (2, 0) and ep.tolist() == [0]
    one = torch.rand(3, 2, device=d, dtype=torch.float64)               # three graphs of one point: no neighbour anywhere
    csr, ep = ng.knn_csr_batched(one, [0, 1, 2, 3], 4)
    assert csr.n_nodes == 3 and csr.n_edges == 0 and ep.tolist() == [0, 0, 0, 0] and csr.rowptr.tolist() == [0, 0, 0, 0] and csr.max_in_degree == 0


def test_with_bounds_given_the_batched_build_never_synchronises():
    d = _dev()
    c, t = _batch("unit_box"), _batch("two_sets")
    pos, ptr = _t(c["pos"], d), torch.from_numpy(c["ptr"])
    kw2 = _batch_kw(t, d, bounds=True)
    ng.knn_csr_batched(pos, ptr, 5, bounds=ao.batch_bounds(c))          # (the library is loaded, the kernels' code objects too)
    torch.cuda.synchronize(d)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one, ep1, g1 = ng.knn_csr_batched(pos, ptr, 5, bounds=ao.batch_bounds(c), return_geometry=True)
        two, ep2 = ng.knn_csr_batched(pos, ptr, 64, cell_size=0.05, **kw2)
        ei, _ = ng.knn_graph_batched(pos, ptr, 5, loop=True, bounds=ao.batch_bounds(c))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _assert_csr(one, *_batch_oracle("unit_box", 5, False)[:3])
    _assert_csr(two, *_batch_oracle("two_sets", 64, False)[:3])
    assert tuple(ei.shape) == (2, int(_batch_oracle("unit_box", 5, True)[3][-1]))


def test_two_batched_calls_and_a_side_stream_give_identical_tensors():
    d = _dev()
    c = _batch("unit_box")
    pos, ptr = _t(c["pos"], d), torch.from_numpy(c["ptr"])
    ref, ep, gref = ng.knn_csr_batched(pos, ptr, 64, return_geometry=True)
    again, ep2, gagain = ng.knn_csr_batched(pos, ptr, 64, return_geometry=True)
    torch.cuda.synchronize(d)
    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        csr, ep3, geom = ng.knn_csr_batched(pos, ptr, 64, return_geometry=True)
        boxed, ep4, gboxed = ng.knn_csr_batched(pos, ptr, 64, return_geometry=True, bounds=ao.batch_bounds(c))
    side.synchronize()
    for got, e, g in ((again, ep2, gagain), (csr, ep3, geom), (boxed, ep4, gboxed)):
        assert _same(got, ref) and torch.equal(e, ep) and torch.equal(g, gref)
    _assert_csr(csr, *_batch_oracle("unit_box", 64, False)[:3])


def test_the_operator_consumes_the_batched_csr():
    d = _dev()
    c = _batch("unit_box")
    pos = _t(c["pos"], d)
    csr, _ = ng.knn_csr_batched(pos, torch.from_numpy(c["ptr"]), 8)
    assert csr.n_edges == 8 * (37 + 64 + 130)
    _module_agrees(csr, pos, 45)


# ---- the torus -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pcase(name):
    if name == "outside_box_2^20":
        return ao.outside_scaled()
    if name == "lattice16":
        return dict(xs=po.lattice16(), period=1.0)
    return po.CASES[name]()


@functools.lru_cache(maxsize=None)
def _poracle(name, k, loop):
    c = _pcase(name)
    rowptr, src, dst = ao.periodic(c["xs"], k, c["period"], c.get("xd"), loop)
    return rowptr, src, dst, ao.periodic_geometry(c["xs"], c.get("xd"), src, dst, c["period"])


def _pkw(c, d, cell=None):
    kw = dict(period=c["period"])
    if "origin" in c:
        kw["origin"] = c["origin"]
    if "xd" in c:
        kw["pos_dst"] = _t(c["xd"], d)
    if cell is not None:
        kw["cell_size"] = cell
    return kw


def _periodic_case_under_every_cell(name, ks):
    d = _dev()
    c = _pcase(name)
    pos = _t(c["xs"], d)
    n_src = len(c["xs"])
    for k in ks:
        for loop in ((False,) if "xd" in c else (False, True)):
            rowptr, src, dst, geom = _poracle(name, k, loop)
            for cell in ao.periodic_cells(c):
                csr, g = ng.knn_csr(pos, k, loop=loop, return_geometry=True, **_pkw(c, d, cell))
                _assert_csr(csr, rowptr, src, dst)
                assert csr.n_src_nodes == (n_src if "xd" in c else None)
                assert csr.max_in_degree == (ko.k_eff(k, n_src, "xd" not in c, loop) if len(src) else 0)
                assert g.dtype == torch.float32 and torch.equal(g.cpu(), torch.from_numpy(geom)), (k, loop, cell)
                assert int(torch.unique(csr.src.long() + n_src * csr.dst.long()).numel()) == csr.n_edges        # no source twice in a row


@pytest.mark.parametrize("name", list(po.CASES))
def test_the_torus_edge_for_edge_against_the_oracle_under_every_cell_size(name):
    _periodic_case_under_every_cell(name, ao.periodic_ks(_pcase(name)))


def test_the_dyadic_lattice_whole_shells_of_equal_keys_and_pairs_at_half_a_period():
    _periodic_case_under_every_cell("lattice16", (1, 4, 8, 9, 24, 255, 256))


def test_points_two_to_the_twenty_periods_outside_the_box():
    _periodic_case_under_every_cell("outside_box_2^20", (1, 8, 64))


def test_the_graph_does_not_depend_on_the_origin_or_the_box():
    d = _dev()
    for name in ("2d_nc3", "outside_box", "3d_open_y"):
        c = _pcase(name)
        pos = _t(c["xs"], d)
        dim = pos.size(1)
        ref, gref = ng.knn_csr(pos, 8, period=c["period"], return_geometry=True)
        for origin in (0.37, [-5.25, 3.0, 1e3][:dim]):
            csr, g = ng.knn_csr(pos, 8, period=c["period"], origin=origin, return_geometry=True)
            assert _same(csr, ref) and torch.equal(g, gref)
        csr, g = ng.knn_csr(pos, 8, period=c["period"], bounds=(-7.0, 11.0), return_geometry=True)
        assert _same(csr, ref) and torch.equal(g, gref)
        _assert_csr(ref, *_poracle(name, 8, False)[:3])


def test_a_period_far_larger_than_the_cloud_gives_the_open_graph():
    d = _dev()
    for name, k in (("clustered", 16), ("two_sets", 9), ("3d_200", 7), ("1d_200", 7)):
        c = ko.CASES[name]()
        pos = _t(c["xs"], d)
        pd = _t(c["xd"], d) if "xd" in c else None
        assert _same(ng.knn_csr(pos, k, pos_dst=pd, period=1000.0), ng.knn_csr(pos, k, pos_dst=pd))
        assert torch.equal(ng.knn_graph(pos, k, pos_dst=pd, period=1000.0), ng.knn_graph(pos, k, pos_dst=pd))
        assert _same(ng.knn_csr(pos, k, pos_dst=pd, period=0.0), ng.knn_csr(pos, k, pos_dst=pd))        # no axis wraps: the open arm itself


def test_one_point_two_points_and_empty_sets_on_the_torus():
    d = _dev()
    x = torch.tensor([[0.95, 0.5], [0.05, 0.5]], device=d, dtype=torch.float64)
    csr, g = ng.knn_csr(x, 3, period=1.0, return_geometry=True)
    assert csr.src.tolist() == [1, 0] and csr.rowptr.tolist() == [0, 1, 2]
    want = ao.periodic_geometry(x.cpu().numpy(), None, np.array([1, 0]), np.array([0, 1]), 1.0)
    assert torch.equal(g.cpu(), torch.from_numpy(want)) and abs(float(g[0, 0]) - 0.1) < 1e-6           # across the seam, not 0.9 back
    assert ng.knn_csr(x, 3, period=1.0, loop=True).src.tolist() == [0, 1, 0, 1]
    one = ng.knn_csr(x[:1], 2, period=1.0)
    assert one.n_edges == 0 and one.rowptr.tolist() == [0, 0]
    assert ng.knn_csr(x[:1], 2, period=1.0, loop=True).src.tolist() == [0]
    none = torch.zeros(0, 2, device=d, dtype=torch.float64)
    for p, pd, n_dst in ((none, None, 0), (x, none, 0), (none, x, 2)):
        csr, g = ng.knn_csr(p, 3, pos_dst=pd, period=(1.0, 0.0), return_geometry=True)
        assert csr.n_edges == 0 and csr.n_nodes == n_dst and tuple(g.shape) == (0, 3) and csr.max_in_degree == 0
        assert torch.equal(csr.rowptr, torch.zeros(n_dst + 1, dtype=torch.int32, device=d))
        assert ng.knn_graph(p, 3, pos_dst=pd, period=1.0).shape == (2, 0)


def test_the_edge_list_and_the_selection_of_the_complete_graph():
    """knn_graph in source-major order, and the statement of the contract itself: select_in_edges on the complete bipartite graph
    under edge_sqdist_keys(period=...)."""
    d = _dev()
    c = _pcase("2d_nc4")
    pos = _t(c["xs"], d)
    n = pos.size(0)
    rowptr, src, dst, _ = _poracle("2d_nc4", 8, False)
    order = np.lexsort((dst, src))
    ei = ng.knn_graph(pos, 8, period=1.0)
    assert ei.dtype == torch.int64 and torch.equal(ei.cpu(), torch.from_numpy(np.stack([src[order], dst[order]])))
    s, t = torch.meshgrid(torch.arange(n, device=d), torch.arange(n, device=d), indexing="ij")
    full = ops.build_csr(torch.stack([s.reshape(-1), t.reshape(-1)]), n)
    cut, _ = ops.select_in_edges(full, 8, ops.edge_sqdist_keys(full, pos, period=1.0))
    assert _same(ng.knn_csr(pos, 8, period=1.0, loop=True), cut)


def test_geometry_agrees_with_the_periodic_radius_builder_to_its_last_bits():
    d = _dev()
    c = _pcase("2d_nc7")                                             # r = 0.13: 2 r < period
    pos = _t(c["xs"], d)
    n = pos.size(0)
    knn, g = ng.knn_csr(pos, 8, period=c["period"], return_geometry=True)
    rad, gr = ops.radius_csr(pos, c["r"], period=c["period"], return_geometry=True)
    kk, kr = knn.src.long() + n * knn.dst.long(), rad.src.long() + n * rad.dst.long()       # ascending in both: rows by dst, sources ascending
    at = torch.searchsorted(kr, kk).clamp(max=kr.numel() - 1)
    both = kr[at] == kk
    assert int(both.sum()) > 1000
    bound = torch.from_numpy(po.geom_bound(c["period"], c["r"], 2)).to(d)
    assert bool(((g[both].double() - gr[at[both]].double()).abs() <= bound).all())
    assert torch.equal(g.cpu(), torch.from_numpy(_poracle("2d_nc7", 8, False)[3]))


def test_with_every_axis_periodic_the_build_never_synchronises():
    d = _dev()
    c = _pcase("two_sets")
    pos, pd = _t(c["xs"], d), _t(c["xd"], d)
    ng.knn_csr(pos, 8, period=1.0)                                    # (the library is loaded, the kernels' code objects too)
    torch.cuda.synchronize(d)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one, g1 = ng.knn_csr(pos, 8, period=1.0, return_geometry=True)
        two, g2 = ng.knn_csr(pos, 8, pos_dst=pd, period=(1.0, 1.0), origin=(0.25, -3.0), return_geometry=True, cell_size=0.05)
        ei = ng.knn_graph(pos, 8, period=1.0, loop=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(one.src.cpu().long(), torch.from_numpy(ao.periodic(c["xs"], 8, 1.0)[1]))
    assert torch.equal(two.src.cpu().long(), torch.from_numpy(_poracle("two_sets", 8, False)[1]))
    assert tuple(ei.shape) == (2, 150 * 8) and tuple(g1.shape) == (150 * 8, 3) and tuple(g2.shape) == (40 * 8, 3)


def test_two_periodic_calls_and_a_side_stream_give_identical_tensors():
    d = _dev()
    c = _pcase("outside_box")
    pos = _t(c["xs"], d)
    ref, gref = ng.knn_csr(pos, 64, period=1.0, return_geometry=True)
    again, gagain = ng.knn_csr(pos, 64, period=1.0, return_geometry=True)
    torch.cuda.synchronize(d)
    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        csr, geom = ng.knn_csr(pos, 64, period=1.0, return_geometry=True)
    side.synchronize()
    for got, g in ((again, gagain), (csr, geom)):
        assert _same(got, ref) and torch.equal(g, gref)


def test_the_operator_consumes_the_periodic_csr():
    d = _dev()
    c = _pcase("2d_nc4")
    pos = _t(c["xs"], d)
    csr = ng.knn_csr(pos, 8, period=1.0)
    assert csr.n_edges == 300 * 8
    _module_agrees(csr, pos, 46)
