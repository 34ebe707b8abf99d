"""GPU tier of the k-nearest-neighbour graphs (graph_pde_amd.neighbor_graph; csrc/gpde_knn.hip; DESIGN.md §6e "The nearest arm").

Oracle 1 (tests/helpers/knn_oracle.py): the complete bipartite edge list in numpy float64, keys by neighbor_cap.d2_open / d2_bits,
rows cut by neighbor_cap.select.  Oracle 2, for loop=True and two point sets: ops.radius_csr(pos, R, max_num_neighbors=k,
select="nearest", return_geometry=True) with R twice the box diagonal.  Every comparison is torch.equal; every case runs under
every cell edge of knn_oracle.cell_sizes and must give the same bits."""
import functools

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import neighbor_graph as ng, ops
from tests.helpers import knn_oracle as ko

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.ascontiguousarray(a)).to(d)


@functools.lru_cache(maxsize=None)
def _case(name):
    return (ko.CASES.get(name) or ko.LARGE[name])()


@functools.lru_cache(maxsize=None)
def _oracle(name, k, loop):
    c = _case(name)
    return ko.oracle(c["xs"], k, c.get("xd"), loop)


def _kw(c, d, cell=None):
    kw = {}
    if "xd" in c:
        kw["pos_dst"] = _t(c["xd"], d)
    if "bounds" in c:
        kw["bounds"] = c["bounds"]
    if cell is not None:
        kw["cell_size"] = cell
    return kw


def _assert_is_the_oracles(csr, c, k, loop, want):
    rowptr, src, dst = want
    n_dst = len(rowptr) - 1
    assert csr.n_nodes == n_dst and csr.n_edges == len(src)
    assert csr.rowptr.dtype == csr.src.dtype == csr.dst.dtype == csr.perm.dtype == torch.int32
    assert torch.equal(csr.rowptr.cpu().long(), torch.from_numpy(rowptr))
    assert torch.equal(csr.src.cpu().long(), torch.from_numpy(src))
    assert torch.equal(csr.dst.cpu().long(), torch.from_numpy(dst))
    assert torch.equal(csr.perm.cpu().long(), torch.arange(len(src)))
    assert csr.n_src_nodes == (len(c["xs"]) if "xd" in c else None)
    assert csr.max_in_degree == ko.k_eff(k, len(c["xs"]), "xd" not in c, loop)


@pytest.mark.parametrize("name,k,loop", ko.params(ko.CASES))
def test_edge_for_edge_against_the_oracle_under_every_cell_size(name, k, loop):
    d = _dev()
    c = _case(name)
    pos = _t(c["xs"], d)
    for cell in ko.cell_sizes(c):
        csr = ng.knn_csr(pos, k, loop=loop, **_kw(c, d, cell))
        _assert_is_the_oracles(csr, c, k, loop, _oracle(name, k, loop))


@pytest.mark.parametrize("name", list(ko.LARGE))
def test_one_larger_cloud(name):
    d = _dev()
    c = _case(name)
    k = c["ks"][0]
    csr, geom = ng.knn_csr(_t(c["xs"], d), k, return_geometry=True)
    want = _oracle(name, k, False)
    _assert_is_the_oracles(csr, c, k, False, want)
    assert torch.equal(geom.cpu(), torch.from_numpy(ko.geometry(c["xs"], None, want[1], want[2])))


@pytest.mark.parametrize("name,k,loop", [(n, k, l) for n, k, l in ko.params(ko.CASES) if l or "xd" in ko.CASES[n]()])
def test_the_capped_radius_graph_of_the_whole_box_is_the_same_graph(name, k, loop):
    """Oracle 2: CSR and geometry rows of radius_csr(..., max_num_neighbors=k, select="nearest") at a radius that holds everything."""
    d = _dev()
    c = _case(name)
    pos = _t(c["xs"], d)
    pts = np.concatenate([ko.as2d(c["xs"]), ko.as2d(c["xd"])]) if "xd" in c else ko.as2d(c["xs"])
    R = 2.0 * float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0))) or 1.0
    ref, gref = ops.radius_csr(pos, R, pos_dst=_kw(c, d).get("pos_dst"), max_num_neighbors=k, select="nearest", return_geometry=True)
    for cell in ko.cell_sizes(c):
        csr, geom = ng.knn_csr(pos, k, loop=loop, return_geometry=True, **_kw(c, d, cell))
        assert torch.equal(csr.rowptr, ref.rowptr) and torch.equal(csr.src, ref.src) and torch.equal(csr.dst, ref.dst)
        assert geom.dtype == torch.float32 and torch.equal(geom, gref)


def test_geometry_and_edge_list_without_self_loops():
    d = _dev()
    c = _case("clustered")
    pos = _t(c["xs"], d)
    want = _oracle("clustered", 16, False)
    csr, geom = ng.knn_csr(pos, 16, return_geometry=True)
    assert tuple(geom.shape) == (csr.n_edges, 3) and torch.equal(geom.cpu(), torch.from_numpy(ko.geometry(c["xs"], None, want[1], want[2])))
    ei = ng.knn_graph(pos, 16)
    order = np.lexsort((want[2], want[1]))                           # source-major, targets ascending: the order of radius_graph
    assert ei.dtype == torch.int64 and torch.equal(ei.cpu(), torch.from_numpy(np.stack([want[1][order], want[2][order]])))
    assert torch.equal(csr.edge_index, torch.stack([csr.src.long(), csr.dst.long()]))


def test_empty_point_sets_and_rows_without_edges():
    d = _dev()
    pos, none = torch.rand(7, 2, device=d, dtype=torch.float64), torch.zeros(0, 2, device=d, dtype=torch.float64)
    for p, pd, n_dst in ((none, None, 0), (pos, none, 0), (none, pos, 7), (pos[:1], None, 1)):
        for kw in (dict(), dict(bounds=(0.0, 1.0))):
            csr, geom = ng.knn_csr(p, 3, pos_dst=pd, return_geometry=True, **kw)
            assert csr.n_edges == 0 and csr.n_nodes == n_dst and tuple(geom.shape) == (0, 3) and csr.max_in_degree == 0
            assert torch.equal(csr.rowptr, torch.zeros(n_dst + 1, dtype=torch.int32, device=d))
            assert ng.knn_graph(p, 3, pos_dst=pd, **kw).shape == (2, 0)


def test_two_calls_and_a_side_stream_give_identical_tensors():
    d = _dev()
    c = _case("clustered")
    pos = _t(c["xs"], d)
    ref, gref = ng.knn_csr(pos, 64, return_geometry=True)
    again, gagain = ng.knn_csr(pos, 64, return_geometry=True)
    torch.cuda.synchronize(d)
    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        csr, geom = ng.knn_csr(pos, 64, return_geometry=True)
        boxed, gboxed = ng.knn_csr(pos, 64, return_geometry=True, bounds=(0.0, 1.0))
    side.synchronize()
    for got, g in ((again, gagain), (csr, geom), (boxed, gboxed)):
        assert torch.equal(got.rowptr, ref.rowptr) and torch.equal(got.src, ref.src) and torch.equal(got.dst, ref.dst) and torch.equal(g, gref)
    _assert_is_the_oracles(csr, c, 64, False, _oracle("clustered", 64, False))


def test_a_build_queued_behind_its_producer_on_a_held_side_stream():
    """The pattern of tests/helpers/streams.py: the positions are produced on a side stream that is held busy, and the build is
    issued there before they exist.  Every launch of the call must be queued on that stream: one that ran elsewhere would read
    the zero-filled pool (all points at the origin - valid ids, another graph)."""
    from tests.helpers import streams as st
    d = _dev()
    c = _case("two_sets")
    given, pd = _t(c["xs"], d), _t(c["xd"], d)
    ref, gref = ng.knn_csr(given, 9, pos_dst=pd, bounds=(0.0, 1.0), return_geometry=True)
    side = torch.cuda.Stream(d)
    st.zeroed_pool(side)
    done = st.hold(side, 50.0)
    with torch.cuda.stream(side):
        pos = given + 0.0                                           # written behind the hold
        csr, geom = ng.knn_csr(pos, 9, pos_dst=pd, bounds=(0.0, 1.0), return_geometry=True)
        still_held = not done.query()
    side.synchronize()
    assert still_held, "the call was issued after the hold ran out: this run raced nothing"
    assert torch.equal(csr.rowptr, ref.rowptr) and torch.equal(csr.src, ref.src) and torch.equal(csr.dst, ref.dst) and torch.equal(geom, gref)


def test_with_bounds_given_the_build_never_synchronises():
    d = _dev()
    c = _case("two_sets")
    pos, pd = _t(c["xs"], d), _t(c["xd"], d)
    ng.knn_csr(pos, 9, bounds=(0.0, 1.0))                             # (the library is loaded, the kernels' code objects too)
    torch.cuda.synchronize(d)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one, g1 = ng.knn_csr(pos, 9, bounds=(0.0, 1.0), return_geometry=True)
        two, g2 = ng.knn_csr(pos, 9, pos_dst=pd, bounds=((0.0, 0.0), (1.0, 1.0)), return_geometry=True, cell_size=0.05)
        ei = ng.knn_graph(pos, 9, bounds=(0.0, 1.0), loop=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(one.src.cpu().long(), torch.from_numpy(ko.oracle(c["xs"], 9)[1]))
    assert torch.equal(two.src.cpu().long(), torch.from_numpy(_oracle("two_sets", 9, False)[1]))
    assert tuple(ei.shape) == (2, 150 * 9) and tuple(g1.shape) == (150 * 9, 3) and tuple(g2.shape) == (40 * 9, 3)


def _net(k0, hidden, out):
    """A small Linear / ReLU kernel network."""
    return torch.nn.Sequential(torch.nn.Linear(k0, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, out))


def _train_step(conv, x, graph, ea, g):
    conv.zero_grad()
    xs = tuple(t.clone().requires_grad_(True) for t in x) if isinstance(x, tuple) else x.clone().requires_grad_(True)
    y = conv(xs, graph, ea)
    (y * g).sum().backward()
    leaves = xs if isinstance(xs, tuple) else (xs,)
    return [y.detach()] + [t.grad.clone() for t in leaves] + [p.grad.clone() for p in conv.parameters()]


@pytest.mark.parametrize("module", ["NNConv_old_64_64", "NNConv_24_40"])
def test_the_operator_consumes_the_csr(module):
    d, n, k = _dev(), 200, 8
    torch.manual_seed(43)
    pos = torch.rand(n, 2, device=d, dtype=torch.float64)
    csr = ng.knn_csr(pos, k)
    assert csr.n_edges == n * k
    cin, cout = (64, 64) if module == "NNConv_old_64_64" else (24, 40)
    net = _net(4, 32 if cin == 64 else 16, cin * cout)
    conv = (gp.NNConv_old if cin == 64 else gp.NNConv)(cin, cout, net, aggr="mean").to(d)
    x, g = torch.randn(n, cin, device=d), torch.randn(n, cout, device=d)
    ei = csr.edge_index
    ea = torch.cat([pos[ei[0]], pos[ei[1]]], dim=1).float()
    a, b = _train_step(conv, x, csr, ea, g), _train_step(conv, x, ei, ea, g)
    assert len(a) == len(b) >= 4
    for i, (u, v) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v), i


def test_the_operator_consumes_a_two_set_graph():
    d, n_src, n_dst, k, cin, cout = _dev(), 150, 40, 8, 24, 40
    c = _case("two_sets")
    ps, pd = _t(c["xs"], d), _t(c["xd"], d)
    csr = ng.knn_csr(ps, k, pos_dst=pd)
    assert csr.n_src_nodes == n_src and csr.n_nodes == n_dst and csr.n_edges == n_dst * k
    torch.manual_seed(44)
    conv = gp.NNConv(cin, cout, _net(4, 16, cin * cout), aggr="mean").to(d)
    xs, xd, g = torch.randn(n_src, cin, device=d), torch.randn(n_dst, cin, device=d), torch.randn(n_dst, cout, device=d)
    ei = csr.edge_index
    ea = torch.cat([ps[ei[0]], pd[ei[1]]], dim=1).float()
    a, b = _train_step(conv, (xs, xd), csr, ea, g), _train_step(conv, (xs, xd), ei, ea, g)
    assert a[0].shape == (n_dst, cout)
    for i, (u, v) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v), i
