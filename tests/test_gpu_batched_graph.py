"""GPU tier: the radius graphs of a batch of point sets in one build (gpde_radius_csr_batched_*, ops.radius_csr_batched /
radius_graph_batched).  Integer work: equality is the only bar.  Expected values come from code that is not under test - the
single-graph builders called once per graph, and the CPU oracle - put together by tests/helpers/batched_graphs.py, whose
assembly the CPU tier pins (tests/test_batched_graph_host.py)."""
import os

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, rel_l2
from tests.conftest import GOLDEN
from tests.helpers import batched_graphs as bg

pytestmark = pytest.mark.gpu

CG_SORT_MAX = 4096          # csrc/gpde_cellgraph.hip: longer rows keep cell order


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _per_graph_csr(pos, ptr, radii, ties, pos_dst=None, ptr_dst=None):
    """The single-graph builder once per graph, assembled: (rowptr, src, dst, edge_ptr) as int64 numpy."""
    per = []
    for b in range(len(ptr) - 1):
        s = _dev(pos[ptr[b]:ptr[b + 1]])
        d = None if pos_dst is None else _dev(pos_dst[ptr_dst[b]:ptr_dst[b + 1]])
        per.append(tuple(t.cpu().numpy() for t in ops.radius_csr_raw(s, float(radii[b]), ties, pos_dst=d)))
    return bg.assemble_csr(per, ptr, ptr_dst)


def _batched(pos, ptr, radii, ties, pos_dst=None, ptr_dst=None):
    """(Csr, edge_ptr, (rowptr, src, dst, edge_ptr) as int64 numpy) of the call under test."""
    csr, edge_ptr = ops.radius_csr_batched(_dev(pos), torch.from_numpy(ptr), radii, pos_dst=None if pos_dst is None else _dev(pos_dst),
                                           ptr_dst=None if ptr_dst is None else torch.from_numpy(ptr_dst), reference_ties=ties)
    assert csr.rowptr.dtype == csr.src.dtype == csr.dst.dtype == torch.int32 and edge_ptr.dtype == torch.int64
    assert csr.n_nodes == csr.rowptr.numel() - 1 and csr.n_edges == csr.src.numel() == csr.dst.numel()
    assert torch.equal(csr.perm.long(), torch.arange(csr.n_edges, device=csr.perm.device))
    return csr, edge_ptr, tuple(t.cpu().numpy().astype(np.int64) for t in (csr.rowptr, csr.src, csr.dst, edge_ptr))


def _assert_same(got, want, what):
    for name, g, w in zip(("rowptr", "src", "dst", "edge_ptr"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)


def _check(pos, ptr, radii, ties, pos_dst=None, ptr_dst=None, what=""):
    """The batched CSR == the per-graph builder == the CPU oracle, bit for bit; no edge leaves its graph."""
    csr, edge_ptr, got = _batched(pos, ptr, radii, ties, pos_dst, ptr_dst)
    _assert_same(got, _per_graph_csr(pos, ptr, radii, ties, pos_dst, ptr_dst), (what, "per-graph builder"))
    _assert_same(got, bg.oracle_csr(pos, ptr, radii, pos_dst, ptr_dst, reference_ties=ties), (what, "oracle"))
    pd = ptr if ptr_dst is None else ptr_dst
    rowptr, src, dst, ep = got
    assert np.array_equal(np.searchsorted(ptr[1:], src, side="right"), np.searchsorted(pd[1:], dst, side="right")), (what, "graph(src) == graph(dst)")
    assert np.array_equal(ep, rowptr[pd]), (what, "edge_ptr")
    assert csr.n_nodes == int(pd[-1]) and csr.n_src_nodes == (None if pos_dst is None else int(ptr[-1]))
    return csr, edge_ptr


@pytest.mark.parametrize("ties", [False, True])
def test_self_graphs_in_one_unit_box(ties):
    """Sizes [37, 0, 1, 64, 130] in [0, 1]^2, r = 0.2: every graph overlaps every other in coordinates."""
    pos, ptr = bg.unit_box_batch()
    csr, edge_ptr = _check(pos, ptr, [0.2] * 5, ties, what="unit box")
    assert edge_ptr.tolist()[0] == 0 and edge_ptr.tolist()[-1] == csr.n_edges and edge_ptr[2] == edge_ptr[1]      # the empty graph
    csr2, _ = ops.radius_csr_batched(_dev(pos), ptr.tolist(), 0.2, reference_ties=ties)                            # r as a float, ptr as a list
    assert torch.equal(csr2.rowptr, csr.rowptr) and torch.equal(csr2.src, csr.src) and torch.equal(csr2.dst, csr.dst)


@pytest.mark.parametrize("ties", [False, True])
def test_degenerate_batches(ties):
    rng = np.random.default_rng(5)
    d = torch.device("cuda:0")
    # B = 1 is ops.radius_csr
    p = rng.random((300, 2))
    p[::7] = np.round(p[::7] * 8) / 8
    one, edge_ptr = ops.radius_csr_batched(_dev(p), torch.tensor([0, 300]), [0.11], reference_ties=ties)
    ref = ops.radius_csr(_dev(p), 0.11, reference_ties=ties)
    assert torch.equal(one.rowptr, ref.rowptr) and torch.equal(one.src, ref.src) and torch.equal(one.dst, ref.dst)
    assert edge_ptr.tolist() == [0, ref.n_edges] and one.n_nodes == ref.n_nodes and one.n_src_nodes is None
    # B = 0
    none, edge_ptr = ops.radius_csr_batched(torch.zeros(0, 2, dtype=torch.float64, device=d), torch.tensor([0]), 0.1, reference_ties=ties)
    assert (none.n_nodes, none.n_edges, none.rowptr.tolist(), edge_ptr.tolist()) == (0, 0, [0], [0])
    # all graphs empty
    none, edge_ptr = ops.radius_csr_batched(torch.zeros(0, 3, dtype=torch.float64, device=d), torch.tensor([0, 0, 0, 0]), [0.1, 0.2, 0.3],
                                            reference_ties=ties)
    assert (none.n_nodes, none.n_edges, none.rowptr.tolist(), edge_ptr.tolist()) == (0, 0, [0], [0, 0, 0, 0])
    # empty first and last graph
    pos, ptr = bg.concat_sets([np.zeros((0, 2)), rng.random((40, 2)), rng.random((9, 2)), np.zeros((0, 2))])
    _check(pos, ptr, [0.3, 0.2, 0.5, 0.1], ties, what="empty first and last")
    # one and three dimensions
    pos, ptr = bg.concat_sets([rng.random((200, 1)) * 3.0 - 1.0, rng.random((1, 1)), rng.random((77, 1))])
    _check(pos, ptr, [0.011, 0.5, 0.05], ties, what="1-D")
    csr, _ = ops.radius_csr_batched(_dev(pos[:, 0]), ptr.tolist(), [0.011, 0.5, 0.05], reference_ties=ties)      # positions [n]
    assert csr.n_edges == int(bg.oracle_csr(pos, ptr, [0.011, 0.5, 0.05], reference_ties=ties)[3][-1])
    pos, ptr = bg.concat_sets([rng.random((150, 3)), rng.random((260, 3)) * [1.0, 0.2, 3.0]])
    _check(pos, ptr, [0.3, 0.16], ties, what="3-D")


@pytest.mark.parametrize("ties", [False, True])
def test_per_graph_radii_and_boxes(ties):
    """Radii [0.05, 0.3, 0.11]; one graph in [0, 1]^2, one in [100, 100.001]^2 (every pair within r, coordinates where the
    dot-product arithmetic rounds), one whose points all coincide (extent 0: a one-cell grid)."""
    rng = np.random.default_rng(9)
    unit = rng.random((400, 2))
    unit[::7] = np.round(unit[::7] * 8) / 8
    far = 100.0 + 0.001 * rng.random((60, 2))
    same = np.tile([[0.25, 0.75]], (23, 1))
    pos, ptr = bg.concat_sets([unit, far, same])
    csr, edge_ptr = _check(pos, ptr, [0.05, 0.3, 0.11], ties, what="radii and boxes")
    e = edge_ptr.tolist()
    assert e[2] - e[1] == 60 * 60 and e[3] - e[2] == 23 * 23
    # a batch whose summed cells exceed the cap is coarsened: the grid is a filter, the edges are the same
    fine = [np.concatenate([0.5 + 1e-4 * rng.random((40, 2)), rng.random((10, 2)), [[0.0, 0.0], [1.0, 1.0]]]) for _ in range(6)]
    pos, ptr = bg.concat_sets(fine)
    alone = ops.batched_plan(torch.tensor([[[0.0, 0.0], [1.0, 1.0]]]), torch.tensor([0, 52]), None, [1.2e-4], 2)[1]
    together = ops.batched_plan(torch.tensor([[[0.0, 0.0], [1.0, 1.0]]] * 6), torch.from_numpy(ptr), None, [1.2e-4] * 6, 2)[1]
    assert 6 * alone > (1 << 24) >= together and together // 6 < alone         # each graph's grid is coarser in the batch than alone
    _check(pos, ptr, [1.2e-4] * 6, ties, what="coarsened")


def test_reference_ties_reproduce_the_pinned_lattice_graph_in_every_copy():
    """Two copies of the 31 x 31 lattice of tests/golden/mesh_ties.npz (the reference's own edge list: pairs at exactly distance r
    kept or dropped as scikit-learn does) and a random graph between them, under reference ties."""
    g = np.load(os.path.join(GOLDEN, "mesh_ties.npz"))
    r = float(g["r"])
    axis = np.linspace(0.0, 1.0, 31)
    lattice = np.vstack([xx.ravel() for xx in np.meshgrid(axis, axis)]).T
    rnd = np.random.default_rng(2).random((500, 2))
    pos, ptr = bg.concat_sets([lattice, rnd, lattice])
    pinned = g["edge_index_s31"].astype(np.int64)
    ei, edge_ptr = ops.radius_graph_batched(_dev(pos), torch.from_numpy(ptr), r, reference_ties=True)
    ei, e = ei.cpu().numpy(), edge_ptr.tolist()
    assert e[1] - e[0] == e[3] - e[2] == pinned.shape[1] == int(g["n_edges_s31"])
    assert np.array_equal(ei[:, e[0]:e[1]], pinned) and np.array_equal(ei[:, e[2]:e[3]] - ptr[2], pinned)
    assert np.array_equal(ei[:, e[1]:e[2]] - ptr[1], bg.oracle_edge_lists(rnd, np.array([0, 500]), [r], reference_ties=True)[0])
    csr, _, got = _batched(pos, ptr, [r] * 3, True)
    want = bg.assemble_csr([bg.csr_of_edges(pinned, 961), bg.csr_of_edges(ei[:, e[1]:e[2]] - ptr[1], 500), bg.csr_of_edges(pinned, 961)], ptr)
    _assert_same(got, want, "pinned CSR")
    exact = ops.radius_csr_batched(_dev(pos), torch.from_numpy(ptr), r)[0]
    assert exact.n_edges > csr.n_edges                               # the exact arithmetic keeps the lattice pairs at distance r


@pytest.mark.parametrize("ties", [False, True])
def test_two_point_sets(ties):
    """ptr and ptr_dst of different sizes; one graph with sources and no destinations, one with destinations and no sources."""
    rng = np.random.default_rng(13)
    srcs = [rng.random((120, 2)), rng.random((50, 2)), np.zeros((0, 2)), rng.random((33, 2)), rng.random((1, 2))]
    dsts = [rng.random((31, 2)), np.zeros((0, 2)), rng.random((17, 2)), rng.random((90, 2)), rng.random((5, 2)) * 3.0]
    srcs[0][::5] = np.round(srcs[0][::5] * 8) / 8
    dsts[0][::3] = np.round(dsts[0][::3] * 8) / 8
    ps, ptr = bg.concat_sets(srcs)
    pd, ptr_dst = bg.concat_sets(dsts)
    csr, edge_ptr = _check(ps, ptr, [0.25, 0.4, 0.3, 0.125, 1.5], ties, pd, ptr_dst, what="two sets")
    e = edge_ptr.tolist()
    assert e[1] == e[2] == e[3] and csr.n_src_nodes == 204 and csr.n_nodes == 143


def test_one_long_row_next_to_a_small_graph():
    """Two destinations of graph 0 have about 4,200 sources within r: rows above CG_SORT_MAX keep cell order and are compared
    after sorting the row; every other row is compared exactly."""
    rng = np.random.default_rng(17)
    cluster = 0.5 + 0.01 * (rng.random((4200, 2)) - 0.5)
    srcs = [np.concatenate([cluster, rng.random((300, 2))]), rng.random((50, 2))]
    dsts = [np.concatenate([[[0.5, 0.5], [0.501, 0.499]], rng.random((6, 2))]), rng.random((20, 2))]
    ps, ptr = bg.concat_sets(srcs)
    pd, ptr_dst = bg.concat_sets(dsts)
    radii = [0.05, 0.3]
    for ties in (False, True):
        _, _, got = _batched(ps, ptr, radii, ties, pd, ptr_dst)
        want = bg.oracle_csr(ps, ptr, radii, pd, ptr_dst, reference_ties=ties)
        per = _per_graph_csr(ps, ptr, radii, ties, pd, ptr_dst)
        rowptr = got[0]
        assert np.array_equal(rowptr, want[0]) and np.array_equal(rowptr, per[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        deg = np.diff(rowptr)
        assert (deg > CG_SORT_MAX).sum() == 2 and deg[0] > CG_SORT_MAX and deg[1] > CG_SORT_MAX
        for i in range(len(deg)):
            a, b = rowptr[i], rowptr[i + 1]
            if deg[i] > CG_SORT_MAX:
                assert np.array_equal(np.sort(got[1][a:b]), want[1][a:b]) and np.array_equal(np.sort(per[1][a:b]), want[1][a:b]), (ties, i)
            else:
                assert np.array_equal(got[1][a:b], want[1][a:b]) and np.array_equal(got[1][a:b], per[1][a:b]), (ties, i)


@pytest.mark.parametrize("ties", [False, True])
def test_radius_graph_batched_is_the_collated_per_graph_edge_lists(ties):
    rng = np.random.default_rng(21)
    pos, ptr = bg.unit_box_batch(sizes=(37, 0, 1, 64, 130), seed=4)
    radii = [0.2, 0.1, 0.3, 0.15, 0.11]
    per = [ops.radius_graph(_dev(pos[ptr[b]:ptr[b + 1]]), radii[b], reference_ties=ties).cpu().numpy() if ptr[b + 1] > ptr[b]
           else np.zeros((2, 0), dtype=np.int64) for b in range(5)]
    want, want_ptr = bg.assemble_edge_index(per, ptr)
    ei, edge_ptr = ops.radius_graph_batched(_dev(pos), torch.from_numpy(ptr), radii, reference_ties=ties)
    assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), want) and edge_ptr.tolist() == want_ptr.tolist()
    ps, ptr_s = bg.concat_sets([rng.random((60, 2)), rng.random((25, 2)), rng.random((4, 2))])
    pd, ptr_d = bg.concat_sets([rng.random((10, 2)), np.zeros((0, 2)), rng.random((30, 2))])
    per = [ops.radius_graph(_dev(ps[ptr_s[b]:ptr_s[b + 1]]), 0.3, reference_ties=ties, pos_dst=_dev(pd[ptr_d[b]:ptr_d[b + 1]])).cpu().numpy()
           if ptr_d[b + 1] > ptr_d[b] else np.zeros((2, 0), dtype=np.int64) for b in range(3)]
    want, want_ptr = bg.assemble_edge_index(per, ptr_s, ptr_d)
    ei, edge_ptr = ops.radius_graph_batched(_dev(ps), ptr_s.tolist(), 0.3, pos_dst=_dev(pd), ptr_dst=ptr_d.tolist(), reference_ties=ties)
    assert np.array_equal(ei.cpu().numpy(), want) and edge_ptr.tolist() == want_ptr.tolist()


def _slot_attr(csr, pos, a):
    """[E, 6] float32 by CSR slot: (pos[src], pos[dst], a[src], a[dst])."""
    s, t = csr.src.long(), csr.dst.long()
    return torch.cat([pos[s], pos[t], a[s].unsqueeze(1), a[t].unsqueeze(1)], dim=1).float().contiguous()


def test_operator_on_the_batched_csr():
    """The batched Csr is consumed as it is.  8 -> 8 'mean' inference: one wave per destination row, the order of the row's sum
    fixed by the row alone - the batched call is the concatenation of the per-graph calls bit for bit.  64 -> 64: within the
    forward bar of 1e-5 (relative L2) of the float64 oracle.

    At 8 -> 8 the per-edge weights are `nn(edge_attr)` by the caller's module: torch GEMMs, not this library.  torch picks its
    GEMM kernel by the row count, and the ONE-row product of the one-edge graph rounds differently from the same row inside the
    batch: measured on an MI355X, max |nn(ea_b) - nn(ea)[rows of b]| = 5.96e-08 for that graph and 0 for the graphs of 185, 468
    and 1,946 edges, which moves its output row by 2.4e-07.  So the operator is compared on EVERY graph given the same per-edge
    weights (rows of the batch's `nn(edge_attr)`: bit for bit, the one-edge and the empty graph included), and whole module calls
    - kernel network included - on every graph of more than one edge."""
    from tests.test_gpu_widths import DenseNet
    d = torch.device("cuda:0")
    torch.manual_seed(6)
    pos_np, ptr = bg.unit_box_batch(sizes=(37, 0, 1, 64, 130), seed=8)
    pos = _dev(pos_np)
    n = int(ptr[-1])
    a = torch.rand(n, dtype=torch.float64, device=d)
    csr, edge_ptr = ops.radius_csr_batched(pos, torch.from_numpy(ptr), 0.2)
    ep = edge_ptr.tolist()
    ea = _slot_attr(csr, pos, a)
    conv = gp.NNConv_old(8, 8, DenseNet([6, 16, 64]), aggr="mean").to(d)
    x = torch.randn(n, 8, device=d)
    with torch.no_grad():
        y = conv(x, csr, ea)
        w_e = conv.nn(ea).float().contiguous()
        assert y.shape == (n, 8) and torch.equal(y, ops.nnconv_forward_edgeweights_any_raw(x, csr, w_e, conv.root, conv.bias, "mean"))
        parts, module_calls = [], 0
        for b in range(len(ptr) - 1):
            lo, hi = int(ptr[b]), int(ptr[b + 1])
            if hi == lo:
                continue
            one = ops.radius_csr(pos[lo:hi], 0.2)
            ea_b = _slot_attr(one, pos[lo:hi], a[lo:hi])
            assert one.n_edges == ep[b + 1] - ep[b] and torch.equal(ea_b, ea[ep[b]:ep[b + 1]])
            parts.append(ops.nnconv_forward_edgeweights_any_raw(x[lo:hi].contiguous(), one, w_e[ep[b]:ep[b + 1]].contiguous(), conv.root, conv.bias, "mean"))
            if one.n_edges > 1:                            # (a one-row GEMM of the caller's module: see above)
                assert torch.equal(conv(x[lo:hi].contiguous(), one, ea_b), y[lo:hi]), b
                module_calls += 1
    assert torch.equal(y, torch.cat(parts)) and module_calls == 3
    mlp = torch.nn.Sequential(torch.nn.Linear(6, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 4096))
    conv = gp.NNConv_old(64, 64, mlp, aggr="mean").to(d)
    x = torch.randn(n, 64, device=d)
    with torch.no_grad():
        y = conv(x, csr, ea)
    lin = ops.mlp_linears(conv.nn)
    ref = nnconv_forward(x.cpu(), csr.edge_index.cpu(), ea.cpu(), [l.weight.detach().cpu() for l in lin], [l.bias.detach().cpu() for l in lin],
                         conv.root.detach().cpu(), conv.bias.detach().cpu(), aggr="mean", dtype=torch.float64)
    err = rel_l2(y, ref)
    print(f"64 -> 64 on the batched Csr (N = {n}, E = {csr.n_edges}): rel-L2 vs the float64 oracle = {err:.3e}")
    assert err <= 1e-5, err
