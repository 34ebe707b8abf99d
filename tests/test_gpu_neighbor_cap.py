"""GPU tier of the capped in-degree: gpde_csr_select_k alone on synthetic rows, the two key kernels against the host
arithmetic, radius_csr / radius_csr_batched with max_num_neighbors end to end, and the operator on a capped graph.  The checker
is tests/helpers/neighbor_cap.py (numpy; it never calls the code under test); the fairness of every periodic "nearest" input
is asserted on the CPU by tests/test_neighbor_cap_host.py, so no case is left out here."""
import functools

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, rel_l2
from tests.helpers import neighbor_cap as nc
from tests.helpers import periodic_oracle as po

pytestmark = pytest.mark.gpu

D = torch.device("cuda:0")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _np(t):
    return t.detach().cpu().numpy()


def _same_graph(a, b):
    return (a.n_nodes, a.n_edges, a.n_src) == (b.n_nodes, b.n_edges, b.n_src) and torch.equal(a.rowptr, b.rowptr) and \
        torch.equal(a.src, b.src) and torch.equal(a.dst, b.dst)


def _check_against_helper(got, full, key_np, k, what):
    """`got` (a capped Csr) is the helper's selection of `full` (the uncapped Csr of the device) under key_np."""
    ptr, kept = nc.select(_np(full.rowptr), key_np, k)
    assert got.n_edges == len(kept) and got.n_nodes == full.n_nodes and got.n_src == full.n_src, what
    assert np.array_equal(_np(got.rowptr), ptr), what
    assert np.array_equal(_np(got.src), _np(full.src)[kept]) and np.array_equal(_np(got.dst), _np(full.dst)[kept]), what
    assert torch.equal(got.perm.long(), torch.arange(got.n_edges, device=D)), what
    return kept


# ---- 1. select_in_edges alone ------------------------------------------------------------------------------------------------------
def _synthetic_csr(k, rect=None):
    rowptr = nc.synthetic_rows(k)
    n, e = len(rowptr) - 1, int(rowptr[-1])
    g = torch.Generator().manual_seed(100 + k)
    src = torch.randint(0, rect or n, (e,), generator=g, dtype=torch.int32)
    dst = torch.repeat_interleave(torch.arange(n, dtype=torch.int32), torch.from_numpy(np.diff(rowptr)))
    perm = torch.randperm(e, generator=g).to(torch.int32)
    return ops.Csr(n, e, _dev(rowptr.astype(np.int32)), src.to(D), dst.to(D), perm.to(D), n_src_nodes=rect)


@pytest.mark.parametrize("k", nc.SELECT_KS)
def test_select_on_synthetic_rows(k):
    """Row lengths 0, 1, k - 1, k, k + 1, 63 .. 129, around the LDS staging limit (2048 keys) and 10,000; four kinds of keys."""
    csr = _synthetic_csr(k, rect=77 if k == 33 else None)
    old_max = 10000
    for kind in nc.KEY_KINDS:
        key = nc.synthetic_keys(kind, csr.n_edges, seed=k)
        got, ids = ops.select_in_edges(csr, k, _dev(key))
        kept = _check_against_helper(got, csr, key, k, (k, kind))
        assert ids.dtype == torch.int64 and np.array_equal(_np(ids), _np(csr.perm)[kept]), (k, kind)
        assert got.max_in_degree == min(old_max, k) == int(np.diff(_np(got.rowptr)).max())
        assert got.n_src_nodes == csr.n_src_nodes and got._flow_flipped == csr._flow_flipped
        again, ids2 = ops.select_in_edges(csr, k, _dev(key))                  # two calls: identical
        assert _same_graph(got, again) and torch.equal(ids, ids2)


@pytest.mark.parametrize("kind", ["int64", "three_values", "float"])
def test_selections_are_nested(kind):
    csr = _synthetic_csr(16)
    key = _dev(nc.synthetic_keys(kind, csr.n_edges, seed=9))
    ids = {k: _np(ops.select_in_edges(csr, k, key)[1]) for k in (8, 16, 64)}
    assert len(ids[8]) < len(ids[16]) < len(ids[64])
    assert np.isin(ids[8], ids[16]).all() and np.isin(ids[16], ids[64]).all()


def test_select_keeps_everything_when_no_row_is_longer_and_refuses_nan():
    csr = _synthetic_csr(2)
    key = _dev(nc.synthetic_keys("float", csr.n_edges, seed=4))
    for k in (10000, 10001, 1 << 40):
        got, ids = ops.select_in_edges(csr, k, key)
        assert _same_graph(got, csr) and torch.equal(ids, csr.perm.long())
        assert torch.equal(got.perm.long(), torch.arange(csr.n_edges, device=D)) and got.max_in_degree == 10000
    bad = key.clone()
    bad[12345] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ops.select_in_edges(csr, 3, bad)
    empty = ops.Csr(3, 0, torch.zeros(4, dtype=torch.int32, device=D), *(torch.zeros(0, dtype=torch.int32, device=D) for _ in range(3)))
    got, ids = ops.select_in_edges(empty, 5, torch.zeros(0, dtype=torch.int64, device=D))
    assert got.n_edges == 0 and got.rowptr.tolist() == [0] * 4 and ids.numel() == 0


# ---- 2. the key kernels ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _open(name):
    """(case, pos, pos_dst | None, the device's uncapped Csr) of an open-box input - built once, shared by the tests."""
    c = nc.OPEN_CASES[name]()
    pos, pd = _dev(c["xs"]), _dev(c.get("xd"))
    return c, pos, pd, ops.radius_csr(pos, c["r"], pos_dst=pd)


@functools.lru_cache(maxsize=None)
def _periodic(name):
    c = po.CASES[name]()
    pos, pd = _dev(c["xs"]), _dev(c.get("xd"))
    csr, geom = ops.radius_csr(pos, c["r"], pos_dst=pd, period=c["period"], origin=c.get("origin"), return_geometry=True)
    return c, pos, pd, csr, geom


@pytest.mark.parametrize("name", sorted(nc.OPEN_CASES))
def test_sqdist_keys_on_open_boxes_are_the_host_bits(name):
    c, pos, pd, full = _open(name)
    want = nc.d2_bits(nc.d2_open(c["xs"], c.get("xd"), _np(full.src), _np(full.dst)))
    got = ops.edge_sqdist_keys(full, pos, pd)
    assert got.dtype == torch.int64 and torch.equal(got, _dev(want))
    if name in ("lattice16", "1d_300"):                       # the periodic entry form with every axis open is the same arithmetic
        assert torch.equal(ops.edge_sqdist_keys(full, pos, pd, period=0.0, origin=0.3), got)


def _periodic_keys(name):
    c, pos, pd, full, _ = _periodic(name)
    got = _np(ops.edge_sqdist_keys(full, pos, pd, period=c["period"], origin=c.get("origin")))
    want = nc.d2_periodic(c["xs"], c.get("xd"), _np(full.src), _np(full.dst), c["period"])
    return c, got, want


@pytest.mark.parametrize("name", sorted(nc.PERIODIC_NEAREST))
def test_sqdist_keys_on_periodic_boxes_are_within_4_ulp(name):
    """Kernel and checker both take d = x_s - x_d on the raw coordinates and d -= L round(d / L) (half to even), unfused: the
    same operations, so the expected difference is 0 ulp; the bound is the issue's 4.  (A first version of the kernel reduced
    both points into the box and subtracted an image x_d +- L, as the periodic builder does: x_d +- L is rounded at the magnitude
    of L, and it measured up to 53 / 41 / 37 / 149 / 22 / 68 / 26 / 43 ulp on 2d_nc2 / 2d_nc3 / 2d_nc4 / 2d_nc7 / 3d_open_y /
    origin / two_sets / long_row and 1416 ulp on outside_box, whose raw coordinates reach +-4.)"""
    c, got, want = _periodic_keys(name)
    ulp = np.abs(got - nc.d2_bits(want))
    print(f"{name}: {len(ulp)} edges, max {int(ulp.max())} ulp, {float((ulp == 0).mean()):.4f} bit-equal")
    assert (got >= 0).all() and int(ulp.max()) <= 4, (name, int(ulp.max()))


@pytest.mark.parametrize("seed", [0, 1, -1, (1 << 62) + 3])
def test_hash_keys_are_the_helper_bits(seed):
    g = np.random.default_rng(7)
    top = (1 << 31) - 1
    src = np.concatenate([[0, 0, top, top, 1, 2], g.integers(0, 1 << 31, size=3000)]).astype(np.int32)
    dst = np.concatenate([[0, top, 0, top, 2, 1], g.integers(0, 1 << 31, size=3000)]).astype(np.int32)
    got = ops.edge_hash_keys(_dev(src), _dev(dst), seed)
    assert got.dtype == torch.int64 and torch.equal(got, _dev(nc.hash_keys(src, dst, seed)))
    assert int(got.min()) >= 0
    assert ops.edge_hash_keys(_dev(src[:0]), _dev(dst[:0]), seed).numel() == 0


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------
SEED = 12345


@pytest.mark.parametrize("mode", ["nearest", "random"])
@pytest.mark.parametrize("name", sorted(nc.OPEN_CASES))
def test_capped_radius_csr_is_the_helper_selection_of_the_uncapped_graph(name, mode):
    c, pos, pd, full = _open(name)
    src, dst = _np(full.src), _np(full.dst)
    deg = np.diff(_np(full.rowptr))
    if name == "hub_5000":
        assert deg[0] >= 5000 and (np.diff(src[:deg[0]]) < 0).any(), "the hub row must be past the row sort: slots in cell order"
    key = nc.d2_bits(nc.d2_open(c["xs"], c.get("xd"), src, dst)) if mode == "nearest" else nc.hash_keys(src, dst, SEED)
    for k in c["ks"]:
        assert (deg > k).any()
        got = ops.radius_csr(pos, c["r"], pos_dst=pd, max_num_neighbors=k, select=mode, seed=SEED)
        _check_against_helper(got, full, key, k, (name, mode, k))
        assert got.max_in_degree == k
        assert (got.n_src_nodes is None) == (pd is None)
    if mode == "random":                                       # the seed matters, and is all that matters
        k = c["ks"][0]
        a = ops.radius_csr(pos, c["r"], pos_dst=pd, max_num_neighbors=k, select="random", seed=SEED + 1)
        b = ops.radius_csr(pos, c["r"], pos_dst=pd, max_num_neighbors=k, select="random", seed=SEED + 1)
        assert _same_graph(a, b)
        assert not torch.equal(a.src, ops.radius_csr(pos, c["r"], pos_dst=pd, max_num_neighbors=k, select="random", seed=SEED).src)


def test_capped_graph_against_brute_force_from_the_positions():
    """No device graph on the checker's side: positions -> float64 brute force -> CSR -> the k nearest, all in numpy."""
    c = nc.OPEN_CASES["two_sets"]()
    ei = nc.brute_open_edges(c["xs"], c["r"], c["xd"])
    rowptr, src, dst = nc.csr_of_edges(ei, len(c["xd"]))
    for k in c["ks"]:
        ptr, kept = nc.select(rowptr, nc.d2_bits(nc.d2_open(c["xs"], c["xd"], src, dst)), k)
        got = ops.radius_csr(_dev(c["xs"]), c["r"], pos_dst=_dev(c["xd"]), max_num_neighbors=k)
        assert np.array_equal(_np(got.rowptr), ptr) and np.array_equal(_np(got.src), src[kept]) and np.array_equal(_np(got.dst), dst[kept])
        rnd = ops.radius_csr(_dev(c["xs"]), c["r"], pos_dst=_dev(c["xd"]), max_num_neighbors=k, select="random", seed=-2)
        ptr, kept = nc.select(rowptr, nc.hash_keys(src, dst, -2), k)
        assert np.array_equal(_np(rnd.rowptr), ptr) and np.array_equal(_np(rnd.src), src[kept]) and np.array_equal(_np(rnd.dst), dst[kept])


@pytest.mark.parametrize("name", sorted(nc.PERIODIC_NEAREST))
def test_capped_periodic_graphs_and_their_geometry(name):
    c, pos, pd, full, geom = _periodic(name)
    src, dst = _np(full.src), _np(full.dst)
    d2 = nc.d2_periodic(c["xs"], c.get("xd"), src, dst, c["period"])
    for k in nc.PERIODIC_NEAREST[name]:
        got, g = ops.radius_csr(pos, c["r"], pos_dst=pd, period=c["period"], origin=c.get("origin"), return_geometry=True,
                                max_num_neighbors=k)
        kept = _check_against_helper(got, full, d2, k, (name, k))
        assert g.dtype == torch.float32 and torch.equal(g, geom[_dev(kept)])
        plain = ops.radius_csr(pos, c["r"], pos_dst=pd, period=c["period"], origin=c.get("origin"), max_num_neighbors=k)
        assert _same_graph(plain, got)
    k = nc.PERIODIC_NEAREST[name][0]
    got, g = ops.radius_csr(pos, c["r"], pos_dst=pd, period=c["period"], origin=c.get("origin"), return_geometry=True,
                            max_num_neighbors=k, select="random", seed=3)
    kept = _check_against_helper(got, full, nc.hash_keys(src, dst, 3), k, (name, "random"))
    assert torch.equal(g, geom[_dev(kept)])


@pytest.mark.parametrize("two_sets", [False, True])
@pytest.mark.parametrize("mode", ["nearest", "random"])
def test_capped_batch_is_the_capped_graphs_concatenated(mode, two_sets):
    xs, ptr, radii = nc.batch_case()
    k = 6
    pos = _dev(xs)
    if two_sets:                                             # destinations: every third point of each graph
        pick = np.concatenate([np.arange(ptr[b], ptr[b + 1])[::3] for b in range(5)])
        ptr_d = np.concatenate([[0], np.cumsum([len(np.arange(ptr[b], ptr[b + 1])[::3]) for b in range(5)])]).astype(np.int64)
        pd = _dev(xs[pick])
        kw = dict(pos_dst=pd, ptr_dst=torch.from_numpy(ptr_d))
    else:
        ptr_d, pd, kw = ptr, None, {}
    got, edge_ptr = ops.radius_csr_batched(pos, torch.from_numpy(ptr), radii, max_num_neighbors=k, select=mode, seed=SEED, **kw)
    full, full_ptr = ops.radius_csr_batched(pos, torch.from_numpy(ptr), radii, **kw)
    assert got.n_edges < full.n_edges and got.max_in_degree == k
    rowptr, src, dst, eptr = [np.zeros(1, dtype=np.int64)], [], [], [0]
    for b in range(5):
        p = pos[ptr[b]:ptr[b + 1]]
        q = None if pd is None else pd[ptr_d[b]:ptr_d[b + 1]]
        one = ops.radius_csr(p, radii[b], pos_dst=q, max_num_neighbors=k, select=mode, seed=SEED)
        rowptr.append(_np(one.rowptr).astype(np.int64)[1:] + eptr[-1])
        src.append(_np(one.src).astype(np.int64) + ptr[b])
        dst.append(_np(one.dst).astype(np.int64) + ptr_d[b])
        eptr.append(eptr[-1] + one.n_edges)
    assert np.array_equal(_np(got.rowptr), np.concatenate(rowptr))
    assert np.array_equal(_np(got.src), np.concatenate(src)) and np.array_equal(_np(got.dst), np.concatenate(dst))
    assert edge_ptr.dtype == torch.int64 and edge_ptr.tolist() == eptr
    assert torch.equal(got.perm.long(), torch.arange(got.n_edges, device=D))
    # and the helper's selection of the uncapped batch (graph-local ids in the hash)
    fs, fd = _np(full.src).astype(np.int64), _np(full.dst).astype(np.int64)
    gid = np.searchsorted(ptr_d[1:], fd, side="right")
    key = nc.d2_bits(nc.d2_open(xs, None if pd is None else _np(pd), fs, fd)) if mode == "nearest" else \
        nc.hash_keys(fs - ptr[gid], fd - ptr_d[gid], SEED)
    _check_against_helper(got, full, key, k, ("batch", mode))


def test_a_cap_above_every_degree_is_the_uncapped_graph():
    c, pos, pd, full = _open("2d_2000")
    big = int(np.diff(_np(full.rowptr)).max())
    for k, mode in ((big, "nearest"), (big + 1, "random"), (1 << 40, "nearest")):
        assert _same_graph(ops.radius_csr(pos, c["r"], max_num_neighbors=k, select=mode), full)
    c, pos, pd, full, geom = _periodic("2d_nc7")
    got, g = ops.radius_csr(pos, c["r"], period=c["period"], return_geometry=True, max_num_neighbors=1000)
    assert _same_graph(got, full) and torch.equal(g, geom)
    xs, ptr, radii = nc.batch_case()
    a, pa = ops.radius_csr_batched(_dev(xs), torch.from_numpy(ptr), radii, max_num_neighbors=100000)
    b, pb = ops.radius_csr_batched(_dev(xs), torch.from_numpy(ptr), radii)
    assert _same_graph(a, b) and torch.equal(pa, pb)


# ---- 4. the operator on a capped graph ---------------------------------------------------------------------------------------------
def test_the_operator_on_a_capped_graph():
    from tests.test_host_logic import DenseNet
    torch.manual_seed(21)
    n, k = 256, 8
    g = np.random.default_rng(22)
    pos = _dev(g.random((n, 2)))
    a = torch.rand(n, device=D)
    full = ops.radius_csr(pos, 0.2)
    s, t = full.src.long(), full.dst.long()
    edge_attr = torch.cat([pos[s], pos[t], a[s][:, None], a[t][:, None]], dim=1).float()       # by slot of the UNCAPPED graph
    csr_k, edge_ids = ops.select_in_edges(full, k, ops.edge_sqdist_keys(full, pos))
    ea = edge_attr[edge_ids].contiguous()
    assert csr_k.n_edges < full.n_edges and csr_k.n_edges == int(edge_ids.numel())
    assert csr_k._max_in_degree == k == csr_k.max_in_degree == int((csr_k.rowptr[1:] - csr_k.rowptr[:-1]).max())
    want_attr = torch.cat([pos[csr_k.src.long()], pos[csr_k.dst.long()], a[csr_k.src.long()][:, None], a[csr_k.dst.long()][:, None]], dim=1).float()
    assert torch.equal(ea, want_attr)                      # edge_ids address the input graph's per-edge rows
    conv = gp.NNConv_old(64, 64, DenseNet([6, 32, 32, 4096], torch.nn.ReLU), aggr="mean").to(D)
    x = torch.randn(n, 64, device=D)
    gout = torch.randn(n, 64, device=D)

    def step(graph):
        xin = x.clone().requires_grad_(True)
        y = conv(xin, graph, ea)
        grads = torch.autograd.grad(y, [xin] + list(conv.parameters()), gout)
        return y.detach(), grads
    y_csr, g_csr = step(csr_k)
    y_ei, g_ei = step(csr_k.edge_index)
    assert torch.equal(y_csr, y_ei)
    for (pname, _), u, v in zip([("x", None)] + list(conv.named_parameters()), g_csr, g_ei):
        assert torch.equal(u, v), pname
    lin = ops.mlp_linears(conv.nn)
    ref = nnconv_forward(x.cpu(), csr_k.edge_index.cpu(), ea.cpu(), [l.weight.detach().cpu() for l in lin],
                         [l.bias.detach().cpu() for l in lin], conv.root.detach().cpu(), conv.bias.detach().cpu(), aggr="mean",
                         dtype=torch.float64)
    err = rel_l2(y_csr, ref)
    print(f"capped operator: N = {n}, E = {full.n_edges} -> {csr_k.n_edges}, rel-L2 vs the float64 oracle {err:.3e}")
    assert err <= 1e-5, err
