"""GPU tier of the sampled graphs (graph_pde_amd.sampled_graph; the sampled arm of csrc/gpde_cellgraph.hip).

Reference: tests/helpers/gaussian_oracle.py - every ordered pair of the fixed inputs in numpy float64, by the formula of
include/gpde.h.  tests/test_gaussian_graph_host.py shows on the CPU that no fixed input has an undecided pair (|u - p| <= 4 ulp(p)),
so rowptr / src / dst are compared edge for edge, with torch.equal."""
import copy

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops, sampled_graph as sg
from tests.helpers import diag_oracle as do
from tests.helpers import gaussian_oracle as go

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD = 1e-5, 2e-5            # the bars of tests/test_gpu_diag.py


def _dev():
    return torch.device("cuda:0")


def _kw(c, d):
    kw = {k: c[k] for k in ("period", "origin", "cutoff") if k in c}
    if "xd" in c:
        kw["pos_dst"] = torch.from_numpy(np.ascontiguousarray(c["xd"])).to(d)
    return kw


def _pos(c, d):
    return torch.from_numpy(np.ascontiguousarray(c["xs"])).to(d)


def _build(c, d, **extra):
    return sg.gaussian_csr(_pos(c, d), c["sigma"], c["seed"], **_kw(c, d), **extra)


def _assert_is_the_oracles(csr, c, o):
    n_undecided = int(o["undecided"].sum())
    assert n_undecided <= go.UNDECIDED_BUDGET * o["undecided"].size and n_undecided == 0
    rowptr, src, dst = go.csr_of(o["keep"])
    assert csr.n_nodes == o["keep"].shape[0] and csr.n_edges == len(src)
    assert csr.rowptr.dtype == csr.src.dtype == csr.dst.dtype == csr.perm.dtype == torch.int32
    assert torch.equal(csr.rowptr.cpu().long(), torch.from_numpy(rowptr))
    assert torch.equal(csr.src.cpu().long(), torch.from_numpy(src))
    assert torch.equal(csr.dst.cpu().long(), torch.from_numpy(dst))
    assert torch.equal(csr.perm.cpu().long(), torch.arange(len(src)))
    assert csr.n_src_nodes == (len(c["xs"]) if "xd" in c else None)


@pytest.mark.parametrize("name", list(go.CASES))
def test_edge_for_edge_against_the_oracle(name):
    d = _dev()
    c, o = go.cached(name)
    csr = _build(c, d)
    _assert_is_the_oracles(csr, c, o)
    # the passes, the edge list and determinism on the same input
    deg = sg.gaussian_in_degrees(_pos(c, d), c["sigma"], c["seed"], **_kw(c, d))
    assert deg.dtype == torch.int32 and torch.equal(deg, csr.rowptr[1:] - csr.rowptr[:-1])
    again = _build(c, d)
    assert torch.equal(again.rowptr, csr.rowptr) and torch.equal(again.src, csr.src) and torch.equal(again.dst, csr.dst)
    ei = sg.gaussian_graph(_pos(c, d), c["sigma"], c["seed"], **_kw(c, d))
    s, t = np.nonzero(o["keep"].T)                                   # source-major, targets ascending: the order of radius_graph
    assert ei.dtype == torch.int64 and torch.equal(ei.cpu(), torch.from_numpy(np.stack([s, t]).astype(np.int64)))
    assert torch.equal(csr.edge_index, torch.stack([csr.src.long(), csr.dst.long()]))


def test_the_named_inputs_give_what_they_were_built_for():
    d = _dev()
    c, _ = go.cached("self_loops")
    csr = _build(c, d)
    n = len(c["xs"])
    assert csr.n_edges == n and torch.equal(csr.src.cpu(), torch.arange(n, dtype=torch.int32)) and torch.equal(csr.src, csr.dst)
    c, _ = go.cached("empty")
    csr, geom = _build(c, d, return_geometry=True)
    assert csr.n_edges == 0 and int(csr.rowptr.abs().max()) == 0 and csr.rowptr.numel() == 91 and tuple(geom.shape) == (0, 3)
    assert csr.n_src_nodes == 200


def test_empty_point_sets_give_an_empty_csr():
    d = _dev()
    pos, none = torch.rand(7, 2, device=d, dtype=torch.float64), torch.zeros(0, 2, device=d, dtype=torch.float64)
    for p, pd, n_dst in ((none, None, 0), (pos, none, 0), (none, pos, 7)):
        csr, geom = sg.gaussian_csr(p, 0.1, pos_dst=pd, return_geometry=True)
        assert csr.n_edges == 0 and csr.n_nodes == n_dst and csr.rowptr.numel() == n_dst + 1 and tuple(geom.shape) == (0, 3)
        assert sg.gaussian_graph(p, 0.1, pos_dst=pd).shape == (2, 0)
        assert torch.equal(sg.gaussian_in_degrees(p, 0.1, pos_dst=pd), torch.zeros(n_dst, dtype=torch.int32, device=d))


@pytest.mark.parametrize("n", go.LONG_ROWS)
def test_long_rows(n):
    """One destination and sigma = 1e9: every source is kept (the oracle agrees).  Up to 4,096 edges the row is sorted by source;
    the 4,097-edge row keeps the builder's deterministic cell order and is compared as a set."""
    d = _dev()
    c, o = go.cached(str(n))
    assert int(o["undecided"].sum()) == 0
    csr, geom = _build(c, d, return_geometry=True)
    kept = torch.from_numpy(np.nonzero(o["keep"][0])[0])
    assert csr.n_edges == len(kept) == n and csr.rowptr.tolist() == [0, n] and int(csr.dst.abs().max()) == 0
    if n <= 4096:
        assert torch.equal(csr.src.cpu().long(), kept)
    else:
        assert torch.equal(csr.src.cpu().long().sort().values, kept)
        again = _build(c, d)
        assert torch.equal(again.src, csr.src)                       # deterministic
    xs, xd = _pos(c, d), torch.from_numpy(c["xd"]).to(d)
    disp = xs[csr.src.long()] - xd[0]
    assert torch.equal(geom[:, :2], disp.float()) and torch.equal(geom[:, 2], disp.square().sum(1).sqrt().float())


def test_the_degree_hint_of_the_fill_pass_only_sizes_the_row_sort():
    """gpde_gaussian_csr_fill's max_in_degree: 0 (not known) and the true value give the same bits; a value below the true one
    leaves the rows longer than its power of two in cell order - the same edges - and every shorter row ascending."""
    import ctypes
    from graph_pde_amd import _lib
    d, lib = _dev(), _lib.lib()
    c = dict(sigma=0.12, seed=23)                                     # 2 x 2 cells: a row in cell order is not ascending
    pos = torch.from_numpy(np.random.default_rng(123).random((2000, 2))).to(d)
    ref = sg.gaussian_csr(pos, c["sigma"], c["seed"])
    n, e = ref.n_nodes, ref.n_edges
    assert ref.max_in_degree > 64 and int((ref.rowptr[1:] - ref.rowptr[:-1]).min()) < 64
    D = ctypes.c_double * 2
    lo, hi = D(*pos.min(0).values.tolist()), D(*pos.max(0).values.tolist())
    ws = torch.empty(int(lib.gpde_gaussian_csr_workspace_bytes(n, 2, c["sigma"], 0.0, lo, hi, None, None)), dtype=torch.uint8, device=d)
    deg = torch.empty(n, dtype=torch.int32, device=d)
    args = (pos.data_ptr(), n, pos.data_ptr(), n, 2, c["sigma"], 0.0, c["seed"], lo, hi, None, None)
    _lib.check(lib.gpde_gaussian_csr_count(*args, deg.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream_ptr(d)), "count")
    assert torch.equal(deg, ref.rowptr[1:] - ref.rowptr[:-1])
    out = {}
    for hint in (0, ref.max_in_degree, 4096, 1 << 40, 1):
        src, dst = torch.full((e,), -1, dtype=torch.int32, device=d), torch.full((e,), -1, dtype=torch.int32, device=d)
        _lib.check(lib.gpde_gaussian_csr_fill(*args, ref.rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(), None, e, hint, ws.data_ptr(),
                                              ws.numel(), ops._stream_ptr(d)), "fill")
        assert torch.equal(dst, ref.dst)
        out[hint] = src
    for hint in (0, ref.max_in_degree, 4096, 1 << 40):
        assert torch.equal(out[hint], ref.src), hint
    short = (deg <= 64).repeat_interleave(deg.long())                 # hint 1: rows of up to 64 edges (one wave step) are sorted
    assert torch.equal(out[1][short], ref.src[short]) and not torch.equal(out[1], ref.src)
    assert torch.equal((ref.dst.long() * n + out[1].long()).sort().values, _code(ref))


def test_seeds_and_directions_are_independent_draws():
    d = _dev()
    c, o = go.cached("rand2d")
    a = _build(c, d)
    b = sg.gaussian_csr(_pos(c, d), c["sigma"], c["seed"] + 1)
    _assert_is_the_oracles(b, c, go.outcome(c["xs"], c["sigma"], c["seed"] + 1))
    assert a.n_edges != b.n_edges or not torch.equal(a.src, b.src)
    keep = torch.zeros(len(c["xs"]), len(c["xs"]), dtype=torch.bool, device=d)
    keep[a.dst.long(), a.src.long()] = True
    assert bool(keep.diagonal().all()) and not torch.equal(keep, keep.t())
    # the extreme seeds are seeds like any other
    for seed in (-(1 << 63), (1 << 63) - 1):
        small, _ = go.cached("rand1d")
        _assert_is_the_oracles(sg.gaussian_csr(_pos(small, d), small["sigma"], seed), small, go.outcome(small["xs"], small["sigma"], seed))


def test_a_build_on_a_side_stream_is_the_default_stream_build():
    d = _dev()
    c, _ = go.cached("periodic2d")
    pos = _pos(c, d)
    ref, gref = sg.gaussian_csr(pos, c["sigma"], c["seed"], period=c["period"], return_geometry=True)
    torch.cuda.synchronize(d)
    side = torch.cuda.Stream(d)
    with torch.cuda.stream(side):
        csr, geom = sg.gaussian_csr(pos, c["sigma"], c["seed"], period=c["period"], return_geometry=True)
        deg = sg.gaussian_in_degrees(pos, c["sigma"], c["seed"], period=c["period"])
    side.synchronize()
    assert torch.equal(csr.rowptr, ref.rowptr) and torch.equal(csr.src, ref.src) and torch.equal(csr.dst, ref.dst)
    assert torch.equal(geom, gref) and torch.equal(deg, ref.rowptr[1:] - ref.rowptr[:-1])


def _code(csr):
    return csr.dst.long() * csr.n_src + csr.src.long()


@pytest.mark.parametrize("name", ["rand2d", "rand3d", "two_sets", "periodic2d", "periodic_origin", "mixed_axes", "mixed3d_two_sets"])
def test_geometry_is_the_radius_builders_rows_for_the_kept_edges(name):
    """geom of the sampled graph against radius_csr(pos, r_support, return_geometry=True): the same float32 bits on every kept
    edge, open and periodic (both builders keep rows in ascending source order, so a mask over the ball's slots aligns them)."""
    d = _dev()
    c, _ = go.cached(name)
    kw = _kw(c, d)
    csr, geom = sg.gaussian_csr(_pos(c, d), c["sigma"], c["seed"], return_geometry=True, **kw)
    ball, gball = ops.radius_csr(_pos(c, d), sg.gaussian_support_radius(c["sigma"]), return_geometry=True, **kw)
    dim = c["xs"].shape[1]
    assert geom.dtype == torch.float32 and tuple(geom.shape) == (csr.n_edges, dim + 1) and csr.n_edges > 0
    kept = torch.isin(_code(ball), _code(csr))
    assert int(kept.sum()) == csr.n_edges, "the sampled graph lies inside the radius graph of r_support"
    assert torch.equal(ball.src[kept], csr.src) and torch.equal(ball.dst[kept], csr.dst)
    assert torch.equal(gball[kept], geom)
    plain = sg.gaussian_csr(_pos(c, d), c["sigma"], c["seed"], **kw)
    assert torch.equal(plain.src, csr.src) and torch.equal(plain.rowptr, csr.rowptr)


def test_agreement_with_the_librarys_own_keys_on_the_s31_lattice():
    """The composite route where it fits: radius_csr at r_support, then edge_hash_keys / edge_sqdist_keys and torch.exp in
    float64 give the same edge set, up to pairs torch's exp leaves undecided."""
    d, s, sigma, seed = _dev(), 31, 0.1, 31
    g = torch.linspace(0.0, 1.0, s, dtype=torch.float64)
    pos = torch.stack([g.repeat(s), g.repeat_interleave(s)], dim=1).to(d)
    csr = sg.gaussian_csr(pos, sigma, seed)
    ball = ops.radius_csr(pos, sg.gaussian_support_radius(sigma))
    u = ((ops.edge_hash_keys(ball.src, ball.dst, seed) >> 10).double() + 0.5) * 2.0 ** -53
    d2 = ops.edge_sqdist_keys(ball, pos).view(torch.float64)
    p = torch.exp(-(d2 / (sigma * sigma)))
    undecided = (u - p).abs() <= go.UNDECIDED_ULPS * torch.from_numpy(np.spacing(p.cpu().numpy())).to(d)
    native = torch.isin(_code(ball), _code(csr))
    assert int(native.sum()) == csr.n_edges and csr.n_edges > 10000
    assert int(undecided.sum()) <= go.UNDECIDED_BUDGET * s ** 4
    assert torch.equal(native[~undecided], (u < p)[~undecided])


def test_nnconv_old_consumes_the_csr():
    d = _dev()
    c, _ = go.cached("rand2d")
    pos = _pos(c, d)
    csr = _build(c, d)
    torch.manual_seed(41)
    mlp = torch.nn.Sequential(torch.nn.Linear(4, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4096))
    conv = gp.NNConv_old(64, 64, mlp, aggr="mean").to(d)
    x = torch.randn(len(c["xs"]), 64, device=d)
    ei = csr.edge_index
    ea = torch.cat([pos[ei[0]], pos[ei[1]]], dim=1).float()
    with torch.no_grad():
        assert torch.equal(conv(x, csr, ea), conv(x, ei, ea))


@pytest.mark.parametrize("name", ["rand2d", "periodic2d"])
def test_nnconv_gaussian_on_the_sampled_graph_vs_float64(name):
    """The operator the graph was written for: pseudo = [|d|, a_i, a_j] with |d| = geom[:, dim]; forward and every gradient
    against the float64 composite of tests/helpers/diag_oracle.py at the bars of tests/test_gpu_diag.py."""
    d, w = _dev(), 24
    c, _ = go.cached(name)
    csr, geom = _build(c, d, return_geometry=True)
    n, dim, ei = len(c["xs"]), c["xs"].shape[1], csr.edge_index
    torch.manual_seed(42)
    a = 0.5 + torch.rand(n, device=d)
    pseudo = torch.stack([geom[:, dim], a[ei[1]], a[ei[0]]], dim=1)
    conv = gp.NNConvGaussian(w, w, torch.nn.Linear(1, w), aggr="mean").to(d)
    with torch.no_grad():
        conv.nn.weight.uniform_(0.6, 1.4).mul_(c["sigma"])           # kernel widths of the order of the graph's sigma
        conv.nn.bias.zero_()
    conv64 = copy.deepcopy(conv).double()
    x, g = torch.randn(n, w, device=d), torch.randn(n, w, device=d)
    xg = x.clone().requires_grad_(True)
    y = conv(xg, csr, pseudo)
    (y * g).sum().backward()
    x64 = x.double().requires_grad_(True)
    k64 = do.gaussian_kernel(pseudo.double(), conv64.nn(torch.ones(1, dtype=torch.float64, device=d)))
    ref = do.diag_reference(x64, x64, ei, k64, conv64.root, conv64.bias, "mean")
    (ref * g.double()).sum().backward()
    figs = {"out": _rel(y, ref), "out_row": do.worst_row(y, ref), "dx": _rel(xg.grad, x64.grad), "dx_row": do.worst_row(xg.grad, x64.grad)}
    for (nm, p), (_, p64) in zip(conv.named_parameters(), conv64.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), nm
        figs["d" + nm] = _rel(p.grad, p64.grad)
    print(f"[sampled] NNConvGaussian on {name}: E={csr.n_edges} " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    bad = {k: v for k, v in figs.items() if not v <= (TOL_FWD if k.startswith("out") else TOL_BWD)}
    assert not bad, bad
    with torch.no_grad():
        assert torch.equal(conv(x, csr, pseudo), conv(x, ei, pseudo))


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
