"""GPU tier: radius graphs on a periodic box (gpde_radius_csr_periodic_*, ops.radius_csr(period=...)) against the float64
minimum-image brute force of tests/helpers/periodic_oracle.py - integer work, bit-exact (every input keeps its pairs 1e-12 r^2
away from the threshold, tests/test_periodic_host.py) - the minimum-image geometry to one float32 ulp, and the property an
open graph cannot have: the operator's result does not change when every point is moved round the torus."""
import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import rel_l2
from tests.helpers import periodic_oracle as po

pytestmark = pytest.mark.gpu

D = torch.device("cuda:0")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(D)


def _build(c, **kw):
    return ops.radius_csr(_dev(c["xs"]), c["r"], pos_dst=_dev(c.get("xd")), period=c["period"], origin=c.get("origin"), **kw)


def _pair_key(src, dst, n_src):
    return dst.astype(np.int64) * n_src + src.astype(np.int64)


def _check_geom(geom, want, bound, what):
    err = np.abs(geom.astype(np.float64) - want)
    print(f"{what}: geom max |err| per column {err.max(axis=0) if len(err) else 0} (bound {bound}), "
          f"bit-equal to the rounded oracle: {np.array_equal(geom, want.astype(np.float32))}")
    assert (err <= bound).all(), (what, err.max(axis=0), bound)


@pytest.mark.parametrize("name", sorted(po.CASES))
def test_periodic_csr_is_the_csr_of_the_minimum_image_brute_force(name):
    c = po.CASES[name]()
    xs = np.asarray(c["xs"])
    n_src, dim = xs.shape
    two = "xd" in c
    n_dst = len(c["xd"]) if two else n_src
    ei, disp, norm = po.periodic_edges(xs, c["r"], c["period"], xd=c.get("xd"))
    want = np.concatenate([disp, norm[:, None]], axis=1)
    ref = ops.csr_for(_dev(ei), n_dst, n_src=n_src if two else None)
    csr, geom = _build(c, return_geometry=True)
    assert (csr.n_nodes, csr.n_src, csr.n_edges) == (n_dst, n_src, ei.shape[1])
    assert torch.equal(csr.rowptr, ref.rowptr) and torch.equal(csr.dst, ref.dst)
    assert torch.equal(csr.perm.long(), torch.arange(csr.n_edges, device=D))
    assert geom.dtype == torch.float32 and tuple(geom.shape) == (csr.n_edges, dim + 1)
    bound = po.geom_bound(c["period"], c["r"], dim)
    if name == "long_row":                           # rows of 5000 > 4096 keep cell order: each row as a set, geometry pair by pair
        assert csr.rowptr.tolist() == [0, 5000, 10000, 15000]
        got_key = _pair_key(csr.src.cpu().numpy(), csr.dst.cpu().numpy(), n_src)
        want_key = _pair_key(ei[0], ei[1], n_src)
        assert len(np.unique(got_key)) == len(got_key) and np.array_equal(np.sort(got_key), np.sort(want_key))
        _check_geom(geom.cpu().numpy()[np.argsort(got_key)], want[np.argsort(want_key)], bound, name)
    else:
        assert torch.equal(csr.src, ref.src)
        _check_geom(geom.cpu().numpy(), want[ref.perm.long().cpu().numpy()], bound, name)
    # without the geometry: the same graph (the plain fill)
    plain = _build(c)
    assert torch.equal(plain.rowptr, csr.rowptr) and torch.equal(plain.src, csr.src) and torch.equal(plain.dst, csr.dst)
    if not two:
        # a same-set graph is symmetric, and the displacement of (j -> i) is minus that of (i -> j)
        s, t = csr.src.cpu().numpy(), csr.dst.cpu().numpy()
        fwd, back = np.argsort(_pair_key(s, t, n_src)), np.argsort(_pair_key(t, s, n_src))
        assert np.array_equal(s[fwd], t[back]) and np.array_equal(t[fwd], s[back]), "edge set not symmetric"
        g = geom.cpu().numpy().astype(np.float64)
        anti = np.abs(g[fwd] * np.array([-1.0] * dim + [1.0]) - g[back])
        print(f"{name}: antisymmetry max |err| {anti.max(axis=0)}, exact: {bool((anti == 0).all())}")
        assert (anti <= bound).all(), (name, anti.max(axis=0))


def test_empty_point_sets():
    some = torch.rand(7, 2, dtype=torch.float64, device=D)
    none = torch.zeros(0, 2, dtype=torch.float64, device=D)
    csr, geom = ops.radius_csr(none, 0.1, pos_dst=some, period=1.0, return_geometry=True)          # no sources
    assert (csr.n_nodes, csr.n_src, csr.n_edges) == (7, 0, 0) and csr.rowptr.tolist() == [0] * 8 and tuple(geom.shape) == (0, 3)
    csr, geom = ops.radius_csr(some, 0.1, pos_dst=none, period=1.0, return_geometry=True)          # no destinations
    assert (csr.n_nodes, csr.n_src, csr.n_edges) == (0, 7, 0) and csr.rowptr.tolist() == [0] and tuple(geom.shape) == (0, 3)
    assert ops.radius_in_degrees(none, 0.1, pos_dst=some, period=1.0).tolist() == [0] * 7
    assert tuple(ops.radius_graph(none, 0.1, period=1.0).shape) == (2, 0)


def test_without_a_wrap_the_graph_is_the_open_builders():
    """Points in [0.25, 0.75]^2 on a box of period 4 with r = 0.2: nothing reaches the seam."""
    pos = (0.25 + 0.5 * torch.rand(2000, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(5))).to(D)
    open_ = ops.radius_csr(pos, 0.2)
    for period in (4.0, (4.0, 0.0), 0.0):                   # periodic, mixed, and every axis open through the periodic entry points
        got, geom = ops.radius_csr(pos, 0.2, period=period, return_geometry=True)
        assert torch.equal(got.rowptr, open_.rowptr) and torch.equal(got.src, open_.src) and torch.equal(got.dst, open_.dst)
        d = pos[got.src.long()] - pos[got.dst.long()]
        want = torch.cat([d, d.pow(2).sum(1, keepdim=True).sqrt()], dim=1).float()
        assert (geom - want).abs().max().item() <= float(np.spacing(np.float32(0.2)))
    got, geom = ops.radius_csr(pos, 0.2, return_geometry=True)           # return_geometry alone: the open graph with its differences
    assert torch.equal(got.src, open_.src) and torch.equal(got.rowptr, open_.rowptr) and tuple(geom.shape) == (got.n_edges, 3)


def _torus_step(conv, pos, x, a, gout):
    """Graph + geometry of `pos` on the unit torus, edge_attr = [dx, dy, |d|, a_src, a_dst] (the reference's torus attributes,
    k0 = 5), one forward and backward of `conv`."""
    csr, geom = ops.radius_csr(pos, 0.2, period=1.0, return_geometry=True)
    ea = torch.cat([geom, a[csr.src.long()][:, None], a[csr.dst.long()][:, None]], dim=1)
    xin = x.clone().requires_grad_(True)
    y = conv(xin, csr, ea)
    (gx,) = torch.autograd.grad(y, xin, gout)
    return csr, geom, y.detach(), gx


def test_translation_round_the_torus_leaves_the_operator_unchanged():
    """The 16 x 16 lattice on [0, 1)^2 moved by (5/16, 11/16) - dyadic, so every reduction, wrap and difference is exact: the same
    node ids get the same edges and bit-identical geometry, hence the same NNConv output and grad_x (<= 1e-5 relative, the
    project's bar; the summation order inside a row is unchanged, so whether they are bit-equal is printed).

    The open builder cannot do this.  The issue asked to show it by the open builder's edge COUNT changing under the shift; the
    moved lattice reduced into the box is the same point set, so the open count cannot change - what changes is which nodes
    sit at the faces.  The check with teeth: the open edge set (same node ids) differs after the move, the open in-degrees
    change, and the open graph has fewer edges than the periodic one (the seam edges are missing)."""
    from tests.test_host_logic import DenseNet
    torch.manual_seed(11)
    lat = po.lattice16()
    moved = lat + np.array([5.0 / 16.0, 11.0 / 16.0])
    pos, pos_m = _dev(lat), _dev(moved)
    n = 256
    conv = gp.NNConv_old(64, 64, DenseNet([5, 32, 64, 4096], torch.nn.ReLU), aggr="mean").to(D)
    x, a, gout = torch.randn(n, 64, device=D), torch.rand(n, device=D), torch.randn(n, 64, device=D)
    csr0, geom0, y0, gx0 = _torus_step(conv, pos, x, a, gout)
    csr1, geom1, y1, gx1 = _torus_step(conv, pos_m, x, a, gout)
    ei = po.periodic_edges(lat, 0.2, 1.0)[0]
    assert csr0.n_edges == ei.shape[1] == 256 * 37
    assert torch.equal(csr0.rowptr, csr1.rowptr) and torch.equal(csr0.src, csr1.src) and torch.equal(csr0.dst, csr1.dst)
    assert torch.equal(geom0, geom1)                                     # bit-identical
    ey, eg = rel_l2(y1, y0), rel_l2(gx1, gx0)
    print(f"translation: out rel {ey:.3e} (bit-equal {torch.equal(y0, y1)}), grad_x rel {eg:.3e} (bit-equal {torch.equal(gx0, gx1)})")
    assert ey <= 1e-5 and eg <= 1e-5, (ey, eg)
    assert float(y0.abs().max()) > 0 and float(gx0.abs().max()) > 0
    # the open builder on the same two placements (the moved one reduced into the box, as a user of an open builder would hold it)
    open0, open1 = ops.radius_csr(pos, 0.2), ops.radius_csr(_dev(np.mod(moved, 1.0)), 0.2)
    deg0, deg1 = open0.rowptr[1:] - open0.rowptr[:-1], open1.rowptr[1:] - open1.rowptr[:-1]
    print(f"open builder: {open0.n_edges} edges before, {open1.n_edges} after the move; periodic {csr0.n_edges}")
    assert not torch.equal(deg0, deg1)
    assert not (torch.equal(open0.src, open1.src) and torch.equal(open0.dst, open1.dst))
    assert open0.n_edges < csr0.n_edges and open1.n_edges < csr0.n_edges


def test_the_other_wrappers_take_a_period():
    c = po.CASES["2d_nc4"]()
    pos = _dev(c["xs"])
    csr = ops.radius_csr(pos, c["r"], period=c["period"])
    assert torch.equal(ops.radius_in_degrees(pos, c["r"], period=c["period"]), csr.rowptr[1:] - csr.rowptr[:-1])
    for name in ("2d_nc4", "two_sets", "origin", "long_row"):
        c = po.CASES[name]()
        ei = ops.radius_graph(_dev(c["xs"]), c["r"], pos_dst=_dev(c.get("xd")), period=c["period"], origin=c.get("origin"))
        assert ei.dtype == torch.int64 and np.array_equal(ei.cpu().numpy(), po.periodic_edges(c["xs"], c["r"], c["period"], xd=c.get("xd"))[0]), name


def test_multilevel_graphs_on_a_periodic_line():
    levels, radii_inner, radii_inter = po.nested_levels_1d()
    out = ops.multilevel_radius_graphs([_dev(p) for p in levels], radii_inner, radii_inter, period=1.0)
    for l, (p, r) in enumerate(zip(levels, radii_inner)):
        assert np.array_equal(out["inner"][l].cpu().numpy(), po.periodic_edges(p, r, 1.0)[0]), l
    for l, r in enumerate(radii_inter):
        want = po.periodic_edges(levels[l], r, 1.0, xd=levels[l + 1])[0]
        assert np.array_equal(out["down"][l].cpu().numpy(), want), l
        assert np.array_equal(out["up"][l].cpu().numpy(), want[::-1]), l
