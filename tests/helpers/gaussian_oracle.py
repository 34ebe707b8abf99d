"""The independent checker of the sampled graphs (graph_pde_amd.sampled_graph, gpde_gaussian_csr_*) and the fixed inputs of
tests/test_gaussian_graph_host.py and tests/test_gpu_gaussian_graph.py.  numpy float64 only; it never calls the code under test.

    u        ((key >> 10) + 0.5) * 2^-53, key = the header's hash of (seed, dst = i, src = j) (neighbor_cap.hash_keys restates
             it from the constants of include/gpde.h); the sum is an ordinary float64 sum (numpy rounds it as the device does);
    d2       open axes d = xd[i] - xs[j], periodic axes d = xs[j] - xd[i], d -= L round(d / L) on the raw coordinates; squares
             summed in axis order, unfused - the arithmetic the header states for gpde_edge_keys_sqdist, so the bits agree;
    p        exp(-(d2 / (sigma * sigma)));
    outcome  kept (u < p), dropped, or UNDECIDED when |u - p| <= 4 ulp(p): the device's exp and numpy's may differ in the last
             place.  A pair past the cutoff (d2 > cutoff^2) is dropped whatever u is.

Every ordered pair is evaluated: dense [n_dst, n_src] arrays, so the inputs stay at a few thousand points."""
import math

import numpy as np

from tests.helpers import neighbor_cap as nc
from tests.helpers import periodic_oracle as po

SUPPORT = math.sqrt(54.0 * math.log(2.0))         # r_support / sigma
UNDECIDED_ULPS = 4.0
UNDECIDED_BUDGET = 1e-6                           # of the candidate (ordered) pairs


def pair_u(n_src, n_dst, seed):
    """u [n_dst, n_src] of every ordered pair (row = destination i, column = source j)."""
    i, j = np.meshgrid(np.arange(n_dst, dtype=np.int64), np.arange(n_src, dtype=np.int64), indexing="ij")
    key = nc.hash_keys(j.ravel(), i.ravel(), seed).reshape(n_dst, n_src)
    return ((key >> 10).astype(np.float64) + 0.5) * 2.0 ** -53


def pair_d2(xs, xd=None, period=None):
    """d2 [n_dst, n_src], operation by operation as the header states."""
    xs = np.asarray(xs, dtype=np.float64).reshape(len(xs), -1)
    xd = xs if xd is None else np.asarray(xd, dtype=np.float64).reshape(len(xd), -1)
    L = po.per_axis(period, xs.shape[1])
    d2 = np.zeros((len(xd), len(xs)), dtype=np.float64)
    for a in range(xs.shape[1]):
        if L[a] > 0.0:
            d = xs[None, :, a] - xd[:, None, a]
            d = d - L[a] * np.round(d / L[a])
        else:
            d = xd[:, None, a] - xs[None, :, a]
        d2 = d2 + d * d
    return d2


def outcome(xs, sigma, seed, xd=None, period=None, cutoff=None):
    """dict(keep, undecided bool [n_dst, n_src]; p, u, d2 float64 [n_dst, n_src]) of every ordered pair."""
    xs = np.asarray(xs, dtype=np.float64).reshape(len(xs), -1)
    n_dst = len(xs) if xd is None else len(xd)
    d2 = pair_d2(xs, xd, period)
    u = pair_u(len(xs), n_dst, seed)
    s2 = np.float64(sigma) * np.float64(sigma)
    with np.errstate(under="ignore"):
        p = np.exp(-(d2 / s2))
    inside = np.ones_like(d2, dtype=bool) if cutoff is None else d2 <= np.float64(cutoff) * np.float64(cutoff)
    undecided = inside & (np.abs(u - p) <= UNDECIDED_ULPS * np.spacing(p))
    return dict(keep=inside & (u < p), undecided=undecided, p=np.where(inside, p, 0.0), u=u, d2=d2)


def csr_of(keep):
    """(rowptr int64 [n_dst + 1], src int64 [E], dst int64 [E]): rows by destination, ascending source inside a row."""
    dst, src = np.nonzero(keep)                    # row-major: destination-major, sources ascending
    rowptr = np.zeros(keep.shape[0] + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=rowptr[1:])
    return rowptr, src.astype(np.int64), dst.astype(np.int64)


def grid_cells(x, r):
    """The open builder's cell of every point for radius r (gpde_cellgraph.hip make_grid: cell edge 1.0001 r from the lower
    corner of the bounding box), as one tuple per point - to count the members of a cell."""
    x = np.asarray(x, dtype=np.float64)
    inv = 1.0 / (r * 1.0001)
    return [tuple(c) for c in np.floor((x - x.min(axis=0)) * inv).astype(np.int64)]


# ---- fixed inputs -----------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


CELL_SIGMA = 0.04
CELL_MEMBERS = {(1, 1): 63, (3, 1): 64, (1, 3): 65, (3, 3): 1}


def _cells():
    """Cells of the builder's grid holding exactly 1, 63, 64 and 65 sources (one wave step is 64 candidates): clusters inside the
    cells (1, 1), (3, 1), (1, 3), (3, 3) of the 5 x 5 grid that the corner points (0, 0) and (1, 1) pin down."""
    g = _rng(104)
    cs = CELL_SIGMA * SUPPORT * 1.0001
    pts = [np.array([[0.0, 0.0], [1.0, 1.0]])]
    for (cx, cy), m in CELL_MEMBERS.items():
        pts.append((np.array([cx, cy]) + 0.5 + 0.8 * (g.random((m, 2)) - 0.5)) * cs)
    x = np.concatenate(pts)
    return dict(xs=x[g.permutation(len(x))], sigma=CELL_SIGMA, seed=5)


def _periodic2d():
    g = _rng(106)
    x = g.random((600, 2))
    x[:40] += g.integers(-2, 3, size=(40, 2)).astype(np.float64)         # points outside the box are legal
    return dict(xs=x, sigma=0.06, seed=7, period=1.0)


def _empty():
    """Two node sets without a coincident point and a tiny sigma: no edge at all, every row empty."""
    return dict(xs=_rng(111).random((200, 2)), xd=_rng(112).random((90, 2)), sigma=1e-7, seed=12)


CASES = {
    "rand1d": lambda: dict(xs=_rng(101).random((400, 1)), sigma=0.02, seed=1),
    "rand2d": lambda: dict(xs=_rng(102).random((1500, 2)), sigma=0.05, seed=2),
    "rand3d": lambda: dict(xs=_rng(103).random((800, 3)), sigma=0.1, seed=-3),
    "lattice16": lambda: dict(xs=po.lattice16(), sigma=0.15, seed=4),
    "cells_1_63_64_65": _cells,
    "two_sets": lambda: dict(xs=_rng(105).random((300, 2)), xd=_rng(115).random((120, 2)), sigma=0.08, seed=6),
    "periodic2d": _periodic2d,
    "periodic_origin": lambda: dict(xs=_rng(116).random((300, 2)) * np.array([1.0, 1.5]) + np.array([-0.3, 0.7]), sigma=0.07, seed=17,
                                    period=(1.0, 1.5), origin=(-0.3, 0.7)),
    "mixed_axes": lambda: dict(xs=_rng(107).random((500, 2)), sigma=0.05, seed=8, period=(1.0, 0.0)),
    "mixed3d_two_sets": lambda: dict(xs=_rng(117).random((300, 3)), xd=_rng(118).random((100, 3)), sigma=0.07, seed=18,
                                     period=(0.0, 1.0, 1.0)),
    "cutoff": lambda: dict(xs=_rng(108).random((1000, 2)), sigma=0.08, seed=9, cutoff=0.15),
    "periodic_cutoff": lambda: dict(xs=_rng(119).random((400, 2)), sigma=0.2, seed=19, period=1.0, cutoff=0.3),
    "one_cell": lambda: dict(xs=_rng(109).random((300, 2)), sigma=0.5, seed=10),
    "self_loops": lambda: dict(xs=_rng(110).random((500, 2)), sigma=1e-7, seed=11),
    "empty": _empty,
}

LONG_ROWS = (4095, 4096, 4097)       # one destination; the builder sorts rows of up to 4096 edges
LONG_SIGMA = 1e9


def long_row_case(n):
    g = _rng(200 + n % 7)
    return dict(xs=g.random((n, 2)), xd=np.array([[0.5, 0.5]]), sigma=LONG_SIGMA, seed=21)


def case_outcome(c):
    return outcome(c["xs"], c["sigma"], c["seed"], xd=c.get("xd"), period=c.get("period"), cutoff=c.get("cutoff"))


_memo = {}


def cached(name):
    """(case dict, outcome) of a fixed input, computed once per process and shared - treat both as read-only."""
    if name not in _memo:
        c = CASES[name]() if name in CASES else long_row_case(int(name))
        _memo[name] = (c, case_outcome(c))
    return _memo[name]
