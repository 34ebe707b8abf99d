"""The independent checker of the k-nearest-neighbour graphs (graph_pde_amd.neighbor_graph, gpde_knn_csr) and the fixed inputs of
tests/test_knn_host.py / tests/test_gpu_knn.py.  numpy only; it never calls the code under test.

    oracle    the complete bipartite edge list (self pairs dropped for loop=False on one point set), keys =
              neighbor_cap.d2_bits(neighbor_cap.d2_open(...)), rows cut by neighbor_cap.select: per row the k_eff smallest
              (key, source), returned in ascending source order.  Before `select` sorts, a row's pairs beyond its k_eff-th smallest
              d2 are dropped - none of them can be among the k_eff smallest (key, source), every tie at that d2 stays - so that
              the 10,000-point inputs sort 10^5 pairs instead of 10^8.  Rows are processed in chunks.
"""
import numpy as np

from tests.helpers import neighbor_cap as nc


def as2d(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(len(x), -1)


def k_eff(k, n_src, one_set, loop):
    return max(0, min(int(k), int(n_src) - (1 if one_set and not loop else 0)))


def oracle(xs, k, xd=None, loop=False, chunk=1000):
    """(rowptr int64 [n_dst + 1], src int64 [E], dst int64 [E]) of the kNN graph, E = n_dst * k_eff."""
    xs = as2d(xs)
    one = xd is None
    xd2 = xs if one else as2d(xd)
    ns, nd = len(xs), len(xd2)
    ke = k_eff(k, ns, one, loop)
    rowptr = np.arange(nd + 1, dtype=np.int64) * ke
    dst = np.repeat(np.arange(nd, dtype=np.int64), ke)
    if ke == 0 or nd == 0:
        return rowptr, np.zeros(0, dtype=np.int64), dst
    out = []
    for r0 in range(0, nd, chunk):
        rows = np.arange(r0, min(r0 + chunk, nd), dtype=np.int64)
        keep = np.ones((len(rows), ns), dtype=bool)
        if one and not loop:
            keep[rows - r0, rows] = False
        if ke < ns:                                             # the cut: the same arithmetic, [rows, n_src] at once
            m = np.zeros((len(rows), ns))
            for a in range(xs.shape[1]):
                t = xd2[rows, None, a] - xs[None, :, a]
                m = m + t * t
            m[~keep] = np.inf
            kth = np.partition(m, ke - 1, axis=1)[:, ke - 1]
            keep &= m <= kth[:, None]
        d, s = np.nonzero(keep)                                 # row-major: ascending source inside a row
        d = d + r0
        rp = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(np.bincount(d - r0, minlength=len(rows)), out=rp[1:])
        new, kept = nc.select(rp, nc.d2_bits(nc.d2_open(xs, None if one else xd2, s, d)), ke)
        assert np.array_equal(np.diff(new), np.full(len(rows), ke))
        out.append(s[kept])
    return rowptr, np.concatenate(out), dst


def geometry(xs, xd, src, dst):
    """float32 [E, dim + 1]: pos[src] - pos_dst[dst] per axis and its norm, float64 rounded once."""
    xs = as2d(xs)
    xd = xs if xd is None else as2d(xd)
    d = xs[src] - xd[dst]
    d2 = np.zeros(len(src))
    for a in range(xs.shape[1]):
        d2 = d2 + d[:, a] * d[:, a]
    return np.concatenate([d, np.sqrt(d2)[:, None]], axis=1).astype(np.float32)


def _rng(seed):
    return np.random.default_rng(seed)


def lattice9(shift=(0.0, 0.0)):
    """The 9 x 9 lattice of coordinates i / 8 (exact binary fractions: points ON the faces of power-of-two grids) + shift."""
    g = np.arange(9, dtype=np.float64) / 8.0
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2) + np.asarray(shift, dtype=np.float64)


def _duplicates():
    g = _rng(51)
    return np.concatenate([np.repeat(g.random((1, 2)), 16, axis=0), g.random((20, 2))])[g.permutation(36)]


def _clustered(n_in=250, n_out=50, seed=52):
    g = _rng(seed)
    return np.concatenate([0.37 + 1e-3 * g.random((n_in, 2)), g.random((n_out, 2))])[g.permutation(n_in + n_out)]


def _line2d():
    return np.stack([_rng(53).random(200), np.full(200, 0.5)], axis=1)


def _two_sets_far():
    xd = _rng(56).random((40, 2))
    xd[5:15] = xd[5:15] * 3.0 + 40.0             # ten destinations far outside the sources' box
    return xd


LATTICE_KS = (1, 4, 5, 8, 9, 12, 80, 81, 100)

# name -> xs, optional xd, ks, loops, `spacing` (the typical point spacing), optional `lattice` (its exact spacing), optional
# `bounds` (a caller-given box)
CASES = {
    "lattice9": lambda: dict(xs=lattice9(), ks=LATTICE_KS, loops=(False, True), spacing=0.125, lattice=0.125),
    "lattice9_shifted": lambda: dict(xs=lattice9((0.1, 0.3)), ks=LATTICE_KS, loops=(False, True), spacing=0.125, lattice=0.125),
    "duplicates": lambda: dict(xs=_duplicates(), ks=(3, 15, 16, 17), loops=(False,), spacing=0.15),
    "clustered": lambda: dict(xs=_clustered(), ks=(1, 16, 64, 256), loops=(False,), spacing=0.05),
    "line_in_2d": lambda: dict(xs=_line2d(), ks=(7,), loops=(False,), spacing=0.005),
    "1d_200": lambda: dict(xs=_rng(54).random((200, 1)), ks=(7,), loops=(False,), spacing=0.005),
    "3d_200": lambda: dict(xs=_rng(55).random((200, 3)), ks=(7,), loops=(False,), spacing=0.17),
    "two_sets": lambda: dict(xs=_rng(57).random((150, 2)), xd=_rng(56).random((40, 2)), ks=(1, 9, 150, 200), loops=(False,), spacing=0.08),
    "two_sets_far": lambda: dict(xs=_rng(57).random((150, 2)), xd=_two_sets_far(), ks=(1, 9, 150, 200), loops=(False,), spacing=0.08),
    # the box [0, 2/3] x [0, 1] cuts off a third of the sources and a third of the destinations
    "two_sets_bounds": lambda: dict(xs=_rng(57).random((150, 2)), xd=_rng(56).random((40, 2)), ks=(1, 9, 150, 200), loops=(False,),
                                    spacing=0.08, bounds=((0.0, 0.0), (2.0 / 3.0, 1.0))),
    "n1": lambda: dict(xs=_rng(58).random((1, 2)), ks=(1, 3), loops=(False, True), spacing=1.0),
    "n2": lambda: dict(xs=_rng(59).random((2, 2)), ks=(2, 5), loops=(False, True), spacing=1.0),
    "n5": lambda: dict(xs=_rng(60).random((5, 3)), ks=(5, 9), loops=(False, True), spacing=0.5),
}

LARGE = {
    "2d_10000": lambda: dict(xs=_rng(61).random((10000, 2)), ks=(16,), loops=(False,), spacing=0.01),
    "3d_10000": lambda: dict(xs=_rng(62).random((10000, 3)), ks=(32,), loops=(False,), spacing=0.046),
}


def cell_sizes(c):
    """The cell edges every case runs under: automatic, the lattice spacing where there is one, a third of the typical
    spacing, and the whole box as one cell."""
    pts = as2d(c["xs"]) if "xd" not in c else np.concatenate([as2d(c["xs"]), as2d(c["xd"])])
    ext = float((pts.max(axis=0) - pts.min(axis=0)).max()) if len(pts) else 0.0
    sizes = [None]
    if "lattice" in c:
        sizes.append(c["lattice"])
    sizes += [c["spacing"] / 3.0, 2.0 * ext if ext > 0.0 else 1.0]
    return sizes


def params(table):
    """[(case name, k, loop)] over a table of cases."""
    return [(name, k, loop) for name, make in table.items() for c in (make(),) for k in c["ks"] for loop in c["loops"]]
