"""The independent checkers of the batched and the periodic k-nearest-neighbour graphs (graph_pde_amd.neighbor_graph:
knn_csr_batched / knn_graph_batched, knn_csr(period=...); csrc/gpde_knn_arms.hip) and the inputs of tests/test_knn_arms_host.py /
tests/test_gpu_knn_arms.py.  numpy only; it never calls the code under test.

    periodic   the complete bipartite edge list (self pairs dropped for loop=False on one point set), keys =
               neighbor_cap.d2_bits(neighbor_cap.d2_periodic(...)) - d = xs - xd, d -= L round(d / L) on the raw coordinates, squares
               summed in axis order - rows cut by neighbor_cap.select: knn_oracle.oracle with the other key.  Geometry: that d per
               axis and sqrt of the sum of squares, float64 rounded once to float32.
    batched    knn_oracle.oracle per graph, assembled with batched_graphs.assemble_csr.
"""
import numpy as np

from tests.helpers import batched_graphs as bg
from tests.helpers import knn_oracle as ko
from tests.helpers import neighbor_cap as nc
from tests.helpers import periodic_oracle as po

MAX_K = 256                 # GPDE_KNN_MAX_K


def periodic(xs, k, period, xd=None, loop=False):
    """(rowptr int64 [n_dst + 1], src int64 [E], dst int64 [E]) of the kNN graph on the torus, E = n_dst * k_eff."""
    xs = ko.as2d(xs)
    one = xd is None
    xd2 = xs if one else ko.as2d(xd)
    ns, nd = len(xs), len(xd2)
    ke = ko.k_eff(k, ns, one, loop)
    rowptr = np.arange(nd + 1, dtype=np.int64) * ke
    dst = np.repeat(np.arange(nd, dtype=np.int64), ke)
    if ke == 0 or nd == 0:
        return rowptr, np.zeros(0, dtype=np.int64), dst
    keep = np.ones((nd, ns), dtype=bool)
    if one and not loop:
        keep[np.arange(nd), np.arange(nd)] = False
    d, s = np.nonzero(keep)                                     # row-major: ascending source inside a row
    rp = np.zeros(nd + 1, dtype=np.int64)
    np.cumsum(np.bincount(d, minlength=nd), out=rp[1:])
    new, kept = nc.select(rp, nc.d2_bits(nc.d2_periodic(xs, None if one else xd2, s, d, period)), ke)
    assert np.array_equal(new, rowptr)
    return rowptr, s[kept], dst


def periodic_geometry(xs, xd, src, dst, period):
    """float32 [E, dim + 1]: the key's minimum-image difference per axis (source minus target) and its norm."""
    xs = ko.as2d(xs)
    xd = xs if xd is None else ko.as2d(xd)
    L = po.per_axis(period, xs.shape[1])
    cols, d2 = [], np.zeros(len(src))
    for a in range(xs.shape[1]):
        d = xs[src, a] - xd[dst, a]
        if L[a] > 0.0:
            d = d - L[a] * np.round(d / L[a])
        cols.append(d)
        d2 = d2 + d * d
    return np.stack(cols + [np.sqrt(d2)], axis=1).astype(np.float32).reshape(len(src), xs.shape[1] + 1)


def periodic_ks(c):
    """The k of a periodic case: 1, 8, 64, and - where the source set has at most 300 points - k = n and k = n + 3 (every source,
    and more than there are); a k past GPDE_KNN_MAX_K = 256 is refused by contract, so n = 300 runs at 256 in its place."""
    n = len(c["xs"])
    ks = [1, 8, 64]
    if n <= 300:
        ks += [min(n, MAX_K), min(n + 3, MAX_K)]
    return sorted(set(ks))


def periodic_cells(c):
    """The cell edges of a periodic case: automatic, L, L / 2, L / 3, L / 7 (grids of 1, 2, 3 and 7 cells on the axis of the
    longest period L) and a third of the typical spacing (many cells)."""
    dim = ko.as2d(c["xs"]).shape[1]
    L = float(po.per_axis(c["period"], dim).max())
    spacing = L / max(len(c["xs"]), 1) ** (1.0 / dim)
    return [None, L, L / 2.0, L / 3.0, L / 7.0, spacing / 3.0]


def outside_scaled():
    """periodic_oracle's `outside_box` with its whole-period offsets multiplied by 2^20: raw coordinates of magnitude 3 * 2^20."""
    g = np.random.default_rng(12)
    x = g.random((300, 2))
    return dict(xs=x + g.integers(-3, 4, size=(300, 2)).astype(np.float64) * float(1 << 20), period=1.0)


def ring8():
    """8 equally spaced points on a ring of length 1."""
    return np.arange(8, dtype=np.float64)[:, None] / 8.0


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def batched(pos, ptr, k, pos_dst=None, ptr_dst=None, loop=False):
    """(rowptr, src, dst, edge_ptr) int64 of the batch: knn_oracle.oracle per graph, assembled with global ids."""
    ss = bg.split(pos, ptr)
    dd = [None] * len(ss) if pos_dst is None else bg.split(pos_dst, ptr_dst)
    none = np.zeros(0, dtype=np.int64)
    per_graph = []
    for s, d in zip(ss, dd):
        nd = len(s) if d is None else len(d)
        if len(s) == 0 or nd == 0:                              # no source or no destination: rows without edges
            per_graph.append((np.zeros(nd + 1, dtype=np.int64), none, none))
        else:
            per_graph.append(ko.oracle(s, k, d, loop))
    return bg.assemble_csr(per_graph, ptr, ptr_dst)


def batch_k_eff(ptr, k, one_set, loop):
    return [ko.k_eff(k, int(ptr[b + 1] - ptr[b]), one_set, loop) for b in range(len(ptr) - 1)]


def _scaled():
    x = np.random.default_rng(71).random((200, 2))
    return bg.concat_sets([x * 1e-3, x * 1e3], 2)


def _two_sets():
    pos, ptr = bg.unit_box_batch()
    pd, ptr_dst = bg.unit_box_batch(sizes=(20, 5, 0, 64, 7), seed=12)      # graph 1: destinations without sources; graph 2: the reverse
    return dict(pos=pos, ptr=ptr, pos_dst=pd, ptr_dst=ptr_dst)


def _lattices():
    return bg.concat_sets([ko.lattice9(), ko.lattice9((0.1, 0.3)), ko.lattice9((-2.0, 5.0))], 2)


UNIT_KS = (1, 5, 36, 37, 64, 200)

# name -> pos, ptr, optional pos_dst / ptr_dst, ks, loops, spacing (the typical point spacing of the finest graph)
BATCHES = {
    "unit_box": lambda: dict(zip(("pos", "ptr"), bg.unit_box_batch()), ks=UNIT_KS, loops=(False, True), spacing=0.09),
    "two_sets": lambda: dict(_two_sets(), ks=UNIT_KS, loops=(False,), spacing=0.09),
    "lattices": lambda: dict(zip(("pos", "ptr"), _lattices()), ks=ko.LATTICE_KS, loops=(False, True), spacing=0.125),
    "scaled": lambda: dict(zip(("pos", "ptr"), _scaled()), ks=(1, 16, 200), loops=(False,), spacing=0.07e-3),
    "b0": lambda: dict(pos=np.zeros((0, 2)), ptr=np.zeros(1, dtype=np.int64), ks=(3,), loops=(False, True), spacing=1.0),
    "b1": lambda: dict(zip(("pos", "ptr"), bg.unit_box_batch(sizes=(130,))), ks=(1, 16, 200), loops=(False, True), spacing=0.09),
}


def batch_cells(c):
    """The cell edges every batch runs under: automatic per graph, a third of the spacing, twice the extent of the whole batch."""
    pts = c["pos"] if "pos_dst" not in c else np.concatenate([c["pos"], c["pos_dst"]])
    ext = float((pts.max(axis=0) - pts.min(axis=0)).max()) if len(pts) else 0.0
    return [None, c["spacing"] / 3.0, 2.0 * ext if ext > 0.0 else 1.0]


def batch_bounds(c):
    """Host [B, 2, dim]: a box around both point sets of every graph (zeros for a graph without points)."""
    ptr = c["ptr"]
    out = np.zeros((len(ptr) - 1, 2, c["pos"].shape[1]))
    for b in range(len(ptr) - 1):
        pts = c["pos"][ptr[b]:ptr[b + 1]]
        if "pos_dst" in c:
            pts = np.concatenate([pts, c["pos_dst"][c["ptr_dst"][b]:c["ptr_dst"][b + 1]]])
        if len(pts):
            out[b, 0], out[b, 1] = pts.min(axis=0), pts.max(axis=0)
    return out
