"""The independent checker of the capped in-degree (ops.select_in_edges, edge_sqdist_keys, edge_hash_keys, radius_csr(...,
max_num_neighbors=k)) and the inputs tests/test_gpu_neighbor_cap.py runs.  numpy only; it never calls the code under test.

    d2        float64, open box: d = xd[i][a] - xs[j][a], d2 += d * d in axis order (numpy does not fuse) - the arithmetic the
              header states, so the bits agree; periodic box: d = xs[j] - xd[i] on the RAW coordinates, d -= L round(d / L), as in
              tests/helpers/periodic_oracle.py (the form the header states for the key);
    hash      the counter-based mix restated from the constants of include/gpde.h (read from the header text), uint64 arithmetic;
    select    per row the k smallest (key, slot) by np.lexsort, returned in ascending slot order.

A periodic "nearest" input is FAIR for a cap k when, in every row longer than k, the k-th and (k + 1)-th smallest oracle d2
differ by more than 1e-12 r^2: then the last bits of d2 cannot change the selection.  tests/test_neighbor_cap_host.py asserts it
for every input below on the CPU; the GPU tests then leave no case out.  Open-box inputs need no such condition (bit-reproducible
d2; ties, as on a lattice, are decided by slot)."""
import os
import re

import numpy as np

from tests.helpers import periodic_oracle as po

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def header_constants():
    """(GPDE_HASH_SEED_MUL, GPDE_HASH_MUL1, GPDE_HASH_MUL2) as Python ints, from the text of include/gpde.h."""
    src = open(os.path.join(REPO, "include", "gpde.h")).read()
    return tuple(int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+)" % n, src).group(1), 16)
                 for n in ("GPDE_HASH_SEED_MUL", "GPDE_HASH_MUL1", "GPDE_HASH_MUL2"))


def hash_keys(src, dst, seed):
    """int64 [E]: the header's hash of (seed, dst id, src id), in uint64 array arithmetic (wraps mod 2^64)."""
    c0, c1, c2 = (np.uint64(c) for c in header_constants())
    s = np.asarray(src).astype(np.int64).astype(np.uint64)
    d = np.asarray(dst).astype(np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = np.full(s.shape, int(seed) % (1 << 64), dtype=np.uint64) * c0 + ((d << np.uint64(32)) | s)
        z = (z ^ (z >> np.uint64(30))) * c1
        z = (z ^ (z >> np.uint64(27))) * c2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(1)).astype(np.int64)


def hash_key_bigint(src, dst, seed):
    """The same for one edge in Python's unbounded integers: every product reduced mod 2^64 by hand."""
    c0, c1, c2 = header_constants()
    m = (1 << 64) - 1
    z = ((int(seed) & m) * c0 + ((int(dst) << 32) | int(src))) & m
    z = ((z ^ (z >> 30)) * c1) & m
    z = ((z ^ (z >> 27)) * c2) & m
    z ^= z >> 31
    return z >> 1


def d2_open(xs, xd, src, dst):
    xs = np.asarray(xs, dtype=np.float64).reshape(len(xs), -1)
    xd = xs if xd is None else np.asarray(xd, dtype=np.float64).reshape(len(xd), -1)
    d2 = np.zeros(len(src), dtype=np.float64)
    for a in range(xs.shape[1]):
        d = xd[dst, a] - xs[src, a]
        d2 = d2 + d * d
    return d2


def d2_periodic(xs, xd, src, dst, period):
    xs = np.asarray(xs, dtype=np.float64).reshape(len(xs), -1)
    xd = xs if xd is None else np.asarray(xd, dtype=np.float64).reshape(len(xd), -1)
    L = po.per_axis(period, xs.shape[1])
    d2 = np.zeros(len(src), dtype=np.float64)
    for a in range(xs.shape[1]):
        d = xs[src, a] - xd[dst, a]
        if L[a] > 0.0:
            d = d - L[a] * np.round(d / L[a])
        d2 = d2 + d * d
    return d2


def d2_bits(d2):
    return np.ascontiguousarray(d2, dtype=np.float64).view(np.int64)


def select(rowptr, key, k):
    """(rowptr_new int64 [n + 1], kept slots int64 [E'] ascending): per row the k smallest (key, slot).  `key`: any numpy array
    that sorts (int64, or floats: -0.0 == 0.0, so such a tie goes to the slot)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n, e = len(rowptr) - 1, int(rowptr[-1])
    key = np.asarray(key)
    assert key.shape == (e,)
    slot = np.arange(e, dtype=np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    order = np.lexsort((slot, key, row))                    # row-major, then key, then slot
    rank = np.arange(e, dtype=np.int64) - rowptr[row[order]]
    kept = np.sort(order[rank < k])
    new = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.minimum(np.diff(rowptr), k), out=new[1:])
    assert len(kept) == new[-1]
    return new, kept


def csr_of_edges(ei, n_dst):
    """(rowptr, src, dst) of an edge list int64 [2, E]: rows by destination, ascending source inside a row."""
    order = np.lexsort((ei[0], ei[1]))
    src, dst = ei[0][order], ei[1][order]
    rowptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
    return rowptr, src, dst


def brute_open_edges(xs, r, xd=None):
    """edge_index int64 [2, E] of the open radius graph by the exact arithmetic, from the positions alone."""
    xs = np.asarray(xs, dtype=np.float64).reshape(len(xs), -1)
    xd = xs if xd is None else np.asarray(xd, dtype=np.float64).reshape(len(xd), -1)
    d2 = np.zeros((len(xs), len(xd)))
    for a in range(xs.shape[1]):
        d = xd[None, :, a] - xs[:, None, a]
        d2 = d2 + d * d
    s, t = np.nonzero(d2 <= float(r) * float(r))
    return np.stack([s, t]).astype(np.int64)


def unfair_rows(rowptr, d2, k, r):
    """Rows longer than k whose k-th and (k + 1)-th smallest d2 are within 1e-12 r^2 of each other."""
    bad = []
    for i in range(len(rowptr) - 1):
        v = np.sort(d2[rowptr[i]:rowptr[i + 1]])
        if len(v) > k and not v[k] - v[k - 1] > 1e-12 * r * r:
            bad.append(i)
    return bad


# ---- inputs of the GPU tier ------------------------------------------------------------------------------------------------------
# periodic "nearest": case of periodic_oracle.CASES -> the caps it runs with (each fair: tests/test_neighbor_cap_host.py)
PERIODIC_NEAREST = {
    "1d_64": (4,),
    "2d_nc2": (32,),
    "2d_nc3": (8, 64),
    "2d_nc4": (16,),
    "2d_nc7": (8,),
    "3d_open_y": (8,),
    "origin": (16,),
    "outside_box": (8,),
    "two_sets": (8,),
    "long_row": (100,),
}


def periodic_case(name):
    """(case dict, rowptr, src, dst, oracle d2 per slot) of a periodic input: the brute-force graph, rows in ascending source order."""
    c = po.CASES[name]()
    xs = np.asarray(c["xs"], dtype=np.float64)
    n_dst = len(c["xd"]) if "xd" in c else len(xs)
    ei = po.periodic_edges(xs, c["r"], c["period"], xd=c.get("xd"))[0]
    rowptr, src, dst = csr_of_edges(ei, n_dst)
    return c, rowptr, src, dst, d2_periodic(xs, c.get("xd"), src, dst, c["period"])


def _rng(seed):
    return np.random.default_rng(seed)


def _hub():
    """5,000 sources in a disc of radius 0.09 around one destination, 300 more spread over the unit square: the hub row is past the
    builders' LDS row sort (4096), so its slots are in cell order."""
    g = _rng(33)
    rad, ang = 0.09 * np.sqrt(g.random(5000)), 2.0 * np.pi * g.random(5000)
    disc = np.array([0.5, 0.5]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    return dict(xs=np.concatenate([disc, g.random((300, 2))]), xd=np.array([[0.5, 0.5], [0.52, 0.47], [0.1, 0.9]]), r=0.1, ks=(64, 4500))


# open boxes: name -> xs, r, optional xd, and the caps `ks`
OPEN_CASES = {
    "1d_300": lambda: dict(xs=_rng(31).random((300, 1)), r=0.05, ks=(1, 8)),
    "2d_2000": lambda: dict(xs=_rng(32).random((2000, 2)), r=0.06, ks=(8, 16)),
    "3d_700": lambda: dict(xs=_rng(34).random((700, 3)), r=0.2, ks=(8, 20)),
    "two_sets": lambda: dict(xs=_rng(35).random((900, 2)), xd=_rng(36).random((130, 2)), r=0.12, ks=(5, 32)),
    "lattice16": lambda: dict(xs=po.lattice16(), r=0.2, ks=(4, 9, 21)),              # dyadic: whole shells of equal d2, ties by slot
    "coincident": lambda: dict(xs=np.repeat(_rng(37).random((60, 2)), 3, axis=0), r=0.3, ks=(2, 7)),
    "hub_5000": _hub,
}


def batch_case():
    """A batch of 5 graphs in 2-D, one of them empty, with per-graph radii: (positions [n, 2], ptr [6], radii [5])."""
    g = _rng(41)
    sizes = [300, 0, 450, 1, 250]
    pos = np.concatenate([g.random((s, 2)) for s in sizes])
    return pos, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), [0.1, 0.2, 0.08, 0.3, 0.15]


LDS_KEYS = 2048        # rows of up to this many keys are staged in LDS by gpde_csr_select_k (gpde_select.hip SEL_LDS_KEYS)
SELECT_KS = (1, 2, 31, 32, 33, 64, 65, 100, 5000)


def synthetic_rows(k):
    """rowptr int64 of the row lengths the select kernel can go wrong at, for cap k."""
    lens = [0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, 127, 129, LDS_KEYS - 1, LDS_KEYS, LDS_KEYS + 1, 10000, 0, 3]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def synthetic_keys(kind, e, seed):
    g = _rng(seed)
    if kind == "int64":
        return g.integers(-(1 << 63), (1 << 63) - 1, size=e, dtype=np.int64, endpoint=True)
    if kind == "three_values":                               # ties span the wave's chunks of 64
        return np.array([-7, 0, 1 << 40], dtype=np.int64)[g.integers(0, 3, size=e)]
    if kind == "all_equal":
        return np.full(e, -5, dtype=np.int64)
    assert kind == "float"
    v = g.standard_normal(e).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0], dtype=np.float32)
    pick = g.random(e) < 0.2
    v[pick] = special[g.integers(0, len(special), size=int(pick.sum()))]
    return v


KEY_KINDS = ("int64", "three_values", "all_equal", "float")
