"""Float64 minimum-image brute force for the periodic radius graphs (ops.radius_csr(period=...) and its wrappers), and the
inputs tests/test_gpu_periodic_graph.py runs.  The reference has no periodic edge list to compare with (its torus_connectivity
shifts an alias of the grid and never wraps), so this is the checker:

    d = xs[:, None] - xd[None];  d -= L * round(d / L) on periodic axes;  edge (j -> i) where sum d^2 <= r^2, source-major.

Every input is also REFUSED if a pair lies within 1e-12 r^2 of the threshold: the kernel takes its differences from positions
reduced into the box, the oracle from the raw ones, and only a pair that close could be decided differently by the last bits -
with it excluded, a differing edge is a wrong edge.  tests/test_periodic_host.py runs this check over every case on the CPU."""
import numpy as np


def per_axis(v, dim):
    if v is None or np.isscalar(v):
        return np.full(dim, 0.0 if v is None else float(v))
    return np.array([0.0 if t is None else float(t) for t in v])


def periodic_edges(xs, r, period, xd=None):
    """(edge_index int64 [2, E] source-major, disp float64 [E, dim] = x_src - image(x_dst), norm float64 [E])."""
    xs = np.asarray(xs, dtype=np.float64).reshape(len(xs), -1)
    xd = xs if xd is None else np.asarray(xd, dtype=np.float64).reshape(len(xd), -1)
    dim = xs.shape[1]
    L = per_axis(period, dim)
    d = xs[:, None, :] - xd[None, :, :]
    for k in range(dim):
        if L[k] > 0.0:
            assert 2.0 * r < L[k], (r, L)
            d[..., k] -= L[k] * np.round(d[..., k] / L[k])
    d2 = (d * d).sum(-1)
    r2 = float(r) * float(r)
    near = np.abs(d2 - r2) <= 1e-12 * r2
    assert not near.any(), f"{int(near.sum())} pair(s) within 1e-12 r^2 of the threshold: not a fair input"
    s, t = np.nonzero(d2 <= r2)
    return np.stack([s, t]).astype(np.int64), d[s, t], np.sqrt(d2[s, t])


def geom_bound(period, r, dim):
    """Per column of geom [dim + 1]: one float32 ulp at magnitude period / 2 on a periodic axis; an open axis' difference and the
    norm are at most r.  Kernel and oracle round float64 values that agree up to their last bits to float32."""
    L = per_axis(period, dim)
    b = [np.spacing(np.float32(L[k] / 2.0 if L[k] > 0.0 else r)) for k in range(dim)]
    return np.array(b + [np.spacing(np.float32(r))], dtype=np.float64)


def _rng(seed):
    return np.random.default_rng(seed)


def _torus2d(n, seed, L=1.0):
    return _rng(seed).random((n, 2)) * L


def _long_row():
    g = _rng(11)
    rad, ang = 0.1 * np.sqrt(g.random(5000)), 2.0 * np.pi * g.random(5000)
    xs = np.stack([np.mod(rad * np.cos(ang), 1.0), np.mod(rad * np.sin(ang), 1.0)], axis=1)      # a disc around the corner (0, 0)
    xd = np.array([[0.02, 0.97], [0.98, 0.04], [0.0, 0.95]])
    return dict(xs=xs, xd=xd, r=0.3, period=1.0)


def _outside():
    g = _rng(12)
    x = g.random((300, 2))
    return dict(xs=x + g.integers(-3, 4, size=(300, 2)).astype(np.float64), r=0.13, period=1.0)


def _coincident():
    x = _torus2d(120, 13)
    x[40:80] = x[:40]                                    # 40 points twice
    x[80:90] = x[0]                                      # one point twelve times
    return dict(xs=x, r=0.24, period=1.0)


def _origin():
    o = np.array([-0.3, 0.7])
    return dict(xs=o + _torus2d(300, 14) * np.array([1.0, 1.5]), r=0.2, period=(1.0, 1.5), origin=(-0.3, 0.7))


def _mixed3d():
    return dict(xs=_rng(15).random((200, 3)) * np.array([1.0, 1.0, 2.0]), r=0.28, period=(1.0, 0.0, 2.0))


def _two_sets():
    return dict(xs=_torus2d(150, 16), xd=_torus2d(40, 17), r=0.24, period=1.0)


# name -> keyword arguments: xs, r, period, and optionally xd, origin
CASES = {
    "1d_64": lambda: dict(xs=_rng(1).random((64, 1)), r=0.06, period=1.0),
    "1d_one_point": lambda: dict(xs=np.array([[0.37]]), r=0.2, period=1.0),
    "2d_nc2": lambda: dict(xs=_torus2d(300, 2), r=0.45, period=1.0),
    "2d_nc3": lambda: dict(xs=_torus2d(300, 3), r=0.30, period=1.0),
    "2d_nc4": lambda: dict(xs=_torus2d(300, 4), r=0.24, period=1.0),
    "2d_nc7": lambda: dict(xs=_torus2d(300, 5), r=0.13, period=1.0),
    "3d_open_y": _mixed3d,
    "origin": _origin,
    "outside_box": _outside,
    "coincident": _coincident,
    "two_sets": _two_sets,
    "long_row": _long_row,
}


def lattice16():
    """The 16 x 16 lattice on [0, 1)^2 (dyadic: every difference and every wrap is exact), node id = 16 * iy + ix."""
    g = np.arange(16, dtype=np.float64) / 16.0
    return np.stack([np.tile(g, 16), np.repeat(g, 16)], axis=1)


def nested_levels_1d():
    """Three nested 1-D levels of 64, 32 and 16 points (each a prefix of the one above), their inner and inter-level radii."""
    x = _rng(21).random((64, 1))
    return [x, x[:32], x[:16]], [0.05, 0.11, 0.21], [0.08, 0.17]
