"""k-nearest-neighbour graphs built natively as the operator's CSR: the counterpart of PyG's `knn_graph` / `knn`.

`knn_csr` runs gpde_knn_csr (csrc/gpde_knn.hip; include/gpde.h states the contract): row i holds the k_eff sources j with the
smallest (d2_bits(j, i), j),

    d2      the float64 squared distance in the arithmetic of ops.edge_sqdist_keys (open box): d = pos_dst[i][a] - pos[j][a],
            d2 += d * d in axis order; d2_bits its int64 bit pattern; ties go to the smaller source id
    k_eff   min(k, n_src); on one point set with loop=False the point itself is excluded by id and k_eff = min(k, n_src - 1)

which is `ops.select_in_edges` applied to the complete bipartite graph - without forming it, and without the radius that
`ops.radius_csr(pos, r, max_num_neighbors=k, select="nearest")` needs: a radius that holds k sources around the loneliest
destination forms quadratically many candidates in the dense parts of a non-uniform cloud.  Every row has k_eff edges, so
E = n_dst k_eff is known on the host and the build needs no synchronisation: with `bounds=` given, a graph over moving points is
rebuilt on the caller's stream without the host ever waiting (DESIGN.md §6e "The nearest arm").

Periodic boxes and batched point sets have no form here.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib, ops

__all__ = ["knn_csr", "knn_graph"]

MAX_K = 256                 # GPDE_KNN_MAX_K of include/gpde.h: the k best pairs of a wave are kept in LDS


def _dim_of(t, name: str) -> int:
    if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name} must be a tensor [n, dim] (or [n]: one dimension) (got {got})")
    return 1 if t.dim() == 1 else int(t.size(1))


def k_eff(k: int, n_src: int, one_set: bool, loop: bool) -> int:
    """Edges per row: min(k, n_src), and min(k, n_src - 1) on one point set without self loops (never negative)."""
    return max(0, min(int(k), int(n_src) - (1 if one_set and not loop else 0)))


def _box(bounds, dim: int):
    """`bounds=(lo, hi)`, each a number (every axis) or one entry per axis, as two lists of `dim` floats (ValueError)."""
    if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
        raise ValueError(f"bounds must be a pair (lo, hi) (got {bounds!r})")
    out = []
    for v, name in zip(bounds, ("lo", "hi")):
        if isinstance(v, torch.Tensor):
            if v.is_cuda:
                raise ValueError(f"bounds: {name} is a device tensor - the box is host data (pass numbers; bounds=None reads it from the points)")
            v = v.tolist()
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            v = [v] * dim
        try:
            v = [float(t) for t in v]
        except (TypeError, ValueError):
            raise ValueError(f"bounds: {name} must be a number or {dim} numbers (got {v!r})") from None
        if len(v) != dim:
            raise ValueError(f"bounds: {name} has {len(v)} entries for positions of dimension {dim}")
        out.append(v)
    lo, hi = out
    for a in range(dim):
        if not (math.isfinite(lo[a]) and math.isfinite(hi[a]) and hi[a] >= lo[a] and math.isfinite(hi[a] - lo[a])):
            raise ValueError(f"bounds: the box [{lo[a]}, {hi[a]}] on axis {a} is empty or not finite")
    return lo, hi


def _host_args(pos, k, pos_dst, loop, bounds, cell_size):
    """Every refusal that needs no device (ValueError): (k, loop, (lo, hi) lists or None, cell edge or 0, dim)."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an int in 1 .. {MAX_K} (got {k!r})")
    if not isinstance(loop, bool):
        raise ValueError(f"loop must be True or False (got {loop!r})")
    dim = _dim_of(pos, "pos")
    if not 1 <= dim <= 3:
        raise ValueError(f"positions of dimension {dim}: the nearest-neighbour graphs are built in 1..3 dimensions")
    if pos_dst is not None:
        if _dim_of(pos_dst, "pos_dst") != dim:
            raise ValueError("pos and pos_dst must have the same dimension")
        if loop:
            raise ValueError("loop=True with pos_dst: two point sets have no self pairs (loop belongs to one point set)")
    cell = 0.0
    if cell_size is not None:
        if isinstance(cell_size, bool) or not isinstance(cell_size, (int, float)):
            raise ValueError(f"cell_size must be a positive finite number (got {cell_size!r})")
        cell = float(cell_size)
        if not (cell > 0.0 and math.isfinite(cell) and math.isfinite(1.0 / cell)):
            raise ValueError(f"cell_size = {cell} must be positive and finite (and so must its reciprocal)")
    box = None if bounds is None else _box(bounds, dim)
    n_src = int(pos.size(0))
    n_dst = n_src if pos_dst is None else int(pos_dst.size(0))
    ke = k_eff(k, n_src, pos_dst is None, loop)
    if n_dst * ke > (1 << 31) - 65:
        raise ValueError(f"n_dst * k_eff = {n_dst * ke} edges exceed the int32 CSR")
    return k, loop, box, cell, dim, ke


def _build(pos, k, pos_dst, loop, bounds, cell_size, geometry: bool):
    """gpde_knn_csr on the caller's current stream: (rowptr, src, dst, geom | None, k_eff)."""
    k, loop, box, cell, dim, ke = _host_args(pos, k, pos_dst, loop, bounds, cell_size)
    one_set = pos_dst is None
    pos, pd = ops._positions(pos, pos_dst)
    n, nd = int(pos.size(0)), int(pd.size(0))
    dev = pos.device
    e = nd * ke
    src = torch.empty(e, dtype=torch.int32, device=dev)
    dst = torch.empty(e, dtype=torch.int32, device=dev)
    geom = torch.empty(e, dim + 1, dtype=torch.float32, device=dev) if geometry else None
    if e == 0:
        return torch.zeros(nd + 1, dtype=torch.int32, device=dev), src, dst, geom, ke
    if box is None:
        lo, hi = ops._host_bounds(pos, pd)                # the call's only synchronisation
    else:
        lo, hi = (ctypes.c_double * dim)(*box[0]), (ctypes.c_double * dim)(*box[1])
    lib = _lib.lib()
    nbytes = int(lib.gpde_knn_csr_workspace_bytes(n, nd, dim, k, cell, lo, hi))
    if nbytes == 0:
        _lib.check(-1, "gpde_knn_csr_workspace_bytes")
    ws = ops._alloc_ws(nbytes, dev)
    rowptr = torch.empty(nd + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        # two point sets go in as loop = 1: nothing is excluded, whatever the two addresses are
        _lib.check(lib.gpde_knn_csr(pos.data_ptr(), n, pos.data_ptr() if one_set else pd.data_ptr(), nd, dim, k,
                                    1 if (loop or not one_set) else 0, cell, lo, hi, rowptr.data_ptr(), src.data_ptr(),
                                    dst.data_ptr(), ops._ptr(geom), ws.data_ptr(), ws.numel(), ops._stream_ptr(dev)),
                   "gpde_knn_csr")
    return rowptr, src, dst, geom, ke


def knn_csr(pos: torch.Tensor, k: int, *, pos_dst: Optional[torch.Tensor] = None, loop: bool = False, bounds=None,
            cell_size: Optional[float] = None, return_geometry: bool = False):
    """The exact k-nearest-neighbour graph of `pos` [n, dim] (dim 1..3, k <= 256) as the `ops.Csr` the operator consumes: row i
    holds the k_eff nearest sources of point i (the module docstring states distance, ties and k_eff), in ascending source
    order; `perm` is the identity; every row has the same length, `rowptr[i] = i * k_eff`.

    `pos_dst`: a second point set - the k nearest sources (in `pos`) of every point of `pos_dst`, level-local ids; the result is
    the rectangular Csr (`n_src_nodes` set), consumed as `conv((x_src, x_dst), csr, edge_attr)` like `ops.radius_csr(pos, r,
    pos_dst=)`.  `loop=True` (one point set only) lets a point be its own neighbour - at distance 0 it always is.
    `bounds=(lo, hi)`: the box of the cell grid as host numbers (one per axis, or one for all).  With it the call performs no
    host synchronisation of any kind; without it the box is read from the points, the call's only synchronisation.  Points
    outside the box are allowed (they are binned into the border cells): the box changes speed, never the result.
    `cell_size` overrides the automatic cell edge (a mean of max(2, k / 2) sources per cell); it, too, changes speed only.
    `return_geometry=True` returns (Csr, geom): geom float32 [E, dim + 1] by CSR slot, the displacement pos[src] - pos_dst[dst]
    and its norm - the rows `ops.radius_csr(..., return_geometry=True)` gives these edges, bit for bit."""
    rowptr, src, dst, geom, ke = _build(pos, k, pos_dst, loop, bounds, cell_size, bool(return_geometry))
    e = int(src.numel())
    csr = ops.Csr(int(rowptr.numel()) - 1, e, rowptr, src, dst, torch.arange(e, dtype=torch.int32, device=src.device),
                  _max_in_degree=ke if e else 0, n_src_nodes=None if pos_dst is None else int(pos.size(0)))
    return (csr, geom) if return_geometry else csr


def knn_graph(pos: torch.Tensor, k: int, *, pos_dst: Optional[torch.Tensor] = None, loop: bool = False, bounds=None,
              cell_size: Optional[float] = None) -> torch.Tensor:
    """edge_index int64 [2, E] of the same graph in the reference's order (sorted by source, then target), as `ops.radius_graph`
    gives the radius graph: `knn_csr(...).edge_index` stably sorted by source."""
    _, src, dst, _, _ = _build(pos, k, pos_dst, loop, bounds, cell_size, False)
    order = torch.sort(src, stable=True).indices          # rows are destination-major: targets stay ascending per source
    return torch.stack([src[order].long(), dst[order].long()])
