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

Two further arms (csrc/gpde_knn_arms.hip; DESIGN.md §6e "The batched nearest arm", "The periodic nearest arm"):

    period=   `knn_csr(pos, k, period=L)` is the graph on a torus: on a periodic axis d = pos[j][a] - pos_dst[i][a],
              d -= L round(d / L) on the raw coordinates - the periodic key of ops.edge_sqdist_keys - and every source is a
              candidate once, at its minimum image.  No radius, no `2 r < period`: k may reach every source on the torus.
    batched   `knn_csr_batched(pos, ptr, k)` builds the graphs of B point sets in one call: the per-graph `knn_csr` results
              concatenated with their offsets, bit for bit, E and edge_ptr known on the host from `ptr` alone.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib, ops

__all__ = ["knn_csr", "knn_graph"]       # the single-graph builders; knn_csr_batched / knn_graph_batched are the module's other two

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


def _scalars(k, loop, cell_size) -> float:
    """k, loop and cell_size of every builder here (ValueError); the cell edge, 0.0 for the automatic one."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an int in 1 .. {MAX_K} (got {k!r})")
    if not isinstance(loop, bool):
        raise ValueError(f"loop must be True or False (got {loop!r})")
    cell = 0.0
    if cell_size is not None:
        if isinstance(cell_size, bool) or not isinstance(cell_size, (int, float)):
            raise ValueError(f"cell_size must be a positive finite number (got {cell_size!r})")
        cell = float(cell_size)
        if not (cell > 0.0 and math.isfinite(cell) and math.isfinite(1.0 / cell)):
            raise ValueError(f"cell_size = {cell} must be positive and finite (and so must its reciprocal)")
    return cell


def _dims(pos, pos_dst, loop) -> int:
    """The dimension of one or two point sets (ValueError for what the builders do not take)."""
    dim = _dim_of(pos, "pos")
    if not 1 <= dim <= 3:
        raise ValueError(f"positions of dimension {dim}: the nearest-neighbour graphs are built in 1..3 dimensions")
    if pos_dst is not None:
        if _dim_of(pos_dst, "pos_dst") != dim:
            raise ValueError("pos and pos_dst must have the same dimension")
        if loop:
            raise ValueError("loop=True with pos_dst: two point sets have no self pairs (loop belongs to one point set)")
    return dim


def _host_args(pos, k, pos_dst, loop, bounds, cell_size, period=None, origin=None):
    """Every refusal that needs no device (ValueError): (k, loop, (lo, hi) lists or None, cell edge or 0, dim, k_eff, torus),
    torus = (period, origin) as two lists of dim floats, or None when no axis wraps."""
    cell = _scalars(k, loop, cell_size)
    dim = _dims(pos, pos_dst, loop)
    box = None if bounds is None else _box(bounds, dim)
    torus = None
    if period is not None or origin is not None:
        per, org = ops._key_box(period, origin, dim)          # the rule of ops.periodic_box: a scalar is every axis, 0 / None an open one
        torus = (per, org) if any(per) else None
    n_src = int(pos.size(0))
    n_dst = n_src if pos_dst is None else int(pos_dst.size(0))
    ke = k_eff(k, n_src, pos_dst is None, loop)
    if n_dst * ke > (1 << 31) - 65:
        raise ValueError(f"n_dst * k_eff = {n_dst * ke} edges exceed the int32 CSR")
    return k, loop, box, cell, dim, ke, torus


def _build(pos, k, pos_dst, loop, bounds, cell_size, geometry: bool, period=None, origin=None):
    """gpde_knn_csr (gpde_knn_csr_periodic where an axis wraps) on the caller's current stream: (rowptr, src, dst, geom | None, k_eff)."""
    k, loop, box, cell, dim, ke, torus = _host_args(pos, k, pos_dst, loop, bounds, cell_size, period, origin)
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
    if box is not None:
        lo, hi = (ctypes.c_double * dim)(*box[0]), (ctypes.c_double * dim)(*box[1])
    elif torus is not None and all(torus[0]):
        lo = hi = None                                    # every axis wraps: no box is read, nothing to wait for
    else:
        lo, hi = ops._host_bounds(pos, pd)                # the call's only synchronisation
    lib = _lib.lib()
    if torus is not None:
        per, org = (ctypes.c_double * dim)(*torus[0]), (ctypes.c_double * dim)(*torus[1])
        nbytes = int(lib.gpde_knn_csr_periodic_workspace_bytes(n, nd, dim, k, cell, lo, hi, org, per))
        if nbytes == 0:
            _lib.check(-1, "gpde_knn_csr_periodic_workspace_bytes")
        ws = ops._alloc_ws(nbytes, dev)
        rowptr = torch.empty(nd + 1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gpde_knn_csr_periodic(pos.data_ptr(), n, pos.data_ptr() if one_set else pd.data_ptr(), nd, dim, k,
                                                 1 if (loop or not one_set) else 0, cell, lo, hi, org, per, rowptr.data_ptr(),
                                                 src.data_ptr(), dst.data_ptr(), ops._ptr(geom), ws.data_ptr(), ws.numel(),
                                                 ops._stream_ptr(dev)), "gpde_knn_csr_periodic")
        return rowptr, src, dst, geom, ke
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
            cell_size: Optional[float] = None, return_geometry: bool = False, period=None, origin=None):
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
    and its norm - the rows `ops.radius_csr(..., return_geometry=True)` gives these edges, bit for bit.
    `period` / `origin` (as in `ops.radius_csr`: a number for every axis or one entry per axis, 0 / None = an open axis): the
    graph on a torus (gpde_knn_csr_periodic) - the module docstring states the key.  Points anywhere on the real line are legal;
    `origin` only anchors the cell grid and `bounds` is read on open axes only: the graph depends on neither, and with every axis
    periodic the call never synchronises.  geom is then taken in the key's arithmetic (the minimum-image d per axis and
    sqrt(sum d^2)): `ops.radius_csr(period=, return_geometry=True)` reduces both points into the box first and agrees with it
    up to the last bits only."""
    rowptr, src, dst, geom, ke = _build(pos, k, pos_dst, loop, bounds, cell_size, bool(return_geometry), period, origin)
    e = int(src.numel())
    csr = ops.Csr(int(rowptr.numel()) - 1, e, rowptr, src, dst, torch.arange(e, dtype=torch.int32, device=src.device),
                  _max_in_degree=ke if e else 0, n_src_nodes=None if pos_dst is None else int(pos.size(0)))
    return (csr, geom) if return_geometry else csr


def knn_graph(pos: torch.Tensor, k: int, *, pos_dst: Optional[torch.Tensor] = None, loop: bool = False, bounds=None,
              cell_size: Optional[float] = None, period=None, origin=None) -> torch.Tensor:
    """edge_index int64 [2, E] of the same graph in the reference's order (sorted by source, then target), as `ops.radius_graph`
    gives the radius graph: `knn_csr(...).edge_index` stably sorted by source."""
    _, src, dst, _, _ = _build(pos, k, pos_dst, loop, bounds, cell_size, False, period, origin)
    order = torch.sort(src, stable=True).indices          # rows are destination-major: targets stay ascending per source
    return torch.stack([src[order].long(), dst[order].long()])


# ----------------------------------------------------------------------------------------------
# the kNN graphs of a BATCH of point sets in one build (gpde_knn_csr_batched)
# ----------------------------------------------------------------------------------------------
def batch_slots(ptr, ptr_dst, k: int, one_set: bool, loop: bool):
    """(k_eff int64 [B], edge_ptr int64 [B + 1]) of a batch, host arithmetic on the host `ptr` tensors alone:
    k_eff[b] = k_eff(k, ns_b, ...), edge_ptr[b + 1] = edge_ptr[b] + nd_b k_eff[b]."""
    ns = ptr[1:] - ptr[:-1]
    nd = ns if ptr_dst is None else ptr_dst[1:] - ptr_dst[:-1]
    ke = torch.clamp(torch.clamp(ns - (1 if one_set and not loop else 0), max=int(k)), min=0)
    edge_ptr = torch.zeros(int(ptr.numel()), dtype=torch.int64)
    torch.cumsum(nd * ke, 0, out=edge_ptr[1:])
    return ke, edge_ptr


def _batched_host_args(pos, ptr, k, pos_dst, ptr_dst, loop, bounds, cell_size, single_graph_only):
    """Every refusal of the batched builders that needs no device (ValueError)."""
    for name in single_graph_only:
        if name in ("period", "origin"):
            raise ValueError(f"{name}= has no batched form: a periodic box keeps its single-graph form (knn_csr(period=...), one call per graph)")
        raise TypeError(f"unexpected keyword argument {name!r}")
    cell = _scalars(k, loop, cell_size)
    if ptr_dst is not None and pos_dst is None:
        raise ValueError("ptr_dst given without pos_dst: a second ptr needs the second point set it divides")
    if pos_dst is not None and ptr_dst is None:
        raise ValueError("pos_dst given without ptr_dst: the second point set needs its own division into graphs")
    dim = _dims(pos, pos_dst, loop)
    ptr_h = ops._host_ptr(ptr, "ptr", int(pos.size(0)))
    n_graphs = int(ptr_h.numel()) - 1
    ptr_dst_h = None
    if pos_dst is not None:
        ptr_dst_h = ops._host_ptr(ptr_dst, "ptr_dst", int(pos_dst.size(0)))
        if int(ptr_dst_h.numel()) != n_graphs + 1:
            raise ValueError(f"ptr_dst divides pos_dst into {int(ptr_dst_h.numel()) - 1} graphs, ptr divides pos into {n_graphs}")
    ke, edge_ptr = batch_slots(ptr_h, ptr_dst_h, k, pos_dst is None, loop)
    if int(edge_ptr[-1]) > (1 << 31) - 65:
        raise ValueError(f"sum of nd_b * k_eff[b] = {int(edge_ptr[-1])} edges exceed the int32 CSR")
    box = None
    if bounds is not None:
        if isinstance(bounds, torch.Tensor) and bounds.is_cuda:
            raise ValueError("bounds is a device tensor - the per-graph boxes are host data [B, 2, dim] (bounds=None reads them from the points)")
        try:
            box = torch.as_tensor(bounds, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"bounds must be host data [B, 2, dim] = [{n_graphs}, 2, {dim}]") from None
        if tuple(box.shape) != (n_graphs, 2, dim):
            raise ValueError(f"bounds has shape {tuple(box.shape)}, the per-graph boxes are [B, 2, dim] = [{n_graphs}, 2, {dim}]")
        box = box.contiguous()
        ok = torch.isfinite(box).all(dim=(1, 2)) & (box[:, 1] >= box[:, 0]).all(dim=1) & torch.isfinite(box[:, 1] - box[:, 0]).all(dim=1)
        bad = (~ok & (ptr_h[1:] > ptr_h[:-1])).nonzero()
        if bad.numel():
            raise ValueError(f"bounds: the box of graph {int(bad[0])} is empty or not finite")
    return cell, dim, ptr_h, ptr_dst_h, ke, edge_ptr, box


def _upload(t: torch.Tensor, dev) -> torch.Tensor:
    """A small host tensor on the device without the host waiting: through pinned memory, on the current stream."""
    return t.pin_memory().to(dev, non_blocking=True)


def _device_boxes(pos, pd, ptr_d, ptr_dst_d, n_graphs: int, dim: int) -> torch.Tensor:
    """Host [B, 2, dim]: the per-graph boxes of both point sets, reduced on the device and copied once (graphs without points
    keep +-inf: the plan does not read the box of a graph without sources)."""
    inf = float("inf")
    lo = torch.full((n_graphs, dim), inf, dtype=torch.float64, device=pos.device)
    hi = torch.full((n_graphs, dim), -inf, dtype=torch.float64, device=pos.device)
    for p, pt in ((pos, ptr_d),) if pd is pos else ((pos, ptr_d), (pd, ptr_dst_d)):
        if p.size(0) > 0 and n_graphs > 0:
            gid = ops._graph_ids(pt, int(p.size(0))).unsqueeze(1).expand(-1, dim).contiguous()
            lo.scatter_reduce_(0, gid, p, "amin")
            hi.scatter_reduce_(0, gid, p, "amax")
    return torch.stack([lo, hi], dim=1).cpu()


def _build_batched(pos, ptr, k, pos_dst, ptr_dst, loop, bounds, cell_size, geometry: bool, single_graph_only):
    """gpde_knn_csr_batched on the caller's current stream: (rowptr, src, dst, geom | None, edge_ptr on the device, max k_eff)."""
    cell, dim, ptr_h, ptr_dst_h, ke, edge_ptr, box = _batched_host_args(pos, ptr, k, pos_dst, ptr_dst, loop, bounds, cell_size,
                                                                          single_graph_only)
    one_set = pos_dst is None
    pos, pd = ops._positions(pos, pos_dst)
    n, nd, n_graphs = int(pos.size(0)), int(pd.size(0)), int(ptr_h.numel()) - 1
    dev = pos.device
    e = int(edge_ptr[-1])
    ke_max = int(ke.max()) if n_graphs > 0 else 0
    src = torch.empty(e, dtype=torch.int32, device=dev)
    dst = torch.empty(e, dtype=torch.int32, device=dev)
    geom = torch.empty(e, dim + 1, dtype=torch.float32, device=dev) if geometry else None
    edge_ptr_d = _upload(edge_ptr, dev)
    if e == 0:
        return torch.zeros(nd + 1, dtype=torch.int32, device=dev), src, dst, geom, edge_ptr_d, 0
    if box is None:                                       # the call's only synchronisation
        ptr_d = _upload(ptr_h, dev)
        box = _device_boxes(pos, pd, ptr_d, ptr_d if one_set else _upload(ptr_dst_h, dev), n_graphs, dim)
    lib = _lib.lib()
    table_h = torch.zeros(n_graphs * _lib.GPDE_KNN_BATCHED_REC_BYTES, dtype=torch.uint8)
    n_cells, nbytes, n_edges = ctypes.c_int64(0), ctypes.c_size_t(0), ctypes.c_int64(0)
    lp = 1 if (loop or not one_set) else 0                # two point sets go in as loop = 1: nothing is excluded
    ptr_dst_c = None if one_set else ptr_dst_h.data_ptr()
    _lib.check(lib.gpde_knn_csr_batched_plan(box.data_ptr(), ptr_h.data_ptr(), ptr_dst_c, n_graphs, dim, k, lp, cell, table_h.data_ptr(),
                                             ctypes.byref(n_cells), ctypes.byref(nbytes), ctypes.byref(n_edges)),
               "gpde_knn_csr_batched_plan")
    assert int(n_edges.value) == e
    table = _upload(table_h, dev)
    ws = ops._alloc_ws(int(nbytes.value), dev)
    rowptr = torch.empty(nd + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_knn_csr_batched(pos.data_ptr(), n, pos.data_ptr() if one_set else pd.data_ptr(), nd, dim, k, lp,
                                            ptr_h.data_ptr(), ptr_dst_c, n_graphs, table.data_ptr(), int(n_cells.value),
                                            rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(), ops._ptr(geom), e, ws.data_ptr(),
                                            ws.numel(), ops._stream_ptr(dev)), "gpde_knn_csr_batched")
    return rowptr, src, dst, geom, edge_ptr_d, ke_max


def knn_csr_batched(pos: torch.Tensor, ptr, k: int, *, pos_dst: Optional[torch.Tensor] = None, ptr_dst=None, loop: bool = False,
                    bounds=None, cell_size: Optional[float] = None, return_geometry: bool = False, **single_graph_only):
    """The kNN graphs of B independent point sets in ONE build (gpde_knn_csr_batched): PyG's `knn_graph(pos, k, batch=batch)` as
    the block-diagonal `ops.Csr`.  Graph b owns the points pos[ptr[b]:ptr[b + 1]] (`ptr` int64 [B + 1] as in
    `ops.radius_csr_batched`; see `ops.ptr_from_batch`; pass it as a host tensor).  Returns (Csr, edge_ptr):
      Csr        global node ids; rowptr / src / dst (and geom) are the per-graph `knn_csr` results concatenated with their
                 offsets, bit for bit - a point of another graph is never a neighbour, however the graphs overlap in space;
                 `perm` is the identity; k_eff[b] = min(k, n_b) (min(k, n_b - 1) on one point set without self loops) differs
                 from graph to graph, every row of graph b has k_eff[b] edges;
      edge_ptr   int64 [B + 1] (device) = rowptr[ptr_dst]: graph b occupies the CSR slots edge_ptr[b] .. edge_ptr[b + 1].  It is
                 host arithmetic on `ptr` (`batch_slots`): E is known before anything runs.
    `pos_dst` with `ptr_dst`: two point sets per graph - a rectangular Csr (`n_src_nodes` set).
    `bounds`: host data [B, 2, dim], lo then hi of every graph's box.  With it the call performs no host synchronisation of any
    kind; without it the per-graph boxes are reduced on the device and copied once, the call's only synchronisation.
    `cell_size`: every graph's cell edge (default: automatic per graph).  Boxes and cells change speed, never the result.
    `return_geometry=True` returns (Csr, edge_ptr, geom).  A periodic box has no batched form."""
    rowptr, src, dst, geom, edge_ptr, ke_max = _build_batched(pos, ptr, k, pos_dst, ptr_dst, loop, bounds, cell_size,
                                                              bool(return_geometry), single_graph_only)
    e = int(src.numel())
    csr = ops.Csr(int(rowptr.numel()) - 1, e, rowptr, src, dst, torch.arange(e, dtype=torch.int32, device=src.device),
                  _max_in_degree=ke_max if e else 0, n_src_nodes=None if pos_dst is None else int(pos.size(0)))
    return (csr, edge_ptr, geom) if return_geometry else (csr, edge_ptr)


def knn_graph_batched(pos: torch.Tensor, ptr, k: int, *, pos_dst: Optional[torch.Tensor] = None, ptr_dst=None, loop: bool = False,
                      bounds=None, cell_size: Optional[float] = None, **single_graph_only):
    """(edge_index int64 [2, E], edge_ptr int64 [B + 1]) of the same batch: every graph in source-major order, graph after graph,
    global node ids - what collating the per-sample `knn_graph` edge lists gives, as `ops.radius_graph_batched`."""
    _, src, dst, _, edge_ptr, _ = _build_batched(pos, ptr, k, pos_dst, ptr_dst, loop, bounds, cell_size, False, single_graph_only)
    order = torch.sort(src, stable=True).indices          # rows are destination-major: targets stay ascending per source
    return torch.stack([src[order].long(), dst[order].long()]), edge_ptr
