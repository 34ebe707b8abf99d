"""Sampled graphs: the reference's `gaussian_connectivity` built natively as the operator's CSR.

Next to `ball_connectivity` every mesh generator of the reference offers `gaussian_connectivity(sigma)`
(graph-neural-operator/utilities.py:257-263, 372-378; multipole-graph-neural-operator/utilities.py:283-289, 419-425): each
ordered pair is kept independently with probability exp(-d^2 / sigma^2).  `gaussian_csr` builds that graph on the device with
the cell-list kernels of gpde_gaussian_csr_count / _fill (include/gpde.h states the contract):

    edge j -> i   iff   u(seed, i, j) < exp(-(d2 / (sigma * sigma)))                   (float64)
    u  = ((key >> 10) + 0.5) * 2^-53,   key = ops.edge_hash_keys(src = j, dst = i, seed)
    d2 = the float64 whose bits ops.edge_sqdist_keys returns for the edge

so the graph is a pure function of positions, sigma and seed.  It lies inside the radius graph of
`gaussian_support_radius(sigma)` = sigma sqrt(54 ln 2): u >= 2^-54, and no pair beyond that radius has a larger probability.
The candidate pairs inside the support are never formed - at sigma = 0.1 on the 241^2 lattice they are 2.13e9, 0.7 % under
what an int32 CSR holds (and 121 GiB of temporaries by the composite route), while the sampled graph has 9.4e7 edges and is
built in 1 GiB (DESIGN.md §6e "The sampled arm").

A hard cap on top composes: `ops.select_in_edges(gaussian_csr(...), k, key)`.  `NNConvGaussian` takes the edge distance as
`pseudo[:, 0]`: that is `geom[:, dim]` of `gaussian_csr(..., return_geometry=True)`.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib, ops

__all__ = ["gaussian_csr", "gaussian_graph", "gaussian_in_degrees", "gaussian_support_radius"]

_SUPPORT = math.sqrt(54.0 * math.log(2.0))       # exp(-d^2 / sigma^2) = 2^-54 at d = _SUPPORT sigma


def _positive(v, name: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"{name} must be a positive finite number (got {v!r})")
    v = float(v)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"{name} = {v} must be positive and finite")
    return v


def gaussian_support_radius(sigma: float) -> float:
    """sigma sqrt(54 ln 2) ~ 6.118 sigma: beyond it exp(-d^2 / sigma^2) < 2^-54, the smallest draw - no pair is ever kept."""
    return _positive(sigma, "sigma") * _SUPPORT


def _dim_of(t, name: str) -> int:
    if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name} must be a tensor [n, dim] (or [n]: one dimension) (got {got})")
    return 1 if t.dim() == 1 else int(t.size(1))


def _host_args(pos, sigma, seed, pos_dst, period, origin, cutoff):
    """Every refusal that needs no device (ValueError): (sigma, cutoff or 0, seed, period list or None, origin list, dim)."""
    sigma = _positive(sigma, "sigma")
    if not (sigma * sigma > 0.0 and math.isfinite(sigma * sigma)):
        raise ValueError(f"sigma = {sigma}: sigma^2 must be positive and finite in float64")
    cut = 0.0 if cutoff is None else _positive(cutoff, "cutoff")
    seed = ops._cap_seed(seed)
    dim = _dim_of(pos, "pos")
    if not 1 <= dim <= 3:
        raise ValueError(f"positions of dimension {dim}: the sampled graphs are built in 1..3 dimensions")
    if pos_dst is not None and _dim_of(pos_dst, "pos_dst") != dim:
        raise ValueError("pos and pos_dst must have the same dimension")
    per = None
    org = [0.0] * dim
    if period is not None:
        per, org = ops._key_box(period, origin, dim)
        reach = sigma * _SUPPORT if cutoff is None else min(sigma * _SUPPORT, cut)
        for k, L in enumerate(per):
            if L > 0.0 and not 2.0 * reach < L:
                raise ValueError(f"2 min(r_support, cutoff) = {2.0 * reach} >= period[{k}] = {L}: a pair would have more than one image "
                                 f"in reach of sigma = {sigma} (r_support = {sigma * _SUPPORT}); pass cutoff= below period / 2")
        if not any(per):
            per = None
    return sigma, cut, seed, per, org, dim


def _build(pos, sigma, seed, pos_dst, period, origin, cutoff, fill: bool, geometry: bool):
    """gpde_gaussian_csr_count (+ _fill) on the caller's current stream: (deg,) or (rowptr, src, dst, geom | None, largest
    in-degree)."""
    sigma, cut, seed, per, org, _ = _host_args(pos, sigma, seed, pos_dst, period, origin, cutoff)
    pos, pd = ops._positions(pos, pos_dst)
    n, nd, dim = int(pos.size(0)), int(pd.size(0)), int(pos.size(1))
    dev = pos.device
    if n == 0 or nd == 0:
        if not fill:
            return (torch.zeros(nd, dtype=torch.int32, device=dev),)
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return (torch.zeros(nd + 1, dtype=torch.int32, device=dev), z, z.clone(),
                torch.zeros(0, dim + 1, dtype=torch.float32, device=dev) if geometry else None, 0)
    lib = _lib.lib()
    lo, hi = ops._host_bounds(pos, pd)
    org_c = (ctypes.c_double * dim)(*org)
    per_c = None if per is None else (ctypes.c_double * dim)(*per)
    nbytes = int(lib.gpde_gaussian_csr_workspace_bytes(n, dim, sigma, cut, lo, hi, org_c, per_c))
    if nbytes == 0:
        _lib.check(-1, "gpde_gaussian_csr_workspace_bytes")
    ws = ops._alloc_ws(nbytes, dev)
    deg = torch.empty(nd, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_gaussian_csr_count(pos.data_ptr(), n, pd.data_ptr(), nd, dim, sigma, cut, seed, lo, hi, org_c, per_c,
                                               deg.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream_ptr(dev)),
                   "gpde_gaussian_csr_count")
    if not fill:
        return (deg,)
    rowptr64 = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=rowptr64[1:])
    e, max_deg = (int(v) for v in torch.stack([rowptr64[-1], deg.max().long()]).cpu())      # the one synchronisation
    if e >= (1 << 31) - 64:
        raise NotImplementedError(f"{e} edges exceed the int32 CSR")
    rowptr = rowptr64.to(torch.int32)
    src = torch.empty(e, dtype=torch.int32, device=dev)
    dst = torch.empty(e, dtype=torch.int32, device=dev)
    geom = torch.empty(e, dim + 1, dtype=torch.float32, device=dev) if geometry else None
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_gaussian_csr_fill(pos.data_ptr(), n, pd.data_ptr(), nd, dim, sigma, cut, seed, lo, hi, org_c, per_c,
                                              rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(), ops._ptr(geom), e, max_deg,
                                              ws.data_ptr(), ws.numel(), ops._stream_ptr(dev)), "gpde_gaussian_csr_fill")
    return rowptr, src, dst, geom, max_deg


def gaussian_csr(pos: torch.Tensor, sigma: float, seed: int = 0, *, pos_dst: Optional[torch.Tensor] = None, period=None,
                 origin=None, cutoff: Optional[float] = None, return_geometry: bool = False):
    """The Gaussian-connectivity graph of `pos` [n, dim] (dim 1..3) as the `ops.Csr` the operator consumes: the edge j -> i is
    kept iff u(seed, i, j) < exp(-d^2 / sigma^2) (the module docstring states u and d^2).  Rows are in ascending source order
    (rows longer than 4,096 edges: the builder's deterministic cell order), `perm` is the identity, self pairs are always
    kept, the two directions of a pair are independent draws.  One synchronisation: the edge count.

    `pos_dst`: a second point set - edges (j in pos -> i in pos_dst) with level-local ids; the result is the rectangular Csr
    (`n_src_nodes` set), as from `ops.radius_csr(pos, r, pos_dst=)`.
    `period` / `origin`: as in `ops.radius_csr` (a scalar or one entry per axis; 0 / None = open axis) - d^2 is the
    minimum-image distance.  A periodic axis needs 2 min(r_support, cutoff) < period, else ValueError.
    `cutoff=r`: additionally drop every pair with d^2 > r^2 - a TRUNCATED Gaussian, a different graph from the untruncated one.
    `return_geometry=True` returns (Csr, geom): geom float32 [E, dim + 1] by CSR slot, the displacement pos[src] -
    image(pos_dst[dst]) and its norm - the rows `ops.radius_csr(..., return_geometry=True)` gives these edges.
    There is one arithmetic (exact float64); the int32 edge limit is refused like the other builders'."""
    rowptr, src, dst, geom, max_deg = _build(pos, sigma, seed, pos_dst, period, origin, cutoff, True, bool(return_geometry))
    e = int(src.numel())
    csr = ops.Csr(int(rowptr.numel()) - 1, e, rowptr, src, dst, torch.arange(e, dtype=torch.int32, device=src.device), _max_in_degree=max_deg,
                  n_src_nodes=None if pos_dst is None else int(pos.size(0)))
    return (csr, geom) if return_geometry else csr


def gaussian_graph(pos: torch.Tensor, sigma: float, seed: int = 0, *, pos_dst: Optional[torch.Tensor] = None, period=None,
                   origin=None, cutoff: Optional[float] = None) -> torch.Tensor:
    """edge_index int64 [2, E] of the same graph in the reference's order (sorted by source, then target), as `ops.radius_graph`
    gives the radius graph: `gaussian_csr(...).edge_index` stably sorted by source."""
    _, src, dst, _, _ = _build(pos, sigma, seed, pos_dst, period, origin, cutoff, True, False)
    order = torch.sort(src, stable=True).indices          # rows are destination-major: targets stay ascending per source
    return torch.stack([src[order].long(), dst[order].long()])


def gaussian_in_degrees(pos: torch.Tensor, sigma: float, seed: int = 0, *, pos_dst: Optional[torch.Tensor] = None, period=None,
                        origin=None, cutoff: Optional[float] = None) -> torch.Tensor:
    """int32 [n_dst]: the in-degree of every destination of that graph - the COUNT pass alone, no edge is written."""
    return _build(pos, sigma, seed, pos_dst, period, origin, cutoff, False, False)[0]
