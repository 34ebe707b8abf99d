"""Test infrastructure shared by the GPU tests of the native backward: the node-aligned chunk walk bwd_impl makes for a plan
(csrc/gpde_bwd.hip), the smallest workspace whose plan holds a wanted number of edges per chunk, and a call run under the
backward's branch trace (_lib.bwd_trace_begin / bwd_trace_end)."""
import torch

from graph_pde_amd import _lib, ops


def walk(rowptr, ec, nc, h_nodes=0):
    """The node-aligned chunks bwd_impl cuts for `ec` edges / `nc` nodes per chunk (a chunk never straddles h_nodes)."""
    n, out, na = len(rowptr) - 1, [], 0
    while na < n and rowptr[-1] > 0:
        lo, hi = na + 1, min(na + nc, n)
        if na < h_nodes:
            hi = min(hi, h_nodes)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if rowptr[mid] - rowptr[na] <= ec:
                lo = mid
            else:
                hi = mid - 1
        out.append((na, lo))
        na = lo
    return out


def ws_for(n, e, dims, want_ec):
    """Smallest workspace (bisection over ops.bwd_plan) whose plan holds >= want_ec edges per chunk."""
    lo, hi = 1 << 20, int(_lib.lib().gpde_nnconv_bwd_workspace_bytes_one_chunk(n, e, len(dims) - 1, _lib.dims_array(dims)))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            ok = ops.bwd_plan(n, e, dims, mid)["edges_per_chunk"] >= want_ec
        except _lib.GpdeError:
            ok = False
        if ok:
            hi = mid
        else:
            lo = mid
    return hi


def traced(fn):
    _lib.bwd_trace_begin()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        recs = _lib.bwd_trace_end()
    return out, recs
