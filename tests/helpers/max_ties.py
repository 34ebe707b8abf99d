"""Test infrastructure: edges whose message ties for the maximum of its destination ('max' aggregation).

Where two in-edges of a node carry messages within rounding of each other in some output channel - exact duplicates of an
edge always do - the device and the float64 oracle may legitimately pick different winners, and the gradient of the
segment max goes to a different edge (or is split between them).  No arithmetic is wrong there, so instead of loosening
the gradient tolerance the 'max' property tests REMOVE those edges from the test graph: for every (destination, channel)
the first edge at the maximum is kept and every other edge within `tau` x (the channel's largest |message| at that
destination) of it is dropped.  The maxima themselves are unchanged by the removal.

Companion of tests/helpers/kinks.py; messages as in the reference's NNConv_old.message (nn_conv.py:273-275)."""
from typing import Optional, Sequence

import torch

from oracle.nnconv_oracle import densenet_forward


def edges_off_the_max_ties(x: torch.Tensor, edge_index: torch.Tensor, edge_attr: torch.Tensor,
                           weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
                           tau: float = 1e-5, chunk: int = 4096) -> torch.Tensor:
    """bool [E]: True for the edges to keep.  float64 on the host, in edge chunks."""
    e, n = edge_index.shape[1], x.shape[0]
    if e == 0:
        return torch.ones(0, dtype=torch.bool)
    src, dst = edge_index[0], edge_index[1]
    xd = x.double()
    Ws = [w.double() for w in weights]
    Bs = [None if b is None else b.double() for b in biases]
    m = torch.empty(e, xd.shape[1], dtype=torch.float64)
    for lo in range(0, e, chunk):
        sl = slice(lo, lo + chunk)
        w = densenet_forward(edge_attr[sl].double(), Ws, Bs).view(-1, xd.shape[1], Ws[-1].shape[0] // xd.shape[1])
        m[sl] = torch.matmul(xd[src[sl]].unsqueeze(1), w).squeeze(1)
    idx = dst.unsqueeze(1).expand_as(m)
    mx = torch.full((n, m.shape[1]), float("-inf"), dtype=torch.float64).scatter_reduce(0, idx, m, "amax")
    scale = torch.zeros(n, m.shape[1], dtype=torch.float64).scatter_reduce(0, idx, m.abs(), "amax")
    near = (mx[dst] - m) <= tau * scale[dst]
    eid = torch.arange(e).unsqueeze(1).expand_as(m)
    first = torch.full((n, m.shape[1]), e, dtype=torch.int64).scatter_reduce(
        0, idx, torch.where(near, eid, torch.full_like(eid, e)), "amin")
    return ~(near & (eid != first[dst])).any(dim=1)
