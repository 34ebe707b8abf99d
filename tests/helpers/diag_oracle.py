"""The diagonal-kernel operator restated in torch (graph-neural-operator/nn_conv.py:83-92 and :174-190), evaluated in the dtype
of its inputs - the tests feed float64 -, differentiable in whatever requires grad; the degree-ladder graph built from the
kernel's own plan (ops.diag_plan).  The row-by-row comparison is any_tilings.worst_row."""
import os

import numpy as np
import torch

from tests.helpers.any_tilings import worst_row  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")


def diag_reference(x_src, x_dst, ei, k, root, bias, aggr, n_dst=None, residual=None, relu=False):
    """out_i = aggr_{e: j -> i} x_src[j] * k_e + x_dst[i] . root + bias (+ residual, ReLU); `k` [E, w] in the order of `ei`
    (ei[0] indexes x_src, ei[1] the destinations).  `x_dst` None: no root term.  `diag_embed(k).view(-1, w, w)` followed by
    `matmul(x_j.unsqueeze(1), .)` (nn_conv.py:84-85) IS the elementwise product: every other term of the row sum is an exact 0."""
    n = int(n_dst if n_dst is not None else (x_dst.shape[0] if x_dst is not None else x_src.shape[0]))
    m = x_src[ei[0]] * k
    w = m.shape[1]
    if aggr == "max":
        out = torch.full((n, w), float("-inf"), dtype=m.dtype, device=m.device)
        out = out.scatter_reduce(0, ei[1].unsqueeze(1).expand_as(m), m, "amax", include_self=True)
        out = torch.where(torch.isinf(out), torch.zeros_like(out), out)
    else:
        out = torch.zeros(n, w, dtype=m.dtype, device=m.device).index_add(0, ei[1], m)
        if aggr == "mean":
            out = out / torch.bincount(ei[1], minlength=n).clamp(min=1).to(m.dtype).unsqueeze(1)
    if root is not None and x_dst is not None:
        out = out + x_dst @ root
    if bias is not None:
        out = out + bias
    if residual is not None:
        out = out + residual
    return torch.relu(out) if relu else out


def gaussian_kernel(pseudo, widths):
    """nn_conv.py:175-180: a (x) 1 * exp(-pseudo[:, 0]^2 / widths^2), a = 1 / sqrt(|pseudo[:, 1] * pseudo[:, 2]|); `widths` =
    nn(ones(1)), [w]."""
    amplitude = (pseudo[:, 1] * pseudo[:, 2]).abs().sqrt().reciprocal().unsqueeze(1)
    return amplitude * torch.exp(-pseudo[:, 0:1].square() / widths.reshape(1, -1).square())


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: (str(z[k]) if k == "aggr" else torch.from_numpy(z[k])) for k in z.files}


def golden_kernel(g, dtype):
    """The per-edge kernel of a golden case from its stored parameters, in `dtype`."""
    t = lambda name: g[name].to(dtype)
    if "W1" in g:           # diag_w8: Linear, ReLU, Linear
        return torch.relu(t("edge_attr") @ t("W0").t() + t("b0")) @ t("W1").t() + t("b1")
    return gaussian_kernel(t("edge_attr"), torch.ones(1, dtype=dtype) @ t("W0").t() + t("b0"))      # diag_gauss_w64: Linear(1, w)


def ladder_degrees(plan):
    """In-degrees 0, 1 and one either side of every boundary of the kernel's loops: the edge slots of a step, a pass, a chain."""
    es, ps, ch = plan["ES"], plan["pass_edges"], plan["chain_edges"]
    return sorted({d for b in (es, ps, 2 * ps, ch, 2 * ch) for d in (b - 1, b, b + 1)} | {0, 1, ch + ps + es + 1})


def ladder_graph(plan, gen, n_trailing=3, n_src=None):
    """(edge_index int64 [2, E] shuffled, n_dst, {in-degree: destination}).  One destination per ladder degree in a shuffled node
    order; self-loops, duplicate edges into the longest row, a quarter of the edges leaving node 1, `n_trailing` isolated nodes at
    the end.  `n_src`: the sources are drawn from that many nodes (a graph between two node sets), else from the destinations."""
    degs = ladder_degrees(plan)
    n = len(degs) + n_trailing
    order = torch.randperm(len(degs), generator=gen).tolist()
    dst = torch.tensor([order[k] for k, d in enumerate(degs) for _ in range(d)], dtype=torch.int64)
    e = dst.numel()
    ns = n - n_trailing if n_src is None else n_src
    src = torch.randint(0, ns, (e,), generator=gen)
    src[torch.rand(e, generator=gen) < 0.25] = 1
    if n_src is None:
        kk = max(1, e // 16)
        src[:kk] = dst[:kk]                                 # self-loops
    big = order[max(range(len(degs)), key=lambda i: degs[i])]
    sel = (dst == big).nonzero().flatten()[: max(2, e // 32)]
    src[sel] = 2 % ns                                       # duplicates of one edge into the longest row
    perm = torch.randperm(e, generator=gen)
    return torch.stack([src[perm], dst[perm]]), n, {d: order[k] for k, d in enumerate(degs)}
