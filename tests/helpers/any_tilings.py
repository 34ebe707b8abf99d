"""Test infrastructure for the any-width operator (csrc/gpde_weconv_any.hip): its lane-tiling classes, the degree-ladder graph
built from a tiling, the float64 statement of the operator given the per-edge weights, and the row-by-row comparison.

A tiling class is what decides which instructions of the kernels run, read from the library's own plan query
(ops.any_width_plan) and the widths:
    (V, LC, R > 1, ES > 1, B, column steps per lane, idle lanes, partly filled last column step, in_channels % R != 0)
`classes()` enumerates all 256 x 256 widths through the query; nothing here restates the plan."""
import functools
import math

import torch

from graph_pde_amd import ops

MAXW = ops.ANY_MAX_WIDTH
N_CLASSES = 128          # add / mean, V by out_channels % 4: counted once from the query; a change of the plan changes it


def tiling_class(cin, cout, plan):
    v, lc, r, es, b = plan["V"], plan["LC"], plan["R"], plan["ES"], plan["B"]
    ncv = cout // v                                   # column accesses of one row
    steps = -(-ncv // lc)                             # ... per lane: 1 (V = 4), 1 .. 4 (V = 1)
    return (v, lc, r > 1, es > 1, b, steps, plan["lanes"] < 64, ncv % lc != 0, cin % r != 0)


def class_name(k):
    v, lc, r, es, b, steps, idle, part, crem = k
    return f"V{v}-LC{lc}-R{'n' if r else '1'}-ES{'n' if es else '1'}-B{b}-s{steps}" + ("-idle" if idle else "") + \
        ("-part" if part else "") + ("-crem" if crem else "")


@functools.lru_cache(maxsize=None)
def classes(aggr="add", aligned=True):
    """{class: [(cin, cout), ...] ascending} over all widths 1 .. 256, from the plan query."""
    out = {}
    for cin in range(1, MAXW + 1):
        for cout in range(1, MAXW + 1):
            out.setdefault(tiling_class(cin, cout, ops.any_width_plan(cin, cout, aligned=aligned, aggr=aggr)), []).append((cin, cout))
    return out


def representatives(aggr="add"):
    """[(class name, class, cin, cout)]: the smallest (cin, cout) of each class, in class order."""
    return [(class_name(k), k, *v[0]) for k, v in sorted(classes(aggr).items())]


def max_representatives():
    """The smallest widths of each distinct (V, LC, ES) of the 'max' plan."""
    seen = {}
    for cin in range(1, MAXW + 1):
        for cout in range(1, MAXW + 1):
            p = ops.any_width_plan(cin, cout, aggr="max")
            seen.setdefault((p["V"], p["LC"], p["ES"]), (cin, cout))
    return [(f"V{k[0]}-LC{k[1]}-ES{k[2]}", k, *v) for k, v in sorted(seen.items())]


def ladder_degrees(plan, eb_cap=None):
    """In-degrees around every boundary of the batch loop: a pass of the forward is EB = B * ES in-edges, ES of them per step."""
    es, eb = plan["ES"], plan["B"] * plan["ES"]
    if eb_cap is not None:
        eb = min(eb, eb_cap)
    return sorted({d for d in (0, 1, es - 1, es, es + 1, eb - 1, eb, eb + 1, 2 * eb + 3, 4 * eb + es + 1) if d >= 0})


def ladder_graph(plan, gen, copies=2, n_trailing=3):
    """(edge_index int64 [2, E] in no sorted order, n_nodes, {in-degree: [destination nodes]}).

    `copies` ladders of destinations in a shuffled node order (~ 20 B ES edges at two copies).  Node 0 has no out-edge and no
    in-edge, a quarter of the edges leave node 1 (which has no in-edge), the other sources are drawn from nodes 1 .. ; duplicate
    edges into the longest row, self-loops, `n_trailing` isolated nodes at the end."""
    degs = ladder_degrees(plan) * copies
    n_dst = len(degs)
    n = n_dst + 2 + n_trailing                          # + nodes 0, 1 shifted in below; trailing nodes touch no edge
    order = (torch.randperm(n_dst, generator=gen) + 2).tolist()   # ladder destinations: nodes 2 .. n_dst + 1, shuffled
    dst = torch.tensor([order[k] for k, d in enumerate(degs) for _ in range(d)], dtype=torch.int64)
    e = dst.numel()
    src = torch.randint(1, n - n_trailing, (e,), generator=gen)
    src[torch.rand(e, generator=gen) < 0.25] = 1        # node 1: many out-edges; node 0: none
    k = max(1, e // 16)
    src[:k] = dst[:k]                                   # self-loops
    big = order[max(range(len(degs)), key=lambda i: degs[i])]
    sel = (dst == big).nonzero().flatten()[: max(2, e // 32)]
    src[sel] = 2 if big != 2 else 3                     # duplicates of one edge into the longest row
    perm = torch.randperm(e, generator=gen)
    by_deg = {}
    for kk, d in enumerate(degs):
        by_deg.setdefault(d, []).append(order[kk])
    return torch.stack([src[perm], dst[perm]]), n, by_deg


def reference64(x, ei, w, root, bias, aggr, residual=None, relu=False):
    """out = aggr_{e -> i} x_src(e) . W_e + x_i . root + bias (+ residual, ReLU) in float64 torch ops on the tensors' device;
    `w` [E, cin * cout] in the order of `ei`.  Differentiable in whatever requires grad."""
    n, cin = x.shape
    cout = w.shape[1] // cin
    m = torch.matmul(x[ei[0]].unsqueeze(1), w.view(-1, cin, cout)).squeeze(1)
    if aggr == "max":
        out = torch.full((n, cout), float("-inf"), dtype=x.dtype, device=x.device)
        out = out.scatter_reduce(0, ei[1].unsqueeze(1).expand_as(m), m, "amax", include_self=True)
        out = torch.where(torch.isinf(out), torch.zeros_like(out), out)
    else:
        out = torch.zeros(n, cout, dtype=x.dtype, device=x.device).index_add(0, ei[1], m)
        if aggr == "mean":
            out = out / torch.bincount(ei[1], minlength=n).clamp(min=1).to(x.dtype).unsqueeze(1)
    if root is not None:
        out = out + x @ root
    if bias is not None:
        out = out + bias
    if residual is not None:
        out = out + residual
    return torch.relu(out) if relu else out


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def worst_row(a, b):
    """max over rows of |a_row - b_row| / max(|b_row|, rms row norm of b): one wrong row of a long tensor shows, a row whose
    reference is (near) zero is measured against the typical row."""
    a, b = a.detach().double().reshape(b.shape[0], -1), b.detach().double().reshape(b.shape[0], -1)
    if b.numel() == 0:
        return 0.0
    rn = b.norm(dim=1)
    scale = torch.maximum(rn, rn.pow(2).mean().sqrt()).clamp_min(1e-300)
    return float(((a - b).norm(dim=1) / scale).max())


def draw_inputs(n, e, cin, cout, gen, device="cpu"):
    """x, W_e (edge order), root, bias, residual, grad_out: continuous random data, messages of unit scale."""
    r = lambda *s: torch.randn(*s, generator=gen)
    x, w = r(n, cin), r(e, cin * cout) / math.sqrt(cin)
    root, bias, res, g = r(cin, cout) / math.sqrt(cin), r(cout), r(n, cout), r(n, cout)
    return [t.to(device) for t in (x, w, root, bias, res, g)]
