"""Float64 checker of the GCN operator (graph_pde_amd.GCNConv, ops.gcn_norm / gcn_forward_raw) and the graphs its tests run on.

It never calls the code under test.  The coefficients are PyG's `gcn_norm` with `add_remaining_self_loops`, written out with
numpy: every node gets one self loop of weight 1 (`improved`: 2) unless it has self-loop edges, in which case the weight of the
one with the LARGEST edge id is taken; the degree is the target-side sum (in-edges of i + the self weight); self-loop edges get
coefficient 0.  The forward and the gradients are torch float64 (autograd)."""
import numpy as np
import torch


def coefficients(edge_index, n, edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    """(coef float64 [E] in the edge order of `edge_index`, self_coef float64 [N]) as numpy arrays."""
    ei = edge_index.detach().cpu().numpy()
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    w = np.ones(src.size) if edge_weight is None else edge_weight.detach().cpu().numpy().astype(np.float64)
    if not normalize:
        return w, np.zeros(n)
    if not add_self_loops:
        deg = np.zeros(n)
        np.add.at(deg, dst, w)
        dinv = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
        return dinv[src] * w * dinv[dst], np.zeros(n)
    loop = src == dst
    selfw = np.full(n, 2.0 if improved else 1.0)
    for e in np.nonzero(loop)[0]:            # ascending edge id: the last one wins
        selfw[src[e]] = w[e]
    deg = selfw.copy()
    np.add.at(deg, dst[~loop], w[~loop])
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    return np.where(loop, 0.0, dinv[src] * w * dinv[dst]), dinv * dinv * selfw


def forward(x, edge_index, weight, bias=None, edge_weight=None, improved=False, add_self_loops=True, normalize=True, relu=False):
    """out float64 [N, out] (torch, differentiable in x / weight / bias when they are float64 leaves); weight None: no multiply."""
    n = x.size(0)
    coef, selfc = coefficients(edge_index, n, edge_weight, improved, add_self_loops, normalize)
    ei = edge_index.detach().cpu()
    xd = x.double()
    msg = xd.index_select(0, ei[0]) * torch.from_numpy(coef).view(-1, 1)
    agg = torch.zeros(n, xd.size(1), dtype=torch.float64).index_add(0, ei[1], msg) + torch.from_numpy(selfc).view(-1, 1) * xd
    out = agg if weight is None else agg @ weight.double()
    if bias is not None:
        out = out + bias.double()
    return out.clamp_min(0) if relu else out


def gradients(x, edge_index, weight, bias, grad_out, **kw):
    """(out, grad_x, grad_weight, grad_bias or None) in float64 by autograd."""
    xd = x.detach().double().cpu().requires_grad_(True)
    wd = weight.detach().double().cpu().requires_grad_(True)
    bd = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    out = forward(xd, edge_index, wd, bd, **kw)
    out.backward(grad_out.detach().double().cpu())
    return out.detach(), xd.grad, wd.grad, None if bd is None else bd.grad


def chain32(x, edge_index, weight, bias, grad_out=None, **kw):
    """The same chain in float32 torch ops on the host (the precision yardstick `e32`): (out, gx, gw, gb)."""
    n = x.size(0)
    coef, selfc = coefficients(edge_index, n, **kw)
    ei = edge_index.detach().cpu()
    xf = x.detach().float().cpu().requires_grad_(True)
    wf = weight.detach().float().cpu().requires_grad_(True)
    bf = None if bias is None else bias.detach().float().cpu().requires_grad_(True)
    msg = xf.index_select(0, ei[0]) * torch.from_numpy(coef).float().view(-1, 1)
    agg = torch.zeros(n, xf.size(1)).index_add(0, ei[1], msg) + torch.from_numpy(selfc).float().view(-1, 1) * xf
    out = agg @ wf + (0 if bf is None else bf)
    if grad_out is None:
        return out.detach(), None, None, None
    out.backward(grad_out.detach().float().cpu())
    return out.detach(), xf.grad, wf.grad, None if bf is None else bf.grad


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def row_excess(a, ref):
    """max over rows of |err_row| / max(|ref_row|, rms row norm): the row rule of tests/test_gpu_width_tilings.py."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    rn = ref.norm(dim=1)
    rms = float(rn.pow(2).mean().sqrt())
    return float(((a - ref).norm(dim=1) / rn.clamp_min(max(rms, 1e-300))).max())


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def _shuffled(src, dst, g):
    order = torch.randperm(len(src), generator=g)
    return torch.stack([torch.tensor(src, dtype=torch.int64)[order], torch.tensor(dst, dtype=torch.int64)[order]])


def ladder(n=300, seed=1):
    """Node i has i % 70 in-edges from random OTHER nodes: rows of length 0 .. 69, n no multiple of a tile; shuffled edge order."""
    g = torch.Generator().manual_seed(seed)
    src, dst = [], []
    for i in range(n):
        k = i % 70
        src += ((i + 1 + torch.randint(0, n - 1, (k,), generator=g)) % n).tolist()
        dst += [i] * k
    return _shuffled(src, dst, g), n


def hub(n=2000, long=8192, seed=2):
    """Node 3 RECEIVES `long` edges, node 5 SENDS `long` edges (a long row of the reversed graph); about 4 in-edges elsewhere."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (4 * n,), generator=g).tolist() + torch.randint(0, n, (long,), generator=g).tolist() + [5] * long
    dst = [i for i in range(n) for _ in range(4)] + [3] * long + torch.randint(0, n, (long,), generator=g).tolist()
    return _shuffled(src, dst, g), n


def selfloops(n=300, seed=3):
    """The ladder on nodes < 290 plus a self-loop edge on every third of them (some twice), duplicate edges, and ten nodes
    (290 ..) with neither in- nor out-edges."""
    ei, _ = ladder(n, seed)
    keep = (ei[0] < 290) & (ei[1] < 290)
    ei = ei[:, keep]
    loops = torch.arange(0, 290, 3)
    twice = torch.arange(0, 290, 12)
    ei = torch.cat([ei, torch.stack([loops, loops]), ei[:, :60], torch.stack([twice, twice])], dim=1)
    g = torch.Generator().manual_seed(seed + 100)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous(), n


def directed(n=150, seed=4):
    """Edges j -> i only with j < i: no edge has its reverse, A^T != A."""
    g = torch.Generator().manual_seed(seed)
    src, dst = [], []
    for i in range(1, n):
        k = min(i, 3)
        src += torch.randint(0, i, (k,), generator=g).tolist()
        dst += [i] * k
    return _shuffled(src, dst, g), n


def grid(nx=5, ny=7):
    """4-neighbour grid, both directions, built [E, 2] and handed out as its TRANSPOSED view: a strided [2, E] edge_index."""
    pairs = []
    for a in range(nx):
        for b in range(ny):
            i = a * ny + b
            if b + 1 < ny:
                pairs += [(i, i + 1), (i + 1, i)]
            if a + 1 < nx:
                pairs += [(i, i + ny), (i + ny, i)]
    t = torch.tensor(pairs, dtype=torch.int64)
    ei = t.t()
    assert not ei.is_contiguous()
    return ei, nx * ny


def weights_for(edge_index, seed=7):
    """Edge weights in [0.1, 1.1]."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(edge_index.size(1), generator=g) + 0.1
