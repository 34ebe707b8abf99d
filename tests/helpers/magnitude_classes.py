"""Test infrastructure: graphs whose outputs each depend on ONE magnitude class.

Every split-f16 path of the library is exact only because each operand carries a power-of-two scale taken from a maximum
(per destination node, per edge row, per row and step, per tile, per call) and each result is un-scaled by the matching
reciprocal.  On randn inputs all those maxima share one binary exponent, so a lane un-scaled with ANOTHER row's scale returns
the bits of a correct kernel.  The graphs built here make such a mix-up visible:

  * C = 4 disjoint components ("classes"); node i belongs to class i % C, so neighbouring CSR rows - and with them the
    128-slot groups of the per-edge kernels - always mix classes; every edge joins two nodes of one class;
  * in-degrees 8 .. ~60 (groups straddle 2+ destinations, rows >= 4 nodes: the split-f16 per-edge backward kernel), one heavy
    node of > 256 in-edges per class, nodes without in-edges, duplicate edges, self-loops, a shuffled edge order; the "low"
    shape (in-degrees 0 .. 6, no heavy node) is the per-edge forward path's;
  * class c multiplies its randn rows of x / grad_out / edge_attr by its own power of two (X_F / GRAD_OUT_F / ATTR_F below);
    class ZERO_CLASS by exactly 0.

The components being disjoint, the rows of `out` and `grad_x` of class c's nodes and the rows of `grad_edge_attr` and
`grad_hidden` of its edges depend on class c's operands only: a relative L2 restricted to one class is meaningful, a class
whose grad_out (or x) is 0 must come back as exact zeros, and scaling one class's grad_out by 2^k must scale that class's
rows by 2^k bit for bit wherever every scale on the path is per row or per node.

Spreads.  grad_out: 2^-24 (a mean loss over ~10^5 nodes) next to 1 and 2^12 - every dZ / dU scale is per node or per row.
x: 2^-6 .. 2^6 and edge_attr 2^6 .. 2^-6 (against the grain of x): the split-f16 aggregation has ONE scale per call for x
and one for h; a hi + lo f16 pair scaled into [2^13, 2^14) keeps its 22 bits for elements down to ~2^-15 of the maximum, and
these spreads stay inside that.

The kernel MLP follows the reference's Linear / ReLU chain (oracle.nnconv_oracle.densenet_forward); edges on a ReLU kink are
removed (tests/helpers/kinks.py).  References are float64 (oracle.nnconv_oracle), computed once per input set and shared."""
import dataclasses
import functools
from typing import List, Optional

import torch

from oracle.nnconv_oracle import densenet_forward, nnconv_forward, nnconv_grads, rel_l2
from tests.helpers.kinks import edges_off_the_kink

C = 4
ZERO_CLASS = 3
SMALL_CLASS = 0                                   # the class of the 2^-24 grad_out
GRAD_OUT_F = (2.0 ** -24, 1.0, 2.0 ** 12, 0.0)
X_F = (2.0 ** -6, 1.0, 2.0 ** 6, 0.0)
ATTR_F = (2.0 ** 6, 1.0, 2.0 ** -6, 0.0)
TOL_FWD, TOL_BWD = 1e-5, 2e-5                     # BASELINE.json north_star; TOL of tests/test_gpu_bwd_regime_properties.py
ORACLE_CHUNK = 4096

# name -> nodes, edges before the kink removal, graph shape, smallest first hidden width the paths of the set are built for
SETS = {
    "small": dict(n=320, e=6000, shape="mixed", k1_min=128),       # eb3 + zagg32, the hidden form, light + deferred, v3 forward
    "table": dict(n=320, e=6000, shape="mixed", k1_min=256),       # attributes gathered from a node table (NodeAttr)
    "big": dict(n=400, e=10500, shape="mixed", k1_min=128),        # one chunk of >= 8192 rows
    "z16": dict(n=1200, e=37500, shape="mixed", k1_min=256),       # >= 32768 edges: split-f16 Z re-aggregation, the v6 forward
    "low": dict(n=1600, e=4800, shape="low", k1_min=128),          # mean in-degree 3: the per-edge forward path
}
HEAVY = 260        # + 7 per class: > 256, and below the smallest set's node count (ops.per_edge_association)
SEEDS = (0, 1)
# (x rotation, grad_out rotation) of the applications of a shared module: application 0 is the set's own x / grad_out; in the
# later ones the zero-x class and the zero-grad_out class differ, and the large x meets the small grad_out
APPLICATIONS = ((0, 0), (1, 2), (2, 1))


def aggr_of(seed: int) -> str:
    """The aggregation of the cases that run one: both get their turn over the seeds."""
    return "mean" if seed % 2 == 0 else "add"


# every (set, seed, aggr) the GPU tier runs; the host tier shows a float32 composite within the bars on each of them
INPUT_SETS = [("small", s, a) for s in SEEDS for a in ("add", "mean")] + \
             [(name, s, aggr_of(s)) for name in ("table", "big", "z16", "low") for s in SEEDS]


def solo_of(gout: torch.Tensor, cls_node: torch.Tensor, factors) -> torch.Tensor:
    """`gout` with every class zeroed but the one whose factor in `factors` is the 2^-24 one."""
    return gout * (cls_node == factors.index(GRAD_OUT_F[SMALL_CLASS])).unsqueeze(1)


def rotate(factors, k):
    """The class factors moved on by k classes: class c gets the factor of class (c + k) % C."""
    return tuple(factors[(c + k) % C] for c in range(C))


def class_rows(cls: torch.Tensor, width: int, factors, g: torch.Generator) -> torch.Tensor:
    """randn [len(cls), width], row r multiplied by factors[cls[r]] (powers of two: exact; the zero class gives +-0)."""
    return torch.randn(cls.numel(), width, generator=g) * torch.tensor(factors, dtype=torch.float32)[cls].unsqueeze(1)


def class_graph(n: int, e: int, shape: str, g: torch.Generator):
    """(src, dst) int64 of a graph of C disjoint components, node i in class i % C (see the module docstring)."""
    assert n % C == 0
    m = n // C
    if shape == "low":
        deg = torch.randint(0, 7, (n,), generator=g)
    else:
        empty = torch.randperm(m, generator=g)[:max(2, m // 16)]
        body = n - C - C * empty.numel()
        hi = max(9, 2 * (e - C * HEAVY) // body - 8)
        deg = torch.randint(8, hi + 1, (n,), generator=g)
        for c in range(C):
            deg[C * ((empty + c) % m) + c] = 0                     # nodes without in-edges, other rows in every class
            deg[C * ((m // 2 + 5 * c) % m) + c] = HEAVY + 7 * c    # one heavy node per class
    dst = torch.repeat_interleave(torch.arange(n), deg)
    cls = dst % C
    src = C * torch.randint(0, m, (dst.numel(),), generator=g) + cls
    for c in range(C):
        idx = (cls == c).nonzero().flatten()
        src[idx[1:6]], dst[idx[1:6]] = src[idx[0]].item(), dst[idx[0]].item()      # five copies of one edge
        src[idx[-6:]] = dst[idx[-6:]]                                               # self-loops
    perm = torch.randperm(dst.numel(), generator=g)                                 # unsorted edge order
    return src[perm], dst[perm]


@dataclasses.dataclass
class Case:
    name: str
    seed: int
    n: int
    dims: List[int]
    ei: torch.Tensor            # int64 [2, E]
    ea: torch.Tensor            # [E, k0]
    x: torch.Tensor
    gout: torch.Tensor
    W: List[torch.Tensor]
    B: List[torch.Tensor]
    root: torch.Tensor
    bias: torch.Tensor
    cls_node: torch.Tensor      # [n]
    cls_edge: torch.Tensor      # [E] class of each edge, in the order of `ei`
    table: Optional[torch.Tensor] = None
    sel: Optional[list] = None

    @property
    def e(self) -> int:
        return int(self.ei.shape[1])

    def operand(self, what: str, k: int, tag: int) -> torch.Tensor:
        """Fresh randn rows of x / grad_out with the class factors rotated by k (the applications of a shared module)."""
        g = torch.Generator().manual_seed(1000003 * self.seed + 7919 * tag + (17 if what == "x" else 29))
        return class_rows(self.cls_node, 64, rotate(X_F if what == "x" else GRAD_OUT_F, k), g)

    def solo_gout(self) -> torch.Tensor:
        """grad_out with every class but the 2^-24 one zeroed: the training-sized gradient on its own."""
        return self.gout * (self.cls_node == SMALL_CLASS).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def case(name: str, seed: int) -> Case:
    s = SETS[name]
    g = torch.Generator().manual_seed(7 + 131 * seed + 17 * sorted(SETS).index(name))
    n = s["n"]
    k0 = 6 if seed % 2 == 0 else 5
    k1 = 256 if (seed % 2 == 0 or s["k1_min"] == 256) else 128
    dims = [k0, k1, 256, 4096]
    src, dst = class_graph(n, s["e"], s["shape"], g)
    cls_node = torch.arange(n) % C
    W = [torch.empty(dims[i + 1], dims[i]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(3)]
    B = [torch.empty(dims[i + 1]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(3)]
    root = torch.empty(64, 64).uniform_(-0.125, 0.125, generator=g)
    bias = torch.empty(64).uniform_(-0.125, 0.125, generator=g)
    table = sel = None
    if name == "table":                 # the table's rows carry the class factors; an edge reads rows of its own class only
        table = class_rows(cls_node, 3, ATTR_F, g)
        sel = [(int(torch.randint(0, 2, (1,), generator=g)), int(torch.randint(0, 3, (1,), generator=g))) for _ in range(k0)]
        ea = torch.stack([table[(dst if ep else src), col] for ep, col in sel], dim=1)
    else:
        ea = class_rows(dst % C, k0, ATTR_F, g)
    x = class_rows(cls_node, 64, X_F, g)
    gout = class_rows(cls_node, 64, GRAD_OUT_F, g)
    keep = edges_off_the_kink(ea, W, B)
    src, dst, ea = src[keep], dst[keep], ea[keep].contiguous()
    return Case(name, seed, n, dims, torch.stack([src, dst]), ea, x, gout, W, B, root, bias, cls_node, dst % C, table, sel)


# ---- references ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_out(name: str, seed: int, aggr: str) -> torch.Tensor:
    c = case(name, seed)
    return nnconv_forward(c.x, c.ei, c.ea, c.W, c.B, c.root, c.bias, aggr=aggr, dtype=torch.float64, chunk_edges=ORACLE_CHUNK)


@functools.lru_cache(maxsize=None)
def reference_grads(name: str, seed: int, aggr: str, solo: bool = False):
    """float64 (grad_x, [grad_W], [grad_b], grad_root, grad_bias, grad_edge_attr); `solo`: only the 2^-24 class has grad_out."""
    c = case(name, seed)
    return nnconv_grads(c.x, c.ei, c.ea, c.W, c.B, c.root, c.bias, aggr, c.solo_gout() if solo else c.gout,
                        chunk_edges=ORACLE_CHUNK, need_attr=True)


def grad_hidden_f64(c: Case, aggr: str, x: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
    """float64 dL/dU [E, k2] of the last hidden layer's pre-activations (rows in the order of c.ei), loss = sum(out * gout):
    autograd through the oracle's last Linear and message, masked by the float64 activations' [H > 0]."""
    src, dst = c.ei[0], c.ei[1]
    Ws, Bs = [w.double() for w in c.W], [b.double() for b in c.B]
    gT = gout.double()
    if aggr == "mean":
        gT = gT / torch.bincount(dst, minlength=c.n).clamp(min=1).double().unsqueeze(1)
    xs = x.double()
    out = torch.empty(c.e, c.dims[-2], dtype=torch.float64)
    for lo in range(0, c.e, ORACLE_CHUNK):
        sl = slice(lo, lo + ORACLE_CHUNK)
        h = torch.relu(densenet_forward(c.ea[sl].double(), Ws[:-1], Bs[:-1])).requires_grad_(True)
        w = densenet_forward(h, Ws[-1:], Bs[-1:]).view(-1, 64, 64)
        m = torch.matmul(xs[src[sl]].unsqueeze(1), w).squeeze(1)
        (m * gT[dst[sl]]).sum().backward()
        out[sl] = h.grad * (h.detach() > 0)
    return out


def composite(c: Case, aggr: str, x: torch.Tensor, gout: torch.Tensor, dtype=torch.float32, chunk: int = 8192):
    """The operator as a plain autograd composite of stock torch ops in `dtype` (no scales, no re-association): the
    reference's chain - kernel MLP, view + matmul, scatter over the destinations, update().  Returns (out, grad_x, [grad_W],
    [grad_b], grad_root, grad_bias, grad_edge_attr) for loss = sum(out * gout); the edges run in chunks (16 KiB per edge)."""
    src, dst = c.ei[0], c.ei[1]
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)          # (a leaf of its own: the case's tensors are left alone)
    xs, ea, Ws, Bs, r, bb = leaf(x), leaf(c.ea), [leaf(w) for w in c.W], [leaf(b) for b in c.B], leaf(c.root), leaf(c.bias)
    gT = gout.to(dtype)
    cnt = torch.bincount(dst, minlength=c.n).clamp(min=1).to(dtype).unsqueeze(1)
    if aggr == "mean":
        gT = gT / cnt
    out = torch.zeros(c.n, 64, dtype=dtype)
    for lo in range(0, c.e, chunk):
        sl = slice(lo, lo + chunk)
        m = torch.matmul(xs[src[sl]].unsqueeze(1), densenet_forward(ea[sl], Ws, Bs).view(-1, 64, 64)).squeeze(1)
        out.index_add_(0, dst[sl], m.detach())
        (m * gT[dst[sl]]).sum().backward()
    if aggr == "mean":
        out = out / cnt
    node = xs @ r + bb
    (node * gout.to(dtype)).sum().backward()
    return (out + node.detach(), xs.grad, [w.grad for w in Ws], [b.grad for b in Bs], r.grad, bb.grad, ea.grad)


# ---- per-class measures -------------------------------------------------------------------------------------------------------

def per_class_errors(got: torch.Tensor, ref: torch.Tensor, cls: torch.Tensor, classes) -> dict:
    """{class: rel_l2 over the rows of that class}."""
    got = got.detach().cpu()
    return {c: rel_l2(got[cls == c], ref[cls == c]) for c in classes}


def nonzero_rows(t: torch.Tensor, cls: torch.Tensor, classes) -> int:
    """Number of non-zero entries (-0.0 counts as zero) in the rows of `classes`."""
    t = t.detach().cpu()
    mask = torch.zeros_like(cls, dtype=torch.bool)
    for c in classes:
        mask |= cls == c
    return int(torch.count_nonzero(t[mask]))


def zero_classes(factors) -> list:
    return [c for c in range(C) if factors[c] == 0.0]


def live_classes(*factor_sets) -> list:
    """Classes none of whose given operands is zero."""
    return [c for c in range(C) if all(f[c] != 0.0 for f in factor_sets)]


def max_destinations_per_group(dst_csr: torch.Tensor) -> int:
    """Largest number of destinations a 128-slot group of the CSR order spans."""
    return max(int(torch.unique(dst_csr[i:i + 128]).numel()) for i in range(0, dst_csr.numel(), 128))
