"""GPU tier: property-based random graphs (SURVEY.md §4 tier ii; VERDICT r4 missing 5).

`hypothesis` draws the structure - node and edge counts, duplicate edges, self-loops, isolated nodes and nodes without
in-edges, unsorted edge order, a strided `edge_index` view, `aggr`, the `root_weight` / `bias` flags of
`NNConv_old.__init__` (/root/reference/graph-neural-operator/nn_conv.py:234-259), a kernel MLP of 2-5 Linear layers with
widths 16..300 (none of them tile multiples, as `DenseNet` allows: utilities.py:201-221) - and the module's forward and all
gradients (`loss.backward()`, UAI1_full_resolution.py:266) are compared with the float64 oracle.  The examples are derived
with `derandomize=True` (no example database; the drawn set still depends on the process it runs in - see FWD_FACTOR).  Edges on the ReLU kink
are removed (tests/helpers/kinks.py) so the gradient tolerance is the plain one."""
import os

import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import graph_pde_amd as gp
from graph_pde_amd import ops
from oracle.nnconv_oracle import nnconv_forward, nnconv_grads, rel_l2
from tests.helpers.kinks import edges_off_the_kink

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_BWD = 1e-6, 2e-5
# The forward bar is max(TOL_FWD, FWD_FACTOR x e32), e32 = the distance of the fp32 ORACLE from float64 on the same inputs: a
# well-conditioned case (fp32 oracle at ~1e-7) is held to 1e-6; a sum that cancels (no root weight and bias, a mean of hundreds of
# messages of random sign) to 4 x the reference's own fp32 rounding - the two-term f16 operands carry 2^-22 of their block's
# largest magnitude where an fp32 product carries 2^-24 of its own.  Whenever the fp32 oracle itself is within E32_WELL of float64,
# the result must also be within NORTH_STAR (1e-5, BASELINE.json) outright.
FWD_FACTOR = 4
NORTH_STAR, E32_WELL = 1e-5, 2.5e-6
# Only a case whose fp32 oracle itself misses E32_WELL - a sum of thousands of cancelling terms - may instead pass on the error
# against the sum of the MAGNITUDES of the terms the operator adds up: KAPPA_FACTOR x 2^-22 per unit of it (_magnitude_norm).
KAPPA_FACTOR = 8


@st.composite
def cases(draw):
    n = draw(st.integers(2, 400))
    e = draw(st.integers(0, 20000))
    n_hidden = draw(st.integers(1, 4))
    widths = [draw(st.integers(16, 300)) for _ in range(n_hidden)]
    return {
        "n": n, "e": e, "k0": draw(st.integers(1, 8)), "widths": widths,
        "aggr": draw(st.sampled_from(["mean", "add"])), "root": draw(st.booleans()), "bias": draw(st.booleans()),
        "dup": draw(st.integers(0, 64)), "loops": draw(st.integers(0, 64)),
        "n_dst": draw(st.integers(1, n)),                       # destinations are drawn from the first n_dst nodes: the rest have no in-edges
        "layout": draw(st.sampled_from(["contiguous", "every_other_column", "transposed_storage"])),
        "seed": draw(st.integers(0, 2 ** 31 - 1)),
    }


def _magnitude_norm(x, ei, ea, W, B, root, bias, aggr):
    """|| M || with M[i][o] = sum_c sum_k (sum_e |x_j[c]| h_e[k]) |W3[(c,o)][k]| + sum_c (sum_e |x_j[c]|) |b3[(c,o)]| (+ |x_i| . |root| + |bias|),
    'mean'-scaled, in float64: the sum of the MAGNITUDES of the terms the re-associated operator adds up - what a
    rounding error of relative size eps per term can amount to.  || M || / || out || is the condition number of the sum."""
    n = x.shape[0]
    h = ea.double()
    for l in range(len(W) - 1):
        h = torch.relu(h @ W[l].double().t() + B[l].double())
    k2 = h.shape[1]
    xa = x.double().abs()
    A = torch.zeros(n, 64, k2, dtype=torch.float64)
    S = torch.zeros(n, 64, dtype=torch.float64)
    for a0 in range(0, ei.shape[1], 2048):
        sl = slice(a0, a0 + 2048)
        xs = xa[ei[0, sl]]
        A.index_add_(0, ei[1, sl], xs.unsqueeze(2) * h[sl].abs().unsqueeze(1))
        S.index_add_(0, ei[1, sl], xs)
    W3 = W[-1].double().abs().view(64, 64, k2)                                   # [(c, o)][k]
    M = torch.einsum("ick,cok->io", A, W3) + torch.einsum("ic,co->io", S, B[-1].double().abs().view(64, 64))
    if aggr == "mean":
        deg = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.shape[1], dtype=torch.float64))
        M = M / deg.clamp_min(1).unsqueeze(1)
    if root is not None:
        M = M + xa @ root.double().abs()
    if bias is not None:
        M = M + bias.double().abs()
    return float(M.norm())


@settings(max_examples=int(os.environ.get("GPDE_HYP_EXAMPLES", "30")), deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
@given(cases())
def test_random_graphs_forward_and_gradients_vs_float64(c):
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(c["seed"])
    # mean in-degree of the destinations at most 8192: 4.6 x the 1,793 of the reference's radius graphs (241^2 grid, r = 0.1)
    n, e = c["n"], min(c["e"], 8192 * c["n_dst"])
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, c["n_dst"], (e,), generator=g)
    dup, loops = min(c["dup"], e // 2), min(c["loops"], e // 2)
    if dup:
        src[:dup], dst[:dup] = src[0].item(), dst[0].item()                       # `dup` copies of one edge
    if loops:
        src[e - loops:] = dst[e - loops:]                                          # self-loops
    dims = [c["k0"]] + c["widths"] + [4096]
    mlp = torch.nn.Sequential(*sum([[torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.ReLU()] for i in range(len(dims) - 1)], [])[:-1])
    conv = gp.NNConv_old(64, 64, mlp, aggr=c["aggr"], root_weight=c["root"], bias=c["bias"])
    with torch.no_grad():
        # weights from the example's seed, not the global RNG - AFTER the module is built: NNConv_old.__init__ resets `nn`
        # (nn_conv.py:258, reset(self.nn)).  Until the end of round 6 this loop ran before the constructor, the weights were the
        # global generator's, and an example's conditioning - and with it whether it met the forward bar - depended on every test
        # that had run before it: the "fails once, passes on replay" reports of that round.
        for p_ in conv.nn.parameters():
            p_.copy_(torch.empty_like(p_).uniform_(-1, 1, generator=g) / (p_.shape[-1] ** 0.5))
        for p_ in (conv.root, conv.bias):
            if p_ is not None:
                p_.copy_(torch.empty_like(p_).uniform_(-0.125, 0.125, generator=g))
    ea = torch.randn(e, c["k0"], generator=g)
    x, gout = torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)
    lin = ops.mlp_linears(conv.nn)
    W, B = [l.weight.detach().clone() for l in lin], [l.bias.detach().clone() for l in lin]
    keep = edges_off_the_kink(ea, W, B) if e else torch.ones(0, dtype=torch.bool)
    src, dst, ea = src[keep], dst[keep], ea[keep].contiguous()
    e = int(src.numel())
    ei = torch.stack([src, dst])
    root = None if conv.root is None else conv.root.detach().clone()
    bias = None if conv.bias is None else conv.bias.detach().clone()
    ref = nnconv_forward(x, ei, ea, W, B, root, bias, aggr=c["aggr"], dtype=torch.float64)
    e32 = rel_l2(nnconv_forward(x, ei, ea, W, B, root, bias, aggr=c["aggr"], dtype=torch.float32), ref)
    rx, rW, rb, rroot, rbias = nnconv_grads(x, ei, ea, W, B, root, bias, c["aggr"], gout, chunk_edges=4096)

    conv = conv.to(d)
    if c["layout"] == "every_other_column":                                         # a strided view
        big = torch.zeros(2, 2 * e, dtype=torch.int64, device=d)
        big[:, ::2] = ei.to(d)
        ei_d = big[:, ::2]
    elif c["layout"] == "transposed_storage":
        ei_d = ei.t().contiguous().to(d).t()
    else:
        ei_d = ei.to(d)
    xin = x.to(d).requires_grad_(True)
    out = conv(xin, ei_d, ea.to(d))
    (out * gout.to(d)).sum().backward()
    torch.cuda.synchronize()
    err = rel_l2(out.detach().cpu(), ref)
    if os.environ.get("GPDE_HYP_CALIBRATE"):
        kappa = _magnitude_norm(x, ei, ea, W, B, root, bias, c["aggr"]) / max(float(ref.norm()), 1e-300)
        kappa = max(kappa, 1e-300)
        with open(os.environ["GPDE_HYP_CALIBRATE"], "a") as fh:
            fh.write(f"{err / (2.0 ** -22 * kappa):.4f} {err / max(e32, 1e-300):.3f} {kappa:.3e} {err:.3e} {e32:.3e} n={c['n']} e={e} widths={c['widths']} {c['aggr']} root={c['root']} bias={c['bias']}\n")
        return
    if e32 <= E32_WELL:
        assert err <= NORTH_STAR, ("forward", c, err, "fp32 oracle vs float64:", e32)
    if not err <= max(TOL_FWD, FWD_FACTOR * e32):
        # the second bar, for sums the first one cannot judge (thousands of cancelling terms into one node), and only for them
        kappa = _magnitude_norm(x, ei, ea, W, B, root, bias, c["aggr"]) / max(float(ref.norm()), 1e-300)
        assert e32 > E32_WELL and err <= KAPPA_FACTOR * 2.0 ** -22 * kappa, \
            ("forward", c, err, "fp32 oracle vs float64:", e32, "kappa:", kappa)
    lin = ops.mlp_linears(conv.nn)
    errs = {"dx": rel_l2(xin.grad.cpu(), rx)}
    for l, layer in enumerate(lin):
        errs[f"dW{l + 1}"] = rel_l2(layer.weight.grad.cpu(), rW[l])
        errs[f"db{l + 1}"] = rel_l2(layer.bias.grad.cpu(), rb[l])
    if conv.root is not None:
        errs["droot"] = rel_l2(conv.root.grad.cpu(), rroot)
    if conv.bias is not None:
        errs["dbias"] = rel_l2(conv.bias.grad.cpu(), rbias)
    bad = {k: v for k, v in errs.items() if not v <= TOL_BWD}
    assert not bad, (c, bad)
