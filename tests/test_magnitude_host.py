"""Host tier of the magnitude-class tests (tests/helpers/magnitude_classes.py; GPU tier: tests/test_gpu_magnitude_classes.py).

1. The construction: no edge joins two classes, the classes interleave in CSR order, 128-slot groups span three or more
   destinations, every class has a heavy node and nodes without in-edges, duplicates and self-loops are there.
2. The bars are reachable without any scaling trick: a plain float32 autograd composite of the operator stays within the GPU
   tier's per-class bars (1e-5 forward, 2e-5 gradients, against float64) on the exact inputs the GPU tests use - every input
   set, the grad_out of the 2^-24 class on its own, and the rotated operands of the shared-module applications."""
import pytest
import torch

from oracle.nnconv_oracle import nnconv_grads, rel_l2
from tests.helpers import magnitude_classes as mc


@pytest.mark.parametrize("name,seed", [(n, s) for n in mc.SETS for s in mc.SEEDS])
def test_construction(name, seed):
    c = mc.case(name, seed)
    src, dst = c.ei[0], c.ei[1]
    assert bool((src % mc.C == dst % mc.C).all())                               # no edge joins two classes
    assert torch.equal(c.cls_node, torch.arange(c.n) % mc.C) and torch.equal(c.cls_edge, dst % mc.C)
    deg = torch.bincount(dst, minlength=c.n)
    order = torch.sort(dst, stable=True).values
    assert not torch.equal(order, dst)                                           # a shuffled edge order
    # the classes interleave in CSR order: every 128-slot group holds edges of at least three classes (all four in most)
    groups = [int(torch.unique(order[i:i + 128] % mc.C).numel()) for i in range(0, c.e - 127, 128)]
    heavy_groups = sum(1 for i in range(0, c.e - 127, 128) if torch.unique(order[i:i + 128]).numel() == 1)
    assert sum(1 for k in groups if k >= 3) >= len(groups) - heavy_groups - 2 * mc.C, (groups, heavy_groups)
    assert mc.max_destinations_per_group(order) >= 3
    for k in range(mc.C):
        dk = deg[c.cls_node == k]
        assert int((dk == 0).sum()) >= 2                                         # nodes without in-edges
        mine = c.cls_edge == k
        assert int((src[mine] == dst[mine]).sum()) >= 5                          # self-loops
        pairs = src[mine] * c.n + dst[mine]
        assert int(torch.bincount(pairs).max()) >= 5                             # duplicate edges
        if mc.SETS[name]["shape"] == "low":
            assert int(dk.max()) <= 64 and c.e <= 4 * c.n and c.e >= 4096        # the per-edge forward path's shape
        else:
            assert int(dk.max()) > 256                                           # a heavy node
            body = dk[(dk > 0) & (dk <= 256)]
            assert float(((body >= 8) & (body <= 64)).float().mean()) >= 0.9
    if mc.SETS[name]["shape"] != "low":
        assert c.e >= 4 * c.n                                                    # rows >= 4 nn: gpde_edge_bwd3_kernel
    # the operands carry the class factors, the zero class exact zeros
    z = c.cls_node == mc.ZERO_CLASS
    assert torch.count_nonzero(c.x[z]) == 0 and torch.count_nonzero(c.gout[z]) == 0
    assert torch.count_nonzero(c.ea[c.cls_edge == mc.ZERO_CLASS]) == 0
    for k in mc.live_classes(mc.X_F):
        rms = lambda t: float(t.double().pow(2).mean().sqrt())
        assert 0.8 * mc.X_F[k] <= rms(c.x[c.cls_node == k]) <= 1.25 * mc.X_F[k]
        assert 0.8 * mc.GRAD_OUT_F[k] <= rms(c.gout[c.cls_node == k]) <= 1.25 * mc.GRAD_OUT_F[k]
        attr = c.ea[c.cls_edge == k] if c.table is None else c.table[c.cls_node == k]      # (the table's columns carry the factors)
        assert 0.8 * mc.ATTR_F[k] <= rms(attr) <= 1.25 * mc.ATTR_F[k]


def _check_composite(c, aggr, x, gout, fx, fg, ref_out, ref, what):
    """The float32 composite against float64, per class where a class is a set of rows, globally for the summed gradients."""
    got = mc.composite(c, aggr, x, gout)
    errs = {}
    if ref_out is not None:
        errs.update({f"out[{k}]": v for k, v in mc.per_class_errors(got[0], ref_out, c.cls_node, mc.live_classes(fx)).items()})
        assert all(v <= mc.TOL_FWD for v in errs.values()), (what, errs)
    errs.update({f"dx[{k}]": v for k, v in mc.per_class_errors(got[1], ref[0], c.cls_node, mc.live_classes(fg)).items()})
    errs.update({f"dattr[{k}]": v for k, v in mc.per_class_errors(got[6], ref[5], c.cls_edge, mc.live_classes(fx, fg)).items()})
    for l in range(3):
        errs[f"dW{l + 1}"], errs[f"db{l + 1}"] = rel_l2(got[2][l], ref[1][l]), rel_l2(got[3][l], ref[2][l])
    errs["droot"], errs["dbias"] = rel_l2(got[4], ref[3]), rel_l2(got[5], ref[4])
    bad = {k: v for k, v in errs.items() if not v <= mc.TOL_BWD}
    assert not bad, (what, bad)
    # what the GPU tier asserts as exact zeros is exactly zero in plain arithmetic too
    assert mc.nonzero_rows(got[1], c.cls_node, mc.zero_classes(fg)) == 0
    assert mc.nonzero_rows(got[6], c.cls_edge, [k for k in range(mc.C) if fx[k] == 0 or fg[k] == 0]) == 0
    return errs


@pytest.mark.parametrize("name,seed,aggr", mc.INPUT_SETS)
def test_float32_composite_is_within_the_bars_per_class(name, seed, aggr):
    c = mc.case(name, seed)
    errs = _check_composite(c, aggr, c.x, c.gout, mc.X_F, mc.GRAD_OUT_F, mc.reference_out(name, seed, aggr),
                            mc.reference_grads(name, seed, aggr), (name, seed, aggr))
    print(name, seed, aggr, {k: f"{v:.2e}" for k, v in errs.items()})
    solo_f = tuple(f if k == mc.SMALL_CLASS else 0.0 for k, f in enumerate(mc.GRAD_OUT_F))
    _check_composite(c, aggr, c.x, c.solo_gout(), mc.X_F, solo_f, None, mc.reference_grads(name, seed, aggr, solo=True),
                     (name, seed, aggr, "solo"))


@pytest.mark.parametrize("seed", mc.SEEDS)
def test_float32_composite_on_the_rotated_applications(seed):
    """The applications of a shared module (the hidden form's accumulation, light + deferred): x and grad_out with their class
    factors rotated - each application's inputs are an input set of their own."""
    c = mc.case("small", seed)
    aggr = mc.aggr_of(seed)
    for l, (kx, kg) in enumerate(mc.APPLICATIONS[1:], start=1):
        x, gout = c.operand("x", kx, l), c.operand("grad_out", kg, l)
        ref = nnconv_grads(x, c.ei, c.ea, c.W, c.B, c.root, c.bias, aggr, gout, chunk_edges=mc.ORACLE_CHUNK, need_attr=True)
        _check_composite(c, aggr, x, gout, mc.rotate(mc.X_F, kx), mc.rotate(mc.GRAD_OUT_F, kg), None, ref, (seed, l))
        fg = mc.rotate(mc.GRAD_OUT_F, kg)              # ... and with only the application's 2^-24 class live
        solo = mc.solo_of(gout, c.cls_node, fg)
        ref = nnconv_grads(x, c.ei, c.ea, c.W, c.B, c.root, c.bias, aggr, solo, chunk_edges=mc.ORACLE_CHUNK, need_attr=True)
        _check_composite(c, aggr, x, solo, mc.rotate(mc.X_F, kx), tuple(f if f == 2.0 ** -24 else 0.0 for f in fg), None, ref,
                         (seed, l, "solo"))
