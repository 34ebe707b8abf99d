#!/usr/bin/env python3
"""Generate tests/golden/diag_w8.npz and diag_gauss_w64.npz by running the REFERENCE's own diagonal-kernel classes:
`NNConv` (graph-neural-operator/nn_conv.py:8-96) and `NNConv_Gaussian` (nn_conv.py:99-194).

Run where the reference lies next to the repository (tests/golden/make_golden.py says where):   python tests/golden/make_golden_diag.py

The reference's file is imported from where it lies, on the CPU, through the import stubs of make_golden.py (whose only behaviour
is `MessagePassing.propagate`, restated from PyG ~1.3).  The fixtures hold DATA only: inputs, parameters, `out_f32` (the reference's
arithmetic) and `out_f64` (the same module after `.double()`, the adjudicator).  Graph: 16 nodes, 60 edges in no sorted order, with
duplicate edges, self-loops and two nodes without in-edges.

The Gaussian class multiplies by 1 / sqrt(|pseudo[:, 1] * pseudo[:, 2]|) and divides by nn(ones(1))^2: its attributes keep
pseudo[:, 1] * pseudo[:, 2] in [0.25, 2.25] and its `nn` (one Linear) emits widths in [0.6, 1.4].  The reference hard-codes 64
channels there (nn_conv.py:180), so that case is the w = 64 one.  Its `ones(1)` is float32 whatever the module's dtype, so the
Linear is wrapped in a module that casts its input to its own dtype - otherwise `.double()` could not run."""
import os

import numpy as np
import torch

import make_golden as mg

HERE = os.path.dirname(os.path.abspath(__file__))


class Widths(torch.nn.Module):
    """nn of the Gaussian case: Linear(1, w) on an input cast to the layer's dtype."""

    def __init__(self, w):
        super().__init__()
        self.lin = torch.nn.Linear(1, w)

    def forward(self, one):
        return self.lin(one.to(self.lin.weight.dtype))


def graph(gen):
    n, e = 16, 60
    src = torch.randint(0, n, (e,), generator=gen)
    dst = torch.randint(0, n - 2, (e,), generator=gen)      # nodes 14, 15: no in-edge
    src[:4], dst[:4] = 3, 7                                 # duplicate edges 3 -> 7
    src[4:8] = dst[4:8]                                     # self-loops
    return torch.stack([src, dst]), n


def run(conv, x, ei, ea):
    with torch.no_grad():
        y32 = conv(x, ei, ea)
        conv64 = conv.double()
        y64 = conv64(x.double(), ei, ea.double())
        conv.float()
    return y32, y64


def save(name, conv, params, x, ei, ea, y32, y64):
    d = {"x": x.numpy(), "edge_index": ei.numpy(), "edge_attr": ea.numpy(), "aggr": np.array(conv.aggr),
         "root": conv.root.detach().float().numpy(), "bias": conv.bias.detach().float().numpy(),
         "out_f32": y32.numpy(), "out_f64": y64.numpy()}
    d.update({k: v.detach().float().numpy() for k, v in params.items()})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **d)
    print(f"{name}: N={x.shape[0]} E={ei.shape[1]} |y|={float(y32.norm()):.4f} "
          f"rel(f32,f64)={float((y32.double() - y64).norm() / y64.norm()):.2e} -> {os.path.getsize(path)} B")


def main():
    mg._install_stubs()
    ref = mg._load("nn_conv", os.path.join(mg.REF, "nn_conv.py"))

    # w = 8: NNConv with a two-layer kernel network, aggr='mean'
    torch.manual_seed(40)
    gen = torch.Generator().manual_seed(41)
    ei, n = graph(gen)
    nn = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, 8))
    conv = ref.NNConv(8, 8, nn, aggr="mean")
    x, ea = torch.randn(n, 8, generator=gen), torch.randn(ei.shape[1], 3, generator=gen)
    save("diag_w8", conv, {"W0": nn[0].weight, "b0": nn[0].bias, "W1": nn[2].weight, "b1": nn[2].bias}, x, ei, ea, *run(conv, x, ei, ea))

    # w = 64: NNConv_Gaussian, aggr='add'
    torch.manual_seed(42)
    gen = torch.Generator().manual_seed(43)
    ei, n = graph(gen)
    nn = Widths(64)
    conv = ref.NNConv_Gaussian(64, 64, nn, aggr="add")
    with torch.no_grad():                                   # (after the constructor: reset_parameters re-draws the Linear)
        nn.lin.weight.copy_(0.6 + 0.8 * torch.rand(64, 1, generator=gen))
        nn.lin.bias.zero_()
    x = torch.randn(n, 64, generator=gen)
    ea = torch.cat([2 * torch.rand(ei.shape[1], 1, generator=gen) - 1, 0.5 + torch.rand(ei.shape[1], 2, generator=gen)], dim=1)
    save("diag_gauss_w64", conv, {"W0": nn.lin.weight, "b0": nn.lin.bias}, x, ei, ea, *run(conv, x, ei, ea))


if __name__ == "__main__":
    main()
