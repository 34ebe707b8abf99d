#!/usr/bin/env python3
"""Generate the RECTANGULAR golden vectors tests/golden/nnconv_rect_*.npz by running the REFERENCE's own classes.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_widths.py

The float64 oracle (oracle/nnconv_oracle.py) takes in_channels / out_channels from the shapes, but the fixtures of
make_golden.py are all 64 -> 64 - where a transposed `view(-1, out, in)` would pass unnoticed.  These cases pin it, and the
native any-width operator (csrc/gpde_weconv_any.hip), at in != out: the reference's `NNConv_old` + `DenseNet`
(graph-neural-operator/nn_conv.py:197-286, utilities.py:201-227; `weight = self.nn(pseudo).view(-1, in_channels,
out_channels)`, nn_conv.py:274) through the import stubs of make_golden.py.

  nnconv_rect_24x40_mean   24 -> 40, aggr='mean', root and bias, 3-Linear kernel network
  nnconv_rect_40x24_add    40 -> 24, aggr='add', no root, no bias, 2-Linear kernel network
  nnconv_rect_1x8_mean      1 ->  8, aggr='mean', x given 1-D (nn_conv.py:269)

Each case: <name>.npz in the layout of make_golden.py (inputs, parameters, out_f32, out_f64) and <name>_grad.npz (gout and the
float64 gradients of sum(out * gout) by autograd through the reference's module).  The graphs carry isolated nodes, duplicate
edges and self-loops, edges in no particular order.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg      # noqa: E402  (the stub installer, the module loader, _run and _save)


def _graph(n, e, k0, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - 5, (e,), generator=g)        # the last 5 nodes have no in-edge
    dst[dst == 2] = 3                                       # node 2 neither
    src[:6], dst[:6] = 1, 4                                 # 6 duplicate edges 1 -> 4
    src[6:12] = dst[6:12]                                   # self-loops
    return torch.stack([src, dst]), torch.randn(e, k0, generator=g), g


def _save_grads(name, conv, x, ei, ea, cout, seed):
    gout = torch.randn(x.shape[0], cout, generator=torch.Generator().manual_seed(seed))
    conv64 = conv.double()
    conv64.zero_grad()
    x64 = x.double().requires_grad_(True)
    out = conv64(x64, ei, ea.double())
    (out * gout.double()).sum().backward()
    layers = [l for l in conv64.nn.layers if isinstance(l, torch.nn.Linear)]
    d = {"gout": gout.numpy(), "gx": x64.grad.numpy()}
    for i, l in enumerate(layers):
        d[f"gW{i}"] = l.weight.grad.numpy()
        d[f"gb{i}"] = l.bias.grad.numpy()
    if conv64.root is not None:
        d["groot"] = conv64.root.grad.numpy()
    if conv64.bias is not None:
        d["gbias"] = conv64.bias.grad.numpy()
    conv.float()
    path = os.path.join(HERE, name + "_grad.npz")
    np.savez_compressed(path, **d)
    print(f"{name}_grad: |gx|={float(x64.grad.norm()):.4f} -> {os.path.getsize(path)} B")


def main():
    mg._install_stubs()
    ref_util = mg._load("utilities", os.path.join(mg.REF, "utilities.py"))
    ref_nn_conv = mg._load("nn_conv", os.path.join(mg.REF, "nn_conv.py"))

    torch.manual_seed(41)
    conv = ref_nn_conv.NNConv_old(24, 40, ref_util.DenseNet([6, 16, 16, 24 * 40], torch.nn.ReLU), aggr="mean")
    ei, ea, g = _graph(60, 300, 6, 141)
    x = torch.randn(60, 24, generator=g)
    mg._save("nnconv_rect_24x40_mean", conv, x, ei, ea, *mg._run(conv, x, ei, ea))
    _save_grads("nnconv_rect_24x40_mean", conv, x, ei, ea, 40, 241)

    torch.manual_seed(42)
    conv = ref_nn_conv.NNConv_old(40, 24, ref_util.DenseNet([5, 12, 40 * 24], torch.nn.ReLU), aggr="add",
                                  root_weight=False, bias=False)
    ei, ea, g = _graph(50, 260, 5, 142)
    x = torch.randn(50, 40, generator=g)
    mg._save("nnconv_rect_40x24_add", conv, x, ei, ea, *mg._run(conv, x, ei, ea))
    _save_grads("nnconv_rect_40x24_add", conv, x, ei, ea, 24, 242)

    torch.manual_seed(43)
    conv = ref_nn_conv.NNConv_old(1, 8, ref_util.DenseNet([3, 10, 8], torch.nn.ReLU), aggr="mean")
    ei, ea, g = _graph(40, 200, 3, 143)
    x = torch.randn(40, generator=g)                        # 1-D: promoted to [N, 1] by the module (nn_conv.py:269)
    mg._save("nnconv_rect_1x8_mean", conv, x, ei, ea, *mg._run(conv, x, ei, ea))
    _save_grads("nnconv_rect_1x8_mean", conv, x, ei, ea, 8, 243)


if __name__ == "__main__":
    main()
