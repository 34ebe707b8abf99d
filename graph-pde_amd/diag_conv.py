"""The DIAGONAL-kernel modules of the reference's operator file, on the native diagonal operator (csrc/gpde_diagconv.hip):

* `NNConvDiag`      -- graph-neural-operator/nn_conv.py:8-96, the class that file calls `NNConv`: `nn(pseudo)`
  emits `out_channels` values per edge, `diag_embed` makes them a diagonal matrix, the message is `x_j * nn(pseudo)`;
* `NNConvGaussian`  -- nn_conv.py:99-194 (`NNConv_Gaussian`): the same message with an analytic Gaussian kernel whose widths
  are `nn(ones(1))`.

    out_i = aggr_{e: j -> i} x_j (.) k_e  +  x_i . root + bias

Same constructor, parameter names (`root`, `bias`, `nn`), `reset_parameters` and `__repr__` as the reference.  The per-edge kernel
k [E, w] is evaluated by torch - it is the caller's network, w floats per edge where the full kernel is w^2 -; gather, message,
aggregation and `update()` are ONE native call.  (`graph_pde_amd.NNConv` stays `torch_geometric.nn.NNConv`, the full kernel.)
"""
from __future__ import annotations

import torch

from . import ops
from .autograd import DiagConvFunction
from .nn_conv import _ConvFront, _dev_of, _front_args, _glued, _materialized, _on_dev, _rows, _slot_rows


class NNConvDiag(_ConvFront):
    r"""x'_i = Theta x_i + aggr_{j in N(i)} x_j (.) h_Theta(e_ij), h_Theta emitting one value per channel and edge
    (nn_conv.py:8-96).  The source width must equal `out_channels` (`diag_embed(...).view(-1, in, out)`, nn_conv.py:84, needs it).

    `in_channels` may be a pair `(in_src, in_dst)` - `root` is then [in_dst, out] - and `forward` takes `x = (x_src, x_dst)` with
    `size=(n_src, n_dst)`, both flows, as `NNConv_old` takes them.  add / mean are differentiable natively (DiagConvFunction: dL/dk
    flows on into `nn`); aggr='max' runs natively without a gradient, through `MessagePassing.propagate` over the torch `message()`
    / `update()` below with a gradient on one node set, and is not built with a gradient on two.  `ops.NodeAttr` attributes are
    materialised (one node set only); an `ops.Csr` is accepted as `edge_index`.  `residual=` / `activation="relu"` are fused into the
    kernel's epilogue when no gradient is needed, torch ops otherwise.  CPU tensors and parameters are staged to the current HIP
    device and the result returns to the caller's device."""

    _nn_line = "nn_conv.py:84"
    _propagate_line = "nn_conv.py:81"

    def __init__(self, in_channels, out_channels, nn, aggr="add", root_weight=True, bias=True, **kwargs):
        if not isinstance(nn, torch.nn.Module):
            raise NotImplementedError(f"nn must be a torch.nn.Module that maps edge attributes [E, k] to [E, out_channels] values "
                                      f"(nn_conv.py:28-32, 84), got {type(nn).__name__}")
        in_channels, flow = _front_args(in_channels, aggr, kwargs, "nn_conv.py:33-35")
        in_src = in_channels[0] if isinstance(in_channels, tuple) else in_channels
        in_dst = in_channels[1] if isinstance(in_channels, tuple) else in_channels
        if in_src != out_channels:
            raise ValueError(f"the diagonal kernel needs in_channels == out_channels (diag_embed(nn(pseudo)).view(-1, in, out), "
                             f"nn_conv.py:84), got {in_src} -> {out_channels}")
        if not (ops.width_supported(in_src, out_channels) and ops.width_supported(in_dst, out_channels)):
            raise NotImplementedError(f"the MI355X diagonal operator is built for widths 1 .. {ops.ANY_MAX_WIDTH}, got "
                                      f"{in_channels}->{out_channels}")
        super().__init__(in_channels, out_channels, nn, aggr, root_weight, bias, flow)

    # ---- the per-edge kernel ----------------------------------------------------------------------------------------------
    def edge_kernel(self, pseudo):
        """k [E, out_channels]: the diagonal of the reference's per-edge matrix (nn_conv.py:84), by torch where `pseudo` lives."""
        return self.nn(pseudo)

    def _checked_kernel(self, pseudo, n_edges):
        k = self.edge_kernel(pseudo)
        w = int(self.out_channels)
        if not torch.is_tensor(k) or k.dim() != 2 or tuple(k.shape) != (n_edges, w):
            raise ValueError(f"the per-edge kernel must be [E, out_channels] = [{n_edges}, {w}] ({self._nn_line}), got "
                             f"{tuple(k.shape) if torch.is_tensor(k) else type(k).__name__}")
        return k

    # ---- forward ----------------------------------------------------------------------------------------------------------
    def forward(self, x, edge_index, edge_attr, *, size=None, residual=None, activation=None):      # nn_conv.py:77-81
        """The reference signature `forward(x, edge_index, edge_attr)`; `x` may be a pair `(x_src, x_dst)` with `size=(n_src,
        n_dst)`.  Keyword-only extras: `residual` [n_dst, out] added to the result and `activation="relu"`."""
        if activation not in (None, "relu"):
            raise ValueError(f"activation must be None or 'relu', got {activation!r}")
        relu = activation == "relu"
        rect = self._rect_call(x, size, residual)
        with ops.ver_scope():
            if rect is not None:
                if isinstance(edge_attr, ops.NodeAttr):
                    raise NotImplementedError("ops.NodeAttr attributes on a call between two node sets are not built: a node table addresses "
                                              "ONE node set - pass the edge_attr tensor")
                return self._propagate_two(*rect, edge_index, _rows(edge_attr), residual, relu)
            x = _rows(x[0] if isinstance(x, (tuple, list)) else x)
            slot_order = False
            if isinstance(edge_attr, ops.NodeAttr):
                if self._flipped():
                    raise NotImplementedError("ops.NodeAttr attributes with flow='target_to_source' are not built - pass the edge_attr tensor")
                # (from a CSR the rows come out in slot order already)
                slot_order = isinstance(edge_index, ops.Csr)
                edge_attr = _materialized(edge_attr, edge_index)
            return self._propagate_one(x, edge_index, _rows(edge_attr), residual, relu, slot_order)

    def _propagate_one(self, x, edge_index, pseudo, residual, relu, slot_order=False):
        w = int(self.out_channels)
        if x.dim() != 2 or x.size(1) != w:
            raise ValueError(f"x must be [N, {w}] (in_channels), got {tuple(x.shape)}")
        if x.dtype != torch.float32 or (residual is not None and residual.dtype != torch.float32):
            raise NotImplementedError(f"the diagonal operator: float32 only (x is {x.dtype})")
        if residual is not None and tuple(residual.shape) != tuple(x.shape):
            raise ValueError(f"residual must be [N, out_channels] = {tuple(x.shape)}, got {tuple(residual.shape)}")
        needs_grad = self._needs_grad(x, residual, pseudo)
        dev = _dev_of(x)
        if self.aggr == "max" and needs_grad:
            # (`_max_detour` over the torch `message()` / `update()` below, where the call runs; a Csr's rows always go in slot order)
            out = self._max_detour(edge_index, x.to(dev), pseudo, slot_rows=not slot_order).to(x.device)
            return _glued(out, residual, relu)
        if self._flipped() and not (isinstance(edge_index, ops.Csr) and edge_index._flow_flipped):
            csr = self._flow_csr(edge_index, x)
        else:
            csr = self._square_csr(edge_index, x)
        if pseudo.size(0) != csr.n_edges:
            raise ValueError(f"edge_attr has {pseudo.size(0)} rows, edge_index {csr.n_edges} edges")
        return self._operator(x, ops._ONE_SET, csr, pseudo if slot_order else _slot_rows(csr, pseudo), dev, needs_grad, residual, relu)

    def _propagate_two(self, x_src, x_dst, n_src, n_dst, edge_index, pseudo, residual, relu):
        """Between two node sets: sources x_src [n_src, out], destinations x_dst [n_dst, in_dst] or None (no root term, PyG's rule),
        edges (edge_index[0] in [0, n_src)) -> (edge_index[1] in [0, n_dst)) (rows swapped under flow='target_to_source')."""
        needs_grad = self._two_sets_gate([t for t in (x_src, x_dst, residual) if t is not None], pseudo)
        dev, csr = _dev_of(x_src), self._rect_csr(edge_index, x_src, n_src, n_dst, pseudo)
        return self._operator(x_src, x_dst, csr, _slot_rows(csr, pseudo), dev, needs_grad, residual, relu)

    def _operator(self, x_src, x_dst, csr, pseudo_s, dev, needs_grad, residual, relu):
        """k = edge_kernel(pseudo rows in slot order) by torch, then gather, message, aggregate and update() as ONE native call
        (gpde_diagconv_fwd; with a gradient DiagConvFunction, whose dL/dk autograd carries back into `nn`)."""
        k = self._checked_kernel(pseudo_s, csr.n_edges)
        k = k.float().to(dev).contiguous()              # (.float(): a float64 kernel network runs with float32 x, as at any width)
        on_dev = lambda t: _on_dev(t, dev, needs_grad)
        root, bias = (None if x_dst is None else on_dev(self.root)), on_dev(self.bias)      # PyG: no x_dst, no root term
        xs_d = x_src.to(dev) if needs_grad else x_src.detach().to(dev)
        xd_d = x_dst if not torch.is_tensor(x_dst) else x_dst.to(dev) if needs_grad else x_dst.detach().to(dev)
        if needs_grad:
            out = _glued(DiagConvFunction.apply(xs_d, xd_d, k, csr, root, bias, self.aggr), residual, relu)
        else:
            res = None if residual is None else residual.detach().to(dev)
            out = ops.diagconv_forward_raw(xs_d, xd_d, csr, k.detach(), root, bias, self.aggr, residual=res, relu=relu)
        return out.to(x_src.device)

    def message(self, x_j, pseudo):                    # nn_conv.py:83-85
        """m_e = x_j[e] . diag(k_e) = x_j[e] * k_e."""
        k = self._checked_kernel(pseudo, x_j.size(0))
        return x_j * k.to(device=x_j.device, dtype=x_j.dtype)

    def update(self, aggr_out, x):                     # nn_conv.py:87-92
        if self.root is not None:
            aggr_out = aggr_out + torch.mm(x, self.root.to(x.device))
        if self.bias is not None:
            aggr_out = aggr_out + self.bias.to(aggr_out.device)
        return aggr_out


class NNConvGaussian(NNConvDiag):
    r"""`NNConv_Gaussian` (nn_conv.py:99-194): the diagonal message with the analytic kernel
        k_e = a_e * exp(-pseudo[e, 0]^2 / nn(ones(1))^2),   a_e = 1 / sqrt(|pseudo[e, 1] * pseudo[e, 2]|)        nn_conv.py:175-180
    `nn` maps a tensor of one element to the `out_channels` widths (the reference's hard-coded 64 is `out_channels` here), and the
    `ones(1)` lives on `pseudo`'s device (the reference takes a module-level `device`)."""

    _nn_line = "nn_conv.py:175-180"

    def edge_kernel(self, pseudo):
        if pseudo.dim() != 2 or pseudo.size(1) < 3:
            raise ValueError(f"the Gaussian kernel reads pseudo[:, 0], pseudo[:, 1] and pseudo[:, 2] (nn_conv.py:176-178), got {tuple(pseudo.shape)}")
        p = next(self.nn.parameters(), None)            # (a float64 `nn` is fed float64)
        one = torch.ones(1, device=pseudo.device, dtype=pseudo.dtype if p is None else p.dtype)
        widths = self.nn(one).reshape(1, -1)
        amplitude = (pseudo[:, 1] * pseudo[:, 2]).abs().sqrt().reciprocal().unsqueeze(1)
        return amplitude * torch.exp(-pseudo[:, 0:1].square() / widths.square())
