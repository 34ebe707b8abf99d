"""`GCNConv` - the graph convolution of Kipf & Welling behind the module surface of `torch_geometric.nn.GCNConv`, on the native
aggregation kernel (csrc/gpde_gcn.hip).  The reference's GCN baseline (multipole-graph-neural-operator/neurips4_GCN.py:28-31,
`GCNConv(width, width)` applied 16 times per forward) imports it from torch_geometric; the shim re-exports this class.

    out = D^-1/2 (A + I) D^-1/2 x W + bias

with PyG's `gcn_norm` (`add_remaining_self_loops`; the degree is the TARGET-side sum of PyG >= 1.6, see ops.gcn_norm).
Parameters are named as in the PyG the reference was written for: `weight` [in, out] (glorot), `bias` [out] (zeros)."""
import math

import torch
from torch.nn import Parameter

from . import ops
from .autograd import GCNFunction
from .message_passing import MessagePassing


def gcn_coefficients(edge_index, n: int, edge_weight=None, improved: bool = False, add_self_loops: bool = True,
                     normalize: bool = True, dtype=torch.float32):
    """(edge_index', coef') of the normalised adjacency with stock torch ops - `add_remaining_self_loops`, index_add degree,
    pow(-0.5) - on whatever device the tensors live: the host path of the module."""
    row, col = edge_index[0], edge_index[1]
    w = torch.ones(row.numel(), dtype=dtype, device=row.device) if edge_weight is None else edge_weight.to(dtype).view(-1)
    if not normalize:
        return edge_index, w
    if add_self_loops:
        loop = row == col
        fill = torch.full((n,), 2.0 if improved else 1.0, dtype=dtype, device=row.device)
        if bool(loop.any()):                                # an existing self loop gives its weight: the largest edge id per node wins
            ids = torch.nonzero(loop).view(-1)
            last = torch.full((n,), -1, dtype=torch.long, device=row.device).scatter_reduce(0, row[ids], ids, "amax")
            fill = torch.where(last >= 0, w[last.clamp(min=0)], fill)
        keep = ~loop
        ar = torch.arange(n, dtype=row.dtype, device=row.device)
        row, col, w = torch.cat([row[keep], ar]), torch.cat([col[keep], ar]), torch.cat([w[keep], fill])
    deg = torch.zeros(n, dtype=dtype, device=row.device).index_add_(0, col, w)
    dinv = deg.pow(-0.5)
    dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
    return torch.stack([row, col]), dinv[row] * w * dinv[col]


class GCNConv(MessagePassing):
    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, normalize=True, add_self_loops=True,
                 flow="source_to_target"):
        for name, v in (("improved", improved), ("cached", cached), ("bias", bias), ("normalize", normalize),
                        ("add_self_loops", add_self_loops)):
            if not isinstance(v, bool):
                raise NotImplementedError(f"{name} must be True or False")
        if not ops.width_supported(in_channels, out_channels):
            raise ValueError(f"GCNConv({in_channels!r}, {out_channels!r}): the native operator is built for widths 1 .. {ops.ANY_MAX_WIDTH}")
        super().__init__(aggr="add", flow=flow)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.improved, self.cached, self.normalize, self.add_self_loops = improved, cached, normalize, add_self_loops
        self.weight = Parameter(torch.empty(self.in_channels, self.out_channels))
        if bias:
            self.bias = Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        bound = math.sqrt(6.0 / (self.in_channels + self.out_channels))            # glorot
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.zero_()
        self._cached_host = self._cached_device = None      # cached=True: the pinned normalisation of the host path / of the device path

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """State dicts written by newer PyG releases store the weight as `lin.weight [out, in]` (a bias-free Linear): accepted
        and transposed, as NNConv does for its root weight."""
        k_new, k_old = prefix + "lin.weight", prefix + "weight"
        if k_new in state_dict and k_old not in state_dict:
            state_dict[k_old] = state_dict.pop(k_new).t().contiguous()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _host_forward(self, x, edge_index, edge_weight):
        if isinstance(edge_index, ops.Csr):
            raise ValueError("an ops.Csr is a device graph: a CPU x needs the edge_index tensor")
        n = x.size(0)
        if self.cached and self._cached_host is not None:
            ei, coef = self._cached_host
        else:
            ei = edge_index.flip(0) if self.flow == "target_to_source" else edge_index
            ei, coef = gcn_coefficients(ei.to(x.device), n, None if edge_weight is None else edge_weight.to(x.device), self.improved,
                                        self.add_self_loops, self.normalize, dtype=x.dtype)
            if self.cached:
                self._cached_host = (ei, coef)
        agg = torch.zeros(n, x.size(1), dtype=x.dtype, device=x.device).index_add(0, ei[1], x.index_select(0, ei[0]) * coef.view(-1, 1))
        out = torch.mm(agg, self.weight.to(x.dtype))
        return out if self.bias is None else out + self.bias.to(x.dtype)

    def forward(self, x, edge_index, edge_weight=None, *, route=None):
        """`edge_index`: int64 [2, E] with any strides, or an `ops.Csr` (under flow='target_to_source' one built with flip=True); `edge_weight` [E] in edge order (no gradient); `route`:
        force one of ops.GCN_ROUTES (tests).  A CPU x computes the same formula with stock torch ops."""
        x = x.unsqueeze(-1) if x.dim() == 1 else x
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"x must be [N, {self.in_channels}], got {tuple(x.shape)}")
        if edge_weight is not None and edge_weight.requires_grad:
            raise NotImplementedError("the gradient with respect to edge_weight is not built: pass edge_weight.detach()")
        if not x.is_cuda:
            return self._host_forward(x, edge_index, edge_weight)
        with ops.ver_scope():
            if self.cached and self._cached_device is not None and self._cached_device.csr.rowptr.device == x.device:
                norm = self._cached_device
                norm.order()             # (pinned here, never looked up again: a call on another stream is a cache hit like any other)
                if norm.csr.n_nodes != x.size(0):
                    raise ValueError(f"cached=True pinned a graph of {norm.csr.n_nodes} nodes, x has {x.size(0)} rows")
            else:
                if not isinstance(edge_index, ops.Csr) and not edge_index.is_cuda:
                    edge_index = ops.stage_const(edge_index, x.device)
                if edge_weight is not None and not edge_weight.is_cuda:
                    edge_weight = ops.stage_const(edge_weight, x.device)
                flip = self.flow == "target_to_source"
                if flip and isinstance(edge_index, ops.Csr):
                    if not edge_index._flow_flipped:
                        raise ValueError("flow='target_to_source' with an ops.Csr: the CSR must have been built for that flow "
                                         "(ops.csr_for(edge_index, n, flip=True)); a CSR cannot be reversed in place")
                    flip = False
                csr = ops.csr_for(edge_index, int(x.size(0)), flip=flip)
                norm = ops.gcn_norm(csr, edge_weight, self.improved, self.add_self_loops, self.normalize)
                if self.cached:
                    self._cached_device = norm
            if torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or (self.bias is not None and self.bias.requires_grad)):
                return GCNFunction.apply(x, self.weight, self.bias, norm, route)
            return ops.gcn_forward_raw(x, norm, self.weight, self.bias, route=route)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"
