"""Test infrastructure: GCNConv as a differentiable composite of stock torch ops, for script-level parity.

`composite_forward(x, edge_index, edge_weight)` is what `torch_geometric.nn.GCNConv` does with torch ops - `add_remaining_self_loops`,
the degree by `index_add`, `pow(-0.5)`, gather by `edge_index[0]`, scale, scatter-add over `edge_index[1]`, `mm` with the weight,
bias - on whatever device the script's tensors live, differentiated by torch autograd: what neurips4_GCN.py ran on before the
native operator existed.  tests/test_gpu_gcn_script.py runs the script once on libgpde.so and once with `GCNConv.forward`
replaced by this.  Only `scripts/run_reference_script.py --composite` installs it; the product never imports it."""
import torch


def composite_forward(self, x, edge_index, edge_weight=None, **kw):
    x = x.unsqueeze(-1) if x.dim() == 1 else x
    n = x.size(0)
    if self.flow == "target_to_source":
        edge_index = edge_index.flip(0)
    row, col = edge_index[0], edge_index[1]
    w = torch.ones(row.numel(), dtype=x.dtype, device=x.device) if edge_weight is None else edge_weight.to(x.dtype)
    if self.normalize:
        if self.add_self_loops:                                   # add_remaining_self_loops
            loop = row == col
            fill = torch.full((n,), 2.0 if self.improved else 1.0, dtype=x.dtype, device=x.device)
            fill[row[loop]] = w[loop]
            ar = torch.arange(n, dtype=row.dtype, device=row.device)
            row, col, w = torch.cat([row[~loop], ar]), torch.cat([col[~loop], ar]), torch.cat([w[~loop], fill])
        deg = torch.zeros(n, dtype=x.dtype, device=x.device).index_add(0, col, w)
        dinv = deg.pow(-0.5)
        dinv = dinv.masked_fill(dinv == float("inf"), 0.0)
        w = dinv[row] * w * dinv[col]
    msg = x.index_select(0, row) * w.view(-1, 1)
    out = torch.mm(torch.zeros(n, x.size(1), dtype=x.dtype, device=x.device).index_add(0, col, msg), self.weight)
    return out if self.bias is None else out + self.bias


def install(counter=None):
    """Replace `forward` of graph_pde_amd.GCNConv (the class the shim re-exports) by the composite.  `counter`: the dict of
    composite_nnconv.install() to share - 'calls' moves with every composite forward of either operator."""
    from graph_pde_amd import gcn_conv
    counter = {"calls": 0} if counter is None else counter

    def fwd(self, x, edge_index, edge_weight=None, **kw):
        counter["calls"] += 1
        return composite_forward(self, x, edge_index, edge_weight, **kw)
    gcn_conv.GCNConv.forward = fwd
    return counter
