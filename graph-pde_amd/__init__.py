"""graph-pde_amd: the MI355X-native edge-conditioned graph convolution (NNConv) of
neuraloperator/graph-pde — hand-written HIP for gfx950 behind the reference's module surface.

    from graph_pde_amd import NNConv_old, NNConv          # drop-in modules (nn_conv.py)
    from graph_pde_amd import NNConvDiag, NNConvGaussian   # the diagonal-kernel classes of the reference's nn_conv.py (diag_conv.py)
    from graph_pde_amd import GCNConv                      # the GCN baseline's convolution on the native aggregation kernel (gcn_conv.py)
    from graph_pde_amd import ops                          # CSR / packing / raw forward
    from graph_pde_amd import sampled_graph                # the reference's gaussian_connectivity as the operator's CSR (sampled_graph.py)
    from graph_pde_amd import neighbor_graph               # exact k-nearest-neighbour graphs as the operator's CSR (neighbor_graph.py)
    fwd = graph_pde_amd.capture(model_fn, x)               # opt-in: the call sequence of a sample as ONE HIP graph (capture.py)

(The directory is named `graph-pde_amd`; `graph_pde_amd.py` at the repo root makes it importable.)
"""
from . import _lib, neighbor_graph, ops, sampled_graph, synth          # noqa: F401
from .nn_conv import ECConv, NNConv, NNConv_old, nnconv_group   # noqa: F401
from .gcn_conv import GCNConv                       # noqa: F401
from .diag_conv import NNConvDiag, NNConvGaussian   # noqa: F401  (the reference's diagonal-kernel classes, nn_conv.py:8-194)
from .ops import NodeAttr                           # noqa: F401  (opt-in: edge attributes from node data)
from .ops import Sin                                # noqa: F401  (torch.sin as a module: the sine kernel network the streamed route reads)
from .capture import capture                        # noqa: F401  (opt-in: a model function's native calls as one HIP graph)

__all__ = ["NNConv_old", "NNConv", "ECConv", "NNConvDiag", "NNConvGaussian", "GCNConv", "NodeAttr", "Sin", "nnconv_group", "capture", "ops", "sampled_graph", "neighbor_graph", "synth"]
