"""Drop-in for graph-neural-operator/nn_conv.py: same module name, same class names.  `NNConv_old` (the class every GKN script
instantiates, nn_conv.py:197-286) is the fused MI355X operator.  `NNConv` (diagonal edge kernel, nn_conv.py:8-96) and
`NNConv_Gaussian` (nn_conv.py:99-194) - imported by neurips1_GKN.py:10 / neurips5_GKN.py:10, instantiated by no script - are
`graph_pde_amd.NNConvDiag` / `NNConvGaussian` on the native diagonal operator.  (Under THIS module name `NNConv` is the diagonal
class, as in the reference's file; `torch_geometric.nn.NNConv` stays the full-kernel class.)"""
import _bootstrap  # noqa: F401
from graph_pde_amd.nn_conv import NNConv_old  # noqa: F401
from graph_pde_amd.diag_conv import NNConvDiag as NNConv  # noqa: F401
from graph_pde_amd.diag_conv import NNConvGaussian as NNConv_Gaussian  # noqa: F401

ECConv = NNConv
