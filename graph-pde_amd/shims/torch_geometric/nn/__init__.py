"""`torch_geometric.nn`: NNConv is the fused MI355X operator, GCNConv the GCN baseline's convolution on the native
aggregation kernel (neurips4_GCN.py:10,28-31; neurips1_MGKN.py:10 imports it without using it)."""
import _bootstrap  # noqa: F401
from graph_pde_amd.nn_conv import NNConv  # noqa: F401
from graph_pde_amd.gcn_conv import GCNConv  # noqa: F401
from . import conv, inits  # noqa: F401
from .conv import MessagePassing  # noqa: F401
