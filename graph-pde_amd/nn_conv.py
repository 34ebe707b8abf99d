"""Drop-in modules with the reference's surface:

* `NNConv_old`  -- /root/reference/graph-neural-operator/nn_conv.py:197-286 (full w x w edge kernel;
  the class every GKN script instantiates), and
* `NNConv`      -- the name `torch_geometric.nn.NNConv` resolves to for the MGKN scripts
  (MGKN_general_darcy2d.py:8,45,53,61; MGKN_orthogonal_burgers1d.py:8,37); same math.

Same constructor, attributes (`in_channels, out_channels, nn, aggr, root, bias`), parameter
names / shapes (`root [in,out]`, `bias [out]`), `reset_parameters`, `forward(x, edge_index,
edge_attr)`, `message(x_j, pseudo)`, `update(aggr_out, x)`, `__repr__`; instances pickle with
`torch.save(model)` (no native handles on the module).  `forward` runs the fused HIP operator of
libgpde.so; there is no other execution path: CPU tensors (a model moved back with `model.cpu()`,
UAI1_full_resolution.py:287-303) are staged to the current HIP device, run through the same kernels and
the result is copied back - without a HIP device the call raises.

`_ConvFront` holds what `NNConv_old` and the diagonal modules of diag_conv.py share: the constructor, the (in_src, in_dst) /
flow plumbing, the validation of a call between two node sets, the CSR of a call and the detour of a gradient through 'max'.
"""
from __future__ import annotations

import math

import torch
from torch.nn import Parameter

from . import hidden_cache, ops
from . import autograd as _ag
from .autograd import (ChainAnyFunction, HiddenAnyFunction, NNConvDeferredFunction, NNConvFunction, NNConvHiddenFunction, SharedParamFunction, WeConvAnyFunction,
                       WeConvFunction)
from .message_passing import MessagePassing


def _reset(nn):
    """`torch_geometric.nn.inits.reset` (imported at nn_conv.py:4): call reset_parameters() on every
    leaf that has one."""
    def _r(item):
        if hasattr(item, "reset_parameters"):
            item.reset_parameters()
    if nn is not None:
        children = list(nn.children()) if hasattr(nn, "children") else []
        if children:
            for item in children:
                _reset(item)
        else:
            _r(nn)


def _uniform(size, tensor):
    """`torch_geometric.nn.inits.uniform`: U(-1/sqrt(size), 1/sqrt(size)).  Written under no_grad on the
    parameter itself (not through `.data`): the in-place version counter moves, so packed-weight caches
    keyed on it cannot serve the old values."""
    if tensor is not None:
        bound = 1.0 / math.sqrt(size)
        with torch.no_grad():
            tensor.uniform_(-bound, bound)


def _rows(t):
    """`t` as rows: a 1-D tensor is one column (an `ops.NodeAttr` answers dim() == 2 and passes)."""
    return t.unsqueeze(-1) if t.dim() == 1 else t


def _materialized(node_attr, edge_index):
    """An `ops.NodeAttr` as the [E, k0] tensor the reference builds: gathered along `edge_index` (a tensor, or a Csr - then along
    its slots: the rows come out in slot order)."""
    return node_attr.materialize(edge_index.edge_index if isinstance(edge_index, ops.Csr) else edge_index.to(node_attr.device))


def _dev_of(x):
    """Where a call on `x` runs: its device, or - CPU tensors - the current HIP device."""
    return x.device if x.is_cuda else ops.staging_device()


def _on_dev(t, dev, needs_grad):
    """`t` (or None) on `dev`: itself when it is there, a differentiable `.to(dev)` when a gradient is needed, else the device copy
    that ops.stage_const caches on the tensor's storage + version."""
    if t is None or t.device == dev:
        return t
    return t.to(dev) if needs_grad and t.requires_grad else ops.stage_const(t, dev)


def _wants_grad(*tensors) -> bool:
    """Whether autograd has to see a call over `tensors` (Nones and `ops.NodeAttr`s - requires_grad False - pass)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _slot_rows(csr, rows):
    """`rows` [E, .], one per edge of the caller's list, in CSR slot order: the order the kernels address a per-edge operand in."""
    return rows if bool(getattr(csr, "_perm_is_identity", False)) else rows.index_select(0, csr.perm.long().to(rows.device))


def _glued(out, residual, relu):
    """act(residual + out) by torch ops: the callers' elementwise glue where it is not fused into a kernel."""
    if residual is not None:
        out = residual.to(out.device) + out
    return torch.relu(out) if relu else out


class _GatherRows(torch.autograd.Function):
    """x.index_select(0, idx) whose backward sums the gradient rows of one index in a FIXED order.  torch's own backward of
    index_select adds them with float atomics on the device: a node with several out-edges then gets a grad_x whose last bits
    differ from run to run (tests/test_gpu_layouts.py saw it on the 'max' chain, the one place a gather of x is left to torch).
    index_put_(accumulate=True) sorts the indices and adds the rows of an index one after the other."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.save_for_backward(idx)
        ctx.shape = tuple(x.shape)
        return x.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return torch.zeros(ctx.shape, dtype=g.dtype, device=g.device).index_put_((idx,), g.contiguous(), accumulate=True), None


def _front_args(in_channels, aggr, kwargs, aggr_line):
    """The constructor checks of `NNConv_old` and `NNConvDiag` (`aggr_line`: where the reference states the choices):
    (in_channels - an int or a pair (in_src, in_dst) -, flow)."""
    flow = kwargs.pop("flow", "source_to_target")
    if flow not in ("source_to_target", "target_to_source"):
        raise ValueError(f"flow must be 'source_to_target' or 'target_to_source', got {flow!r}")
    if kwargs:
        raise TypeError(f"unexpected arguments {sorted(kwargs)}")
    if aggr not in ("add", "mean", "max"):
        raise ValueError(f"aggr must be 'add', 'mean' or 'max' ({aggr_line}), got {aggr!r}")
    if isinstance(in_channels, (tuple, list)):
        if len(in_channels) != 2:
            raise ValueError(f"in_channels must be an int or a pair (in_src, in_dst), got {in_channels!r}")
        in_channels = (in_channels[0], in_channels[1])
    return in_channels, flow


class _ConvFront(MessagePassing):
    """The front `NNConv_old` and `NNConvDiag` share.  Both derive `MessagePassing` like the reference (nn_conv.py:8, 197) and
    override `propagate` with a native operator; `in_channels` may be a pair (in_src, in_dst), `flow` either direction."""

    def __init__(self, in_channels, out_channels, nn, aggr, root_weight, bias, flow):
        super().__init__(aggr=aggr, flow=flow)                     # nn_conv.py:53, 242
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.nn = nn
        if root_weight:
            self.root = Parameter(torch.Tensor(self._in_dst(), out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):                       # nn_conv.py:72-75, 261-265
        _reset(self.nn)
        size = self._in_src()
        _uniform(size, self.root)
        _uniform(size, self.bias)

    def _in_src(self):
        return self.in_channels[0] if isinstance(self.in_channels, tuple) else self.in_channels

    def _in_dst(self):
        return self.in_channels[1] if isinstance(self.in_channels, tuple) else self.in_channels

    def _flipped(self) -> bool:
        return self.flow == "target_to_source"

    def _needs_grad(self, *tensors) -> bool:
        """Whether this call needs a gradient: autograd is on and one of `tensors` or of the module's parameters asks for one."""
        return torch.is_grad_enabled() and (_wants_grad(*tensors) or any(p.requires_grad for p in self.parameters()))

    def _rect_call(self, x, size, residual=None):
        """Whether `forward(x, ..., size)` / `propagate(..., size=, x=)` is a call between two node sets, validated without a device:
        None for today's square call (a tensor, or a pair of the SAME tensor, with `size` square or None, on a module of one
        width), else (x_src, x_dst, n_src, n_dst)."""
        pair = isinstance(x, (tuple, list))
        if pair and len(x) != 2:
            raise ValueError(f"x must be a tensor or a pair (x_src, x_dst), got {len(x)} entries")
        x_src, x_dst = (x[0], x[1]) if pair else (x, x)
        if not torch.is_tensor(x_src) or not (x_dst is None or torch.is_tensor(x_dst)):
            raise ValueError("x must be a tensor or a pair (x_src tensor, x_dst tensor or None)")
        if size is not None:
            sz = list(size) if isinstance(size, (list, tuple)) else [size, size]
            if len(sz) != 2:
                raise ValueError(f"size must be (n_src, n_dst), got {size!r}")
            sz = [None if v is None else int(v) for v in sz]
        else:
            sz = [None, None]
        x_src = _rows(x_src)
        if x_dst is not None:
            x_dst = _rows(x_dst)
        n = int(x_src.size(0))
        same = (not pair) or (x[1] is x[0])
        if same and not isinstance(self.in_channels, tuple) and all(v is None or v == n for v in sz):
            return None
        if sz[0] is not None and sz[0] != n:
            raise ValueError(f"size[0] = {sz[0]} but x_src has {n} rows")
        if x_dst is not None and sz[1] is not None and sz[1] != int(x_dst.size(0)):
            raise ValueError(f"size[1] = {sz[1]} but x_dst has {int(x_dst.size(0))} rows")
        if sz[1] is not None:
            n_dst = sz[1]
        elif x_dst is not None:
            n_dst = int(x_dst.size(0))
        else:
            raise ValueError("the number of destination nodes is unknown: give size=(n_src, n_dst) or x_dst (it is not guessed from the "
                             "largest index of edge_index)")
        if n < 0 or n_dst < 0:
            raise ValueError(f"size must be non-negative, got ({n}, {n_dst})")
        cs, cd, co = self._in_src(), self._in_dst(), self.out_channels
        if x_src.dim() != 2 or x_src.size(1) != cs:
            raise ValueError(f"x_src must be [n_src, {cs}] (in_channels of the sources), got {tuple(x_src.shape)}")
        if x_dst is not None and (x_dst.dim() != 2 or x_dst.size(1) != cd):
            raise ValueError(f"x_dst must be [n_dst, {cd}] (in_channels of the destinations), got {tuple(x_dst.shape)}")
        if residual is not None and tuple(residual.shape) != (n_dst, co):
            raise ValueError(f"residual must be [n_dst, out_channels] = [{n_dst}, {co}], got {tuple(residual.shape)}")
        return x_src, x_dst, n, n_dst

    def _no_unflipped_csr(self, edge_index):
        if self._flipped() and isinstance(edge_index, ops.Csr) and not edge_index._flow_flipped:
            raise NotImplementedError("flow='target_to_source' with a destination CSR (ops.Csr): a CSR has its direction built in - "
                                      "pass the edge_index tensor")

    def _square_csr(self, edge_index, x, flip=False):
        """The CSR of a call on one node set: a `Csr` as it is, else the cached CSR of `edge_index` (rows swapped: `flip`) where
        the call runs - an index tensor that lives elsewhere is staged there."""
        if isinstance(edge_index, ops.Csr):
            return edge_index
        dev = _dev_of(x)
        return ops.csr_for(edge_index if edge_index.device == dev else ops.stage_const(edge_index, dev), x.size(0), flip=flip)

    def _flow_csr(self, edge_index, x):
        """flow='target_to_source': the operator runs on `edge_index` with its rows swapped.  The destination CSR of the swapped
        list, built (and cached) from the caller's tensor in place; every square path takes a `Csr` where it takes edge_index."""
        self._no_unflipped_csr(edge_index)
        return self._square_csr(edge_index, x, flip=True)

    def _rect_csr(self, edge_index, x_src, n_src, n_dst, pseudo):
        """The rectangular CSR of a call between two node sets (rows swapped under flow='target_to_source'; a `Csr` is checked
        against both node counts), `pseudo` checked against its edges."""
        dev = _dev_of(x_src)
        self._no_unflipped_csr(edge_index)
        if isinstance(edge_index, ops.Csr):
            csr = ops.csr_for(edge_index, n_dst, n_src=n_src)
        else:
            csr = ops.csr_for(edge_index if edge_index.device == dev else ops.stage_const(edge_index, dev), n_dst, n_src=n_src,
                              flip=self._flipped())
        if pseudo.size(0) != csr.n_edges:
            raise ValueError(f"edge_attr has {pseudo.size(0)} rows, edge_index {csr.n_edges} edges")
        return csr

    def _two_sets_gate(self, tensors, pseudo) -> bool:
        """The refusals every call between two node sets shares; returns whether the call needs a gradient (`tensors`: x_src,
        x_dst and residual where given)."""
        if any(t.dtype != torch.float32 for t in tensors):
            raise NotImplementedError(f"a call between two node sets: float32 only (got {[str(t.dtype) for t in tensors]})")
        needs_grad = self._needs_grad(*tensors, pseudo)
        if self.aggr == "max" and needs_grad:
            raise NotImplementedError("aggr='max' with a gradient on a call between two node sets is not built (inference runs natively: "
                                      "call under torch.no_grad())")
        return needs_grad

    def _max_detour(self, edge_index, x, pseudo, slot_rows=None):
        """A gradient through aggr='max' on one node set (no graph-pde script uses it; a freshly built module in grad mode lands
        here): PyG's own chain - gather, `message`, segment max, `update` (MessagePassing.propagate applies `flow`
        itself) - over the module's differentiable `message()` / `update()`, x_j gathered by `_GatherRows`: grad_x is the same bits
        on every run.  A `Csr` is handed over as its slot list, turned back where it was built with the rows swapped; `slot_rows`:
        whether the rows of `pseudo` still have to be put in slot order for it (default: for a swapped CSR only - NNConv_old reads
        a caller's own `Csr` with its rows as given)."""
        if isinstance(edge_index, ops.Csr):
            csr, edge_index = edge_index, edge_index.edge_index
            swapped = csr._flow_flipped and self._flipped()
            if swapped if slot_rows is None else slot_rows:
                pseudo = _slot_rows(csr, pseudo)
            if swapped:
                edge_index = edge_index.flip(0)
        return MessagePassing.propagate(self, edge_index.to(x.device), x=x, pseudo=pseudo, _gather=_GatherRows.apply)

    def propagate(self, edge_index, size=None, **kwargs):
        """`propagate(edge_index, x=x, pseudo=pseudo)` (the reference's call, nn_conv.py:81, 271): gather x_j, `message`, aggregate
        over `edge_index[1]`, `update` - as the native operator `forward` runs instead of PyG's index_select / message / scatter /
        update chain.  `size`: (n_src, n_dst) of a call between two node sets; otherwise it may only restate the node count."""
        if set(kwargs) != {"x", "pseudo"}:
            raise TypeError(f"propagate() takes x= and pseudo= ({self._propagate_line}), got {sorted(kwargs)}")
        return self.forward(kwargs["x"], edge_index, kwargs["pseudo"], size=size)

    def __repr__(self):                               # nn_conv.py:94-96, 284-286
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


class NNConv_old(_ConvFront):
    r"""x'_i = Theta x_i + aggr_{j in N(i)} x_j . h_Theta(e_ij)   with h_Theta a kernel MLP emitting
    in_channels*out_channels values per edge (nn_conv.py:197-232).  Derives `MessagePassing` like the reference
    (nn_conv.py:197, 242) and overrides `propagate` with the fused HIP operator.

    A call is decided top to bottom, each step once: `forward` (`propagate` is `forward` without the extras) validates, tells a
    call between two node sets from a square one, refuses `ops.NodeAttr` where it is not built, swaps the rows under
    flow='target_to_source' and makes `x` rows -> `_propagate_rect` (two node sets) or `_propagate_one`, which composes the glue
    by torch ops unless it can be fused and hands the operator to `_operator_one`: any other width -> `_propagate_any_width`;
    CPU tensors -> staged, then as on the device; a kernel network outside the Linear / ReLU chain -> `_propagate_general_nn`;
    else `_propagate_64` -> `_train_64` with a gradient, `_infer_64` without.

    Widths: 64 -> 64 (every reference configuration) runs the re-associated fused kernels.  Any other pair of
    1 <= in_channels, out_channels <= 256 takes the reference's own order for every kernel network: `weight =
    self.nn(pseudo)` by the caller's module ([E, in * out], as nn_conv.py:274 materialises it), then message / aggregate /
    update as ONE native kernel over it (`_propagate_any_width`, csrc/gpde_weconv_any.hip).  Wider raises
    NotImplementedError.

    Two node sets (torch_geometric.nn.NNConv's bipartite form): `in_channels` may be a pair `(in_src, in_dst)` - `nn` emits
    in_src * out values per edge, `root` is [in_dst, out] -, `forward` takes `x = (x_src, x_dst)` (x_dst may be None: no root
    term) and `size = (n_src, n_dst)`, and `edge_index[0]` then indexes the sources, `edge_index[1]` the destinations:
        out_i = aggr_{e: j -> i} x_src[j] . W_e  (+ x_dst[i] . root)  + bias                          out [n_dst, out_channels]
    Such a call runs the any-width kernels at every width (`_propagate_rect`; 64 -> 64 included).  Not built for it: a gradient
    through aggr='max', `ops.NodeAttr` attributes, the hidden / edge-weight caches and the shared launch of `nnconv_group`.
    `flow='target_to_source'` swaps the two rows of `edge_index` (read in place through a negative row stride, no copy) at every
    width.

    Kernel networks with other activations: `Linear, (act, Linear)+` with act one of ReLU, LeakyReLU (slope >= 0), ELU, Tanh, Sigmoid,
    GELU (both forms), SiLU and `graph_pde_amd.Sin` per hidden layer (ops.mlp_chain) has a route that forms no per-edge tensor wider
    than `edge_attr`: the STREAMED any-width route (gpde_nnconv_*_chain_act), taken under GPDE_ANY_REASSOC=streamed, under `auto` by
    a call whose per-edge weights do not fit, and at 64 -> 64 on one node set by a call that `_propagate_general_nn` would refuse
    for memory.  Calls that fit keep their route.  The reference's `DenseNet_sin` applies `torch.sin` inside its `forward`, where no
    parser of layers sees it, and therefore keeps the general route; `DenseNet(layers, graph_pde_amd.Sin)` is the streamed form."""

    _propagate_line = "nn_conv.py:271"

    def __init__(self, in_channels, out_channels, nn, aggr="add", root_weight=True, bias=True,
                 **kwargs):
        in_channels, flow = _front_args(in_channels, aggr, kwargs, "nn_conv.py:222-224")
        super().__init__(in_channels, out_channels, nn, aggr, root_weight, bias, flow)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """State dicts written by newer PyG releases store the root weight as `lin.weight [out, in]` (a bias-free
        Linear) instead of `root [in, out]`: accepted and transposed."""
        k_new, k_old = prefix + "lin.weight", prefix + "root"
        if k_new in state_dict and k_old not in state_dict:
            state_dict[k_old] = state_dict.pop(k_new).t().contiguous()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x, edge_index, edge_attr, *, size=None, residual=None, activation=None):      # nn_conv.py:267-271
        """The reference signature `forward(x, edge_index, edge_attr)`; `x` may be a pair `(x_src, x_dst)` and `size=` the pair
        `(n_src, n_dst)` (torch_geometric.nn.NNConv: a graph between two node sets, class docstring; `size` is keyword-only here:
        the positional parameters are the reference's three).  Two more keyword-only, opt-in extras fuse the
        callers' elementwise glue into the operator's last kernel: `residual` (a [N, 64] tensor
        added to the result) and `activation="relu"` - `conv(x, ei, ea, residual=x, activation="relu")` equals
        `F.relu(x + conv(x, ei, ea))` (MGKN_general_darcy2d.py:79-80).  Fused for inference on device tensors;
        when a gradient is needed the same value is composed from the unfused operator and torch ops.
        The one entry of `forward` and `propagate`: everything a call is normalised by happens here, once."""
        if activation not in (None, "relu"):
            raise ValueError(f"activation must be None or 'relu', got {activation!r}")
        rect = self._rect_call(x, size, residual)
        flip = rect is None and self._flipped() and not (isinstance(edge_index, ops.Csr) and edge_index._flow_flipped)
        if isinstance(edge_attr, ops.NodeAttr):
            if rect is not None:
                raise NotImplementedError("ops.NodeAttr attributes on a call between two node sets are not built: a node table addresses ONE "
                                          "node set - pass the edge_attr tensor")
            if flip:
                raise NotImplementedError("ops.NodeAttr attributes with flow='target_to_source' are not built - pass the edge_attr tensor")
        with ops.ver_scope():        # (inference tensors: one content checksum per tensor and call, shared by all cache keys)
            if rect is not None:
                return self._propagate_rect(*rect, edge_index, _rows(edge_attr), residual, activation == "relu")
            x = x[0] if isinstance(x, (tuple, list)) else x
            fusable = x.dim() == 2          # (a 1-D x - in_channels == 1 - has always composed its glue by torch ops)
            x = _rows(x)
            if flip:
                edge_index = self._flow_csr(edge_index, x)
            return self._propagate_one(x, edge_index, edge_attr, residual, activation == "relu", fusable)

    def _propagate_one(self, x, edge_index, edge_attr, residual, relu, fusable):
        """A call on ONE node set, normalised by `forward`.  `residual` / `relu` are fused into the operator's last kernel for
        inference on device tensors (float32 `x`, a tensor `edge_attr`, at 64 -> 64 a Linear / ReLU chain); otherwise the same
        value is composed from the plain operator and torch ops."""
        if residual is not None or relu:
            if not self._is_width_64():
                self._check_width()
            fusable = fusable and x.is_cuda and x.dtype == torch.float32 and torch.is_tensor(edge_attr) and \
                (residual is None or residual.device == x.device) and not self._needs_grad(x, edge_attr, residual) and \
                (not self._is_width_64() or self._nn_is_linear_relu_chain())
            if not fusable:
                return _glued(self._operator_one(x, edge_index, edge_attr), residual, relu)
        return self._operator_one(x, edge_index, edge_attr, residual, relu)

    def _operator_one(self, x, edge_index, edge_attr, residual=None, relu=False):
        """The operator of a call on one node set (`residual` / `relu`: fused, the caller made sure they can be): which regime
        runs, and - in one place - what becomes of an `ops.NodeAttr`."""
        wide = self._is_width_64()
        if not wide:
            self._check_width()
        lin = self._linears() if wide and x.is_cuda else None
        if isinstance(edge_attr, ops.NodeAttr):
            # opt-in: attributes read from node data inside the kernel, for a Linear / ReLU chain at 64 -> 64
            # on the device.  Inference on the default f16-split kernel, and training (round 4) where the descriptor can travel
            # the ordinary ladder - every native call then reads the table (`node_attr` of the entry points); anything else,
            # and a node table that wants a gradient (the node-table kernels do not differentiate the table, the differentiable
            # gather does -> grad_edge_attr of gpde_nnconv_bwd), takes the tensor the reference would build.
            native = lin is not None and not _wants_grad(edge_attr.table)
            needs_grad = self._needs_grad(x)
            if native and not needs_grad and self.aggr != "max" and len(lin) == 3 and ops.DEFAULT_PRECISION == "f16split":
                csr = ops.csr_for(edge_index, x.size(0))
                pm = ops.pack_mlp([l.weight for l in lin], [l.bias for l in lin])
                return ops.nnconv_forward_nodeattr_raw(x, csr, edge_attr, pm, self.root, self.bias, self.aggr)
            if not (native and needs_grad and self.aggr in ("add", "mean") and x.dtype == torch.float32 and
                    all(l.bias is not None for l in lin) and
                    ops.nodeattr_train_supported([lin[0].in_features] + [l.out_features for l in lin])):
                edge_attr = _materialized(edge_attr, edge_index)
        pseudo = _rows(edge_attr)
        if not wide:
            return self._propagate_any_width(x, edge_index, pseudo, residual=residual, relu=relu)
        if not x.is_cuda:
            # CPU tensors (`model.cpu()` + evaluation, UAI1_full_resolution.py:287-303): inputs and parameters are
            # copied to the current HIP device (`.to()` is differentiable, so gradients flow back to the CPU parameters), the SAME
            # kernels run without the hidden cache, the output returns to the caller's device
            dev = ops.staging_device()
            ei_d = edge_index if isinstance(edge_index, ops.Csr) else ops.stage_const(edge_index, dev)
            ea_d = pseudo.to(dev) if pseudo.requires_grad else ops.stage_const(pseudo, dev)
            return self._propagate_64(x.to(dev), ei_d, ea_d, *self._params_on(dev, torch.is_grad_enabled()), use_hidden_cache=False).to(x.device)
        if lin is None:
            return self._propagate_general_nn(x, edge_index, pseudo)
        return self._propagate_64(x, edge_index, pseudo, [l.weight for l in lin], [l.bias for l in lin], self.root, self.bias,
                                  use_hidden_cache=True, residual=residual, relu=relu)

    def _linears(self):
        """The Linear layers of `nn` when it is the Linear / ReLU chain the fused kernels re-associate, else None."""
        try:
            return ops.mlp_linears(self.nn)
        except NotImplementedError:
            return None

    def _nn_is_linear_relu_chain(self) -> bool:
        return self._linears() is not None

    def _propagate_general_nn(self, x, edge_index, pseudo):
        """`nn` is "a neural network h_Theta ... e.g. torch.nn.Sequential" (nn_conv.py:217-221): anything that is not the
        Linear / ReLU chain the fused kernels re-associate - `DenseNet(normalize=True)` (BatchNorm1d) or `out_nonlinearity`
        (utilities.py:207-221), `DenseNet_sin` (multipole utilities.py:233-252), a user's own module.  The reference's own order
        then: `weight = self.nn(pseudo).view(-1, in, out)` (nn_conv.py:274) by the caller's module as torch ops on the device -
        16 KiB per edge, exactly the tensor the reference materialises - and message / aggregate / update (nn_conv.py:275-282) as
        ONE native kernel over it (gpde_nnconv_fwd_edgeweights; backward gpde_nnconv_bwd_edgeweights, whose dL/dW_e autograd
        carries back into `nn`).  The operator itself never leaves libgpde.so; what cannot be fused is the caller's network."""
        if self.aggr not in ("add", "mean"):
            return self._max_detour(edge_index, x, pseudo)
        if x.dtype != torch.float32:
            raise NotImplementedError(f"a kernel network outside the Linear / ReLU chain: float32 only (x is {x.dtype})")
        csr = ops.csr_for(edge_index, x.size(0))
        need = csr.n_edges * ops.WIDTH * ops.WIDTH * 4
        free, _ = ops.device_free_bytes(x.device)
        if 2 * need > free:
            # the per-edge weights do not fit.  `Linear, (act, Linear)+` with an activation the library generates (ops.mlp_chain:
            # GELU, SiLU, tanh, sin, ...) runs STREAMED instead, from the edge attributes by block of destination nodes
            # (gpde_nnconv_*_chain_act; the any-width kernels take 64 -> 64).  A call that fits keeps its route and its bits
            chain = ops.mlp_chain(self.nn)
            if chain is not None:
                lin, acts = chain
                dims = [lin[0].in_features] + [l.out_features for l in lin]
                route = ops.any_width_route(csr.n_nodes, csr.n_edges, ops.WIDTH, ops.WIDTH, dims[-2], self.aggr, dims[-1] == ops.WIDTH * ops.WIDTH,
                                            free, mode="off" if ops.ANY_REASSOC == "off" else "auto", dims=dims, acts=acts)
                if route["route"] == "streamed":
                    return self._any_width_operator(x, ops._ONE_SET, csr, pseudo, "streamed", lin, x.device, self._needs_grad(x, pseudo), None,
                                                    False, acts=acts)
            raise RuntimeError(f"kernel network {type(self.nn).__name__} is not a Linear / ReLU chain: its per-edge weights are materialised as in the "
                               f"reference (nn_conv.py:274) - {csr.n_edges} edges x 16 KiB = {need / 2**30:.1f} GiB (twice that with gradients), "
                               f"{free / 2**30:.1f} GiB free")
        weight = self.nn(_slot_rows(csr, pseudo))       # (`nn` acts row by row, batch statistics are order-free)
        if weight.dim() != 2 or weight.size(0) != csr.n_edges or weight.size(1) != ops.WIDTH * ops.WIDTH:
            raise ValueError(f"nn(pseudo) must be [E, {ops.WIDTH * ops.WIDTH}] (in_channels * out_channels, nn_conv.py:274), got {tuple(weight.shape)}")
        weight = weight.float().contiguous()
        if _wants_grad(x, weight, self.root, self.bias):
            return WeConvFunction.apply(x, weight, csr, self.root, self.bias, self.aggr, None)
        return ops.nnconv_forward_edgeweights_raw(x, csr, weight.detach(), self.root, self.bias, self.aggr)

    def _is_width_64(self) -> bool:
        """64 -> 64: the width of every reference configuration, the one the fused (re-associated) kernels are built for."""
        return self.in_channels == ops.WIDTH and self.out_channels == ops.WIDTH

    def _check_width(self):
        if not ops.width_supported(self.in_channels, self.out_channels):
            raise NotImplementedError(
                f"the MI355X operator is built for 1 <= in_channels, out_channels <= {ops.ANY_MAX_WIDTH} (fused kernels at "
                f"{ops.WIDTH} -> {ops.WIDTH}, the per-edge-weight kernels of gpde_weconv_any.hip at every other width), "
                f"got {self.in_channels}->{self.out_channels}")

    def _propagate_any_width(self, x, edge_index, pseudo, residual=None, relu=False):
        """The operator of a module whose widths are not (64, 64), for EVERY kernel network (the Linear / ReLU chain included):
        the route of `_propagate_general_nn` at run-time widths, on ONE node set.  This front validates, builds the square CSR and
        decides the route (ops.any_width_route states the rule: the per-edge weights materialised as in the reference, or - a
        Linear / ReLU chain under add / mean that does not fit, GPDE_ANY_REASSOC=auto, or every such call, =on - the last Linear
        re-associated; =streamed: every such call from the edge attributes, hidden rows by node block); `_any_width_operator` runs
        it.  `residual` / `relu`: fused into the kernel's epilogue; callers pass them
        only when no gradient is needed.  aggr='max': the native kernel when no gradient is needed, else `_max_detour`, as at 64."""
        cin, cout = int(self.in_channels), int(self.out_channels)
        if x.dim() != 2 or x.size(1) != cin:
            raise ValueError(f"x must be [N, {cin}] (in_channels), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise NotImplementedError(f"widths other than {ops.WIDTH} -> {ops.WIDTH}: float32 only (x is {x.dtype})")
        needs_grad = self._needs_grad(x, pseudo)
        if self.aggr == "max" and needs_grad:
            return self._max_detour(edge_index, x, pseudo)
        dev, csr = _dev_of(x), self._square_csr(edge_index, x)
        # the route (ops.any_width_route; GPDE_ANY_REASSOC = auto | on | off): a call whose per-edge weights fit runs on them exactly
        # as before; a Linear / ReLU chain under add / mean that does not fit (auto), or every such call (on), re-associates the
        # last Linear and never forms [E, in * out]
        route, lin, acts, free = self._any_width_route(csr, dev)
        if route["route"] == "refused":
            other = ""
            if route["eligible"] and ops.ANY_REASSOC != "off":
                other = (f"; re-associated (GPDE_ANY_REASSOC={ops.ANY_REASSOC}): hidden activations and one node block of Z' = "
                         f"{route['bytes_reassociated'] / 2**30:.2f} GiB (twice that with gradients)")
            raise RuntimeError(f"{self!r}: at widths other than {ops.WIDTH} -> {ops.WIDTH} the per-edge weights are materialised as in the reference "
                               f"(nn_conv.py:274) - {csr.n_edges} edges x {cin} x {cout} x 4 B = {route['bytes_materialised'] / 2**30:.2f} GiB "
                               f"(twice that with gradients), {free / 2**30:.2f} GiB free{other}")
        return self._any_width_operator(x, ops._ONE_SET, csr, pseudo, route["route"], lin, dev, needs_grad, residual, relu, acts=acts)

    def _any_width_route(self, csr, dev):
        """(ops.any_width_route of a call on `csr`, the Linear layers of `nn` when it is a Linear / ReLU chain or - ops.mlp_chain - a
        chain with other hidden activations, else None -, those activations - None for the ReLU chain -, the free bytes of `dev`)."""
        cin, cout = int(self._in_src()), int(self.out_channels)
        free, _ = ops.device_free_bytes(dev)
        lin, acts = self._linears(), None
        if lin is None:
            lin, acts = ops.mlp_chain(self.nn) or (None, None)
        chain = lin is not None and lin[-1].out_features == cin * cout
        dims = [lin[0].in_features] + [l.out_features for l in lin] if chain else None
        args = (csr.n_nodes, csr.n_edges, cin, cout, lin[-1].in_features if chain else None, self.aggr, chain, free)
        kw = {} if acts is None else {"dims": dims, "acts": acts}      # (a Linear / ReLU chain asks exactly as it always did)
        route = ops.any_width_route(*args, **kw)
        if route["route"] == "streamed" and not ops.chain_any_supported(dims):       # a chain the library does not generate: as under `off`
            route = ops.any_width_route(*args, mode="off", **kw)
        return route, lin, acts, free

    def _any_width_operator(self, x_src, x_dst, csr, pseudo, route, lin, dev, needs_grad, residual, relu, acts=None):
        """The operator of `_propagate_any_width` (`x_dst` ops._ONE_SET) and of `_propagate_rect` (`x_dst` a tensor or None) once the
        route is decided - a call on one node set is the two-set call that hands one table twice.  Rows of `pseudo` in CSR slot
        order, where the module lives; parameters and CPU tensors staged to `dev` (`.to()` is differentiable), the result back on
        the caller's device.
        Materialised: `weight = self.nn(pseudo)` [E, in_src * out] by the caller's module - the tensor the reference materialises
        (nn_conv.py:274) -, then gather, message, aggregate and update() (nn_conv.py:275-282) as ONE native kernel
        (gpde_nnconv_fwd_edgeweights_any / _bip; the backward's dL/dW_e autograd carries back into `nn`).
        Re-associated (`lin`: a Linear / ReLU chain, add / mean): H = relu(L_{n-1}(... pseudo)) [E, K] by torch, then aggregation, the
        LAST Linear per destination and update() as ONE native call (gpde_nnconv_fwd_hidden_any / _bip; dL/dH flows on through the
        earlier layers by autograd).
        Streamed (GPDE_ANY_REASSOC=streamed; the same chains): `pseudo` and the chain's weights go to ONE native call that generates
        the hidden rows by block of destination nodes (gpde_nnconv_fwd_chain_any; its backward recomputes them and differentiates the
        whole chain) - no per-edge tensor wider than `pseudo` exists.  `acts` (ops.mlp_chain): the chain's hidden activations when
        they are not all ReLU - GELU, SiLU, tanh, sin, ... -, which only this route takes (gpde_nnconv_*_chain_act).
        `residual` [n_dst, out] / `relu`: the kernel's epilogue on the materialised call without a gradient, torch ops otherwise."""
        one = x_dst is ops._ONE_SET
        cin, cout = int(self._in_src()), int(self.out_channels)
        pseudo_s = None if route == "streamed" else _slot_rows(csr, pseudo)      # (`nn` acts row by row, batch statistics are order-free)
        on_dev = lambda t: _on_dev(t, dev, needs_grad)
        root, bias = (None if x_dst is None else on_dev(self.root)), on_dev(self.bias)      # PyG: no x_dst, no root term
        xs_d = x_src.to(dev) if needs_grad else x_src.detach().to(dev)
        xd_d = x_dst if not torch.is_tensor(x_dst) else x_dst.to(dev) if needs_grad else x_dst.detach().to(dev)
        if route == "streamed":
            # (.float(): as on the re-associated route, a float64 kernel network runs with float32 x)
            params = [on_dev(l.weight).float() for l in lin] + [None if l.bias is None else on_dev(l.bias).float() for l in lin]
            ea = pseudo.to(dev) if needs_grad and pseudo.requires_grad else pseudo.detach().to(dev)
            out = ChainAnyFunction.apply(xs_d, xd_d, ea, csr, root, bias, self.aggr, acts, *params)      # (no graph when nothing needs one)
        elif route == "reassociated":
            h = pseudo_s
            for l in lin[:-1]:
                h = torch.relu(torch.nn.functional.linear(h, l.weight, l.bias))
            hidden = h.float().to(dev).contiguous()
            # (.float(): a float64 kernel network runs with float32 x on the other route too, through `weight.float()`)
            w_last, b_last = on_dev(lin[-1].weight).float(), None if lin[-1].bias is None else on_dev(lin[-1].bias).float()
            if needs_grad:
                out = HiddenAnyFunction.apply(xs_d, xd_d, hidden, w_last, b_last, csr, root, bias, self.aggr)
            elif one:
                out = ops.nnconv_forward_hidden_any_raw(xs_d, csr, hidden.detach(), w_last, b_last, root, bias, self.aggr)
            else:
                out = ops.nnconv_forward_hidden_bip_raw(xs_d, xd_d, csr, hidden.detach(), w_last, b_last, root, bias, self.aggr)
        else:
            weight = self.nn(pseudo_s)
            if weight.dim() != 2 or weight.size(0) != csr.n_edges or weight.size(1) != cin * cout:
                raise ValueError(f"nn(pseudo) must be [E, {cin * cout}] = [{csr.n_edges}, {'in_channels' if one else 'in_src'} * out_channels] "
                                 f"(nn_conv.py:274), got {tuple(weight.shape)}")
            weight = weight.float().to(dev).contiguous()
            if needs_grad:
                out = WeConvAnyFunction.apply(xs_d, xd_d, weight, csr, root, bias, self.aggr)
            else:
                res = None if residual is None else residual.detach().to(dev)
                if one:
                    out = ops.nnconv_forward_edgeweights_any_raw(xs_d, csr, weight.detach(), root, bias, self.aggr, residual=res, relu=relu)
                else:
                    out = ops.nnconv_forward_edgeweights_bip_raw(xs_d, xd_d, csr, weight.detach(), root, bias, self.aggr, residual=res, relu=relu)
                return out.to(x_src.device)
        return _glued(out, residual, relu).to(x_src.device)

    def _propagate_rect(self, x_src, x_dst, n_src, n_dst, edge_index, pseudo, residual, relu):
        """A call BETWEEN TWO NODE SETS: sources x_src [n_src, in_src], destinations x_dst [n_dst, in_dst] or None, edges
        (edge_index[0] in [0, n_src)) -> (edge_index[1] in [0, n_dst)) (rows swapped under flow='target_to_source'), out
        [n_dst, out].  The routes of `_propagate_any_width` at EVERY width, 64 -> 64 included, on the rectangular entry points
        (gpde_nnconv_*_edgeweights_bip / gpde_nnconv_*_hidden_bip; ops.any_width_route decides with n_dst as its node count).
        This front validates, builds the rectangular CSR and decides the route; `_any_width_operator` runs it.  x_dst None: no root
        term although the module may have a root (PyG's rule).  aggr='max' with a gradient is not built."""
        cin, cind, cout = self._in_src(), self._in_dst(), self.out_channels
        if not (ops.width_supported(cin, cout) and ops.width_supported(cind, cout)):
            raise NotImplementedError(f"the MI355X operator is built for 1 <= in_channels, out_channels <= {ops.ANY_MAX_WIDTH}, got "
                                      f"{self.in_channels}->{self.out_channels}")
        needs_grad = self._two_sets_gate([t for t in (x_src, x_dst, residual) if t is not None], pseudo)
        dev, csr = _dev_of(x_src), self._rect_csr(edge_index, x_src, n_src, n_dst, pseudo)
        route, lin, acts, free = self._any_width_route(csr, dev)
        if route["route"] == "refused":
            raise RuntimeError(f"{self!r}: a call between two node sets materialises the per-edge weights as the reference does (nn_conv.py:274) - "
                               f"{csr.n_edges} edges x {int(cin)} x {int(cout)} x 4 B = {route['bytes_materialised'] / 2**30:.2f} GiB (twice that with "
                               f"gradients), {free / 2**30:.2f} GiB free (GPDE_ANY_REASSOC={ops.ANY_REASSOC})")
        return self._any_width_operator(x_src, x_dst, csr, pseudo, route["route"], lin, dev, needs_grad, residual, relu, acts=acts)

    def _propagate_64(self, x, edge_index, pseudo, weights, biases, root, bias, use_hidden_cache, residual=None, relu=False):
        """The 64 -> 64 operator of a Linear / ReLU chain on device tensors: gather, message, aggregate, update of the reference as
        native calls.  `weights / biases / root / bias` are the tensors to use (the module's own, or staged copies).  Computed once,
        here: `needs_grad`, the CSR and the packed kernel MLP; then the training or the inference ladder."""
        needs_grad = self._needs_grad(x, pseudo)
        if self.aggr == "max":
            if needs_grad:
                return self._max_detour(edge_index, x, pseudo)      # (the fused inference kernel serves the calls without a gradient)
            if residual is None and not relu and (pseudo.dtype != torch.float32 or x.dtype != torch.float32):
                raise NotImplementedError(f"aggr='max': float32 only (got x {x.dtype}, edge_attr {pseudo.dtype})")
        csr = ops.csr_for(edge_index, x.size(0))
        pm = ops.pack_mlp(weights, biases)
        if needs_grad:          # (`residual` / `relu` are None / False: the glue of a call with a gradient is composed by torch ops)
            return self._train_64(x, csr, pseudo, pm, weights, biases, root, bias, use_hidden_cache)
        return self._infer_64(x, csr, pseudo, pm, weights, biases, root, bias, residual, relu, use_hidden_cache=use_hidden_cache)

    def _train_64(self, x, csr, pseudo, pm, weights, biases, root, bias, use_hidden_cache):
        """The training ladder at 64 -> 64: the shared W_e node, the shared H, the deferred backward, the direct operator."""
        # cross-depth reuse (hidden_cache.py): this module applied again with the same edge_attr and
        # weights shares one hidden-activation tensor with the earlier applications
        if use_hidden_cache and hidden_cache.MODE != "off" and self.aggr in ("add", "mean") and \
                pseudo.dtype == torch.float32 and x.dtype == torch.float32:
            hit = hidden_cache.lookup(self, pseudo, csr, pm, weights, biases,
                                      allow_partial=hidden_cache.defer_possible(pseudo, pm, weights, biases, self.aggr))
            if hit is not None and hit[2] == csr.n_nodes:
                hidden, hmax, _ = hit
                # low in-degree / small graph (the MGKN V-cycles): the per-edge weights as a shared autograd node, the
                # call itself one streaming kernel forward and one backward
                we = hidden_cache.lookup_edge_weights_train(self, hidden, csr, pm, weights, biases)
                if we is not None:
                    tok = hidden_cache.we_token_of(self, we)
                    if tok is not None and _ag.ACCUMULATE_GRAD_HIDDEN:
                        # root / bias behind private identity nodes, one per step and module: the applications sum their
                        # gradients in place there (autograd.SharedParamFunction)
                        # (... of THESE parameter objects at THEIR current versions: the W_e node outlives a forward whose
                        # backward never ran, and a root / bias written in place since then invalidates the old views)
                        vers = (None if root is None else ops._ver(root), None if bias is None else ops._ver(bias))
                        if tok.side_in is None or tok.side_in[2] is not root or tok.side_in[3] is not bias or tok.side_in[4] != vers:
                            tok.side_in = (None if root is None else SharedParamFunction.apply(root, tok, 0),
                                           None if bias is None else SharedParamFunction.apply(bias, tok, 1), root, bias, vers)
                        return WeConvFunction.apply(x, we, csr, tok.side_in[0], tok.side_in[1], self.aggr, tok)
                    return WeConvFunction.apply(x, we, csr, root, bias, self.aggr, None)
                return NNConvHiddenFunction.apply(x, hidden, csr, pm, weights[-1], biases[-1],
                                                  root, bias, self.aggr, hmax, hidden_cache.token_of(self, hidden, csr))
            # H wanted but too large for the device (the 241^2 graph: 391 GB): the applications of this forward share a
            # "virtual H" node instead - light backward per application, ONE deferred pass for the hidden layers; the
            # part of H that does fit (`hit`: the in-edges of the leading nodes) is read instead of recomputed
            d = hidden_cache.lookup_deferred(self, pseudo, csr, pm, weights, biases, self.aggr, hpart=hit)
            if d is not None:
                return NNConvDeferredFunction.apply(x, d[0], csr, pseudo, root, bias, self.aggr, d[1],
                                                    len(weights), *weights, *biases)
        return NNConvFunction.apply(x, csr, pseudo, root, bias, self.aggr, len(weights), *weights, *biases)

    def _infer_64(self, x, csr, pseudo, pm, weights, biases, root, bias, residual=None, relu=False, *, use_hidden_cache=True,
                  explicit=False, batch=None):
        """The inference ladder at 64 -> 64, for a call that needs NO gradient: the per-edge-weight call, the cached H (full, or
        partial -> the mixed forward), the direct operator.  What its callers differ in is said by its parameters:
          * `residual` / `relu` (the fused glue): the raw wrappers fuse it, on a FULL H or on the edge attributes - no partial H, no
            mixed forward; no per-edge association (ops.per_edge_association: NNConvFunction's, which has no epilogue); and
            aggr='max' beyond the per-edge-weight form is refused by the direct operator instead of answered here;
          * `explicit` (nnconv_group): the caller opted into the per-edge-weight form, hidden_cache.WE_MODE is not consulted;
            `batch`: its list - a call in that form is appended to it for the shared launch and None returned;
          * `use_hidden_cache=False` (staged CPU calls): no cache is consulted, aggr='max' apart (it has no other form)."""
        glue = residual is not None or relu
        force = self.aggr == "max"
        # inference on a low in-degree / small graph (or aggr='max'): one streaming kernel over the cached per-edge weights
        # (hidden_cache.lookup_edge_weights - None when the form does not apply: graph too dense / too large, not opted in or,
        # in `auto`, module not seen repeating yet -).
        # (the glue call never had the edge_attr dtype guard; it matters under aggr='max' only, whose forced build then refuses
        # float64 attributes itself - any other float64 call finds no H to derive W_e from)
        if (glue or pseudo.dtype == torch.float32) and x.dtype == torch.float32 and (use_hidden_cache or force):
            we = hidden_cache.lookup_edge_weights(self, pseudo, csr, pm, weights, biases, force=force, explicit=explicit)
            if we is not None:
                call = dict(x=x, csr=csr, edge_weights=we, root=root, bias=bias, aggr=self.aggr, residual=residual, relu=relu)
                if batch is not None:
                    batch.append(call)
                    return None
                return ops.nnconv_forward_edgeweights_group([call])[0]
        if force and not glue:
            if csr.n_edges == 0:
                # a graph without edges: every segment is empty, its max is 0 (PyG's fill) exactly as its sum - update() alone
                return NNConvFunction.apply(x, csr, pseudo, root, bias, "add", len(weights), *weights, *biases)
            raise NotImplementedError(
                f"aggr='max': the per-edge weights of this call ({csr.n_edges} edges x 16 KiB) "
                "exceed the cache budget (GPDE_HIDDEN_CACHE_GB / GPDE_EDGE_WEIGHT_CACHE_GB)")
        if use_hidden_cache and hidden_cache.MODE != "off" and self.aggr in ("add", "mean") and \
                pseudo.dtype == torch.float32 and x.dtype == torch.float32:
            hit = hidden_cache.lookup(self, pseudo, csr, pm, weights, biases, allow_partial=not glue)
            if hit is not None and hit[2] == csr.n_nodes and glue:
                return ops.nnconv_forward_hidden_raw(x, csr, hit[0].detach(), pm, root, bias, self.aggr, hmax=hit[1],
                                                     residual=residual, relu=relu)
            if hit is not None and hit[2] == csr.n_nodes:
                return NNConvHiddenFunction.apply(x, hit[0], csr, pm, weights[-1], biases[-1], root, bias, self.aggr, hit[1],
                                                  hidden_cache.token_of(self, hit[0], csr))
            if hit is not None:        # H of the leading nodes only: mixed forward (never with the glue: allow_partial)
                return ops.nnconv_forward_mixed_raw(x, csr, pseudo, hit[0], hit[1], hit[2], pm, root, bias, self.aggr)
        if glue:
            return ops.nnconv_forward_raw(x, csr, pseudo, pm, root, bias, self.aggr, residual=residual, relu=relu)
        # (the plain call runs the autograd Functions as a call with a gradient does - under torch.no_grad() they still keep Z for a
        # parameter that requires a gradient, other bits than the raw wrappers' - ; the fused glue exists on the raw wrappers only)
        return NNConvFunction.apply(x, csr, pseudo, root, bias, self.aggr, len(weights), *weights, *biases)

    def _params_on(self, dev, need_grad):
        """The module's parameters as tensors on `dev`: (kernel-MLP weights, biases, root, bias).  Parameters already
        there are returned AS THEY ARE (same objects: the pack cache of ops.pack_mlp recognises them).  CPU parameters
        (a model moved back with `model.cpu()`): a differentiable `.to(dev)` when a gradient is needed, otherwise the
        device copy cached by ops.stage_const on the CPU tensor's storage + version - repeated evaluation calls then
        share one copy and one pack instead of re-packing 24 MB per call."""
        one = lambda t: _on_dev(t, dev, need_grad)
        lin = ops.mlp_linears(self.nn)
        return [one(l.weight) for l in lin], [one(l.bias) for l in lin], one(self.root), one(self.bias)

    def message(self, x_j, pseudo):                    # nn_conv.py:273-275
        """m_e = x_j[e] . W(pseudo_e)  ([E, in] x [E, in, out] -> [E, out]).  Computed by the same native
        operator on the graph in which every edge has its own target (E nodes, edge e: e -> e, aggr='add', no
        root / bias): out[e] = x_j[e] . h_Theta(pseudo_e), exactly the reference's message."""
        self._check_width()
        x_j, pseudo = _rows(x_j), _rows(pseudo)
        e, dev = x_j.size(0), _dev_of(x_j)
        ar = torch.arange(e, device=dev, dtype=torch.int64)
        ident = torch.stack([ar, ar])                      # (a one-off graph: built by ops.build_csr, nothing cached)
        if not self._is_width_64():
            # any other width: `weight = self.nn(pseudo)` (nn_conv.py:274), then the native operator on the identity graph
            weight = self.nn(pseudo)
            if weight.dim() != 2 or tuple(weight.shape) != (e, self.in_channels * self.out_channels):
                raise ValueError(f"nn(pseudo) must be [E, {self.in_channels * self.out_channels}] (nn_conv.py:274), got {tuple(weight.shape)}")
            weight = weight.float().to(dev).contiguous()
            csr = ops.build_csr(ident, e)
            if _wants_grad(x_j, weight):
                out = WeConvAnyFunction.apply(x_j.float().to(dev), ops._ONE_SET, weight, csr, None, None, "add")
            else:
                out = ops.nnconv_forward_edgeweights_any_raw(x_j.detach().float().to(dev), csr, weight.detach(), None, None, "add")
            return out.to(x_j.device)
        weights, biases, _, _ = self._params_on(dev, torch.is_grad_enabled())
        out = NNConvFunction.apply(x_j.to(dev), ops.build_csr(ident, e), pseudo.to(dev), None, None, "add", len(weights), *weights, *biases)
        return out.to(x_j.device)

    def update(self, aggr_out, x):                     # nn_conv.py:277-282
        """aggr_out + x . root + bias.  The `x . root + bias` term is the native operator on the graph without
        edges (its epilogue kernel); the sum with aggr_out is one elementwise add."""
        if self.root is None and self.bias is None:
            return aggr_out
        self._check_width()
        dev = _dev_of(x)
        empty = torch.empty(2, 0, dtype=torch.int64, device=dev)
        if not self._is_width_64():
            # any other width: x . root + bias is the any-width operator on the graph without edges
            x = _rows(x)
            wants = _wants_grad(x, self.root, self.bias)
            root, bias = _on_dev(self.root, dev, wants), _on_dev(self.bias, dev, wants)
            csr = ops.build_csr(empty, x.size(0))
            no_we = torch.empty(0, int(self.in_channels) * int(self.out_channels), dtype=torch.float32, device=dev)
            if wants:
                term = WeConvAnyFunction.apply(x.float().to(dev), ops._ONE_SET, no_we, csr, root, bias, "add")
            else:
                term = ops.nnconv_forward_edgeweights_any_raw(x.detach().float().to(dev), csr, no_we, root, bias, "add")
            return aggr_out + term.to(aggr_out.device)
        weights, biases, root, bias = self._params_on(dev, torch.is_grad_enabled())
        csr = ops.build_csr(empty, x.size(0))      # edgeless: no sort, nothing cached
        no_attr = torch.empty(0, weights[0].size(1), device=dev)
        if not _wants_grad(x, root, bias):
            term = ops.nnconv_forward_raw(x.to(dev), csr, no_attr, ops.pack_mlp(weights, biases), root, bias, "add")
        else:
            # the kernel MLP takes no part in update(): its (staged) parameters enter detached
            term = NNConvFunction.apply(x.to(dev), csr, no_attr, root, bias, "add", len(weights),
                                        *[w.detach() for w in weights], *[None if b is None else b.detach() for b in biases])
        return aggr_out + term.to(aggr_out.device)


class NNConv(NNConv_old):
    """`torch_geometric.nn.NNConv` as the MGKN scripts use it (full edge kernel, same math as
    NNConv_old).  Note: the diagonal variant that
    graph-neural-operator/nn_conv.py:8-96 also calls `NNConv` is `graph_pde_amd.NNConvDiag` (diag_conv.py)."""
    pass


ECConv = NNConv


def nnconv_group(calls):
    """Run several INDEPENDENT NNConv calls - e.g. the 13 `conv_list[l](phi[l], ...)` of one upward sweep of the
    MGKN-orthogonal V-cycle, whose inputs the downward pass fixed beforehand (MGKN_orthogonal_burgers1d.py:65-82) - and
    return their outputs in order.  `calls`: sequence of (conv, x, edge_index, edge_attr[, residual[, activation]]).
    Calls that can run from cached per-edge weights (inference, low in-degree / small graphs: DESIGN.md §6d) share ONE
    kernel launch per 16 (gpde_nnconv_fwd_edgeweights_group); every other call runs as `conv(x, edge_index, edge_attr,
    residual=, activation=)`.  The result of each call is bit-identical to calling the module on its own."""
    outs = [None] * len(calls)
    batch, where = [], []
    for k, c in enumerate(calls):
        conv, x, edge_index, edge_attr = c[0], c[1], c[2], c[3]
        residual = c[4] if len(c) > 4 else None
        activation = c[5] if len(c) > 5 else None
        if activation not in (None, "relu"):
            raise ValueError(f"activation must be None or 'relu', got {activation!r}")
        # the shared launch is built for square 64 -> 64 inference calls on device tensors in the caller's own edge order; a call
        # between two node sets, with the rows swapped, of another width or with a gradient simply runs on its own
        square = not (isinstance(x, (tuple, list)) or isinstance(conv.in_channels, tuple) or conv.flow != "source_to_target")
        if square and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and torch.is_tensor(edge_attr) and \
                edge_attr.dtype == torch.float32 and (residual is None or residual.device == x.device) and conv._is_width_64() and \
                not conv._needs_grad(x, residual, edge_attr):
            # the module's own inference ladder, opted into the per-edge-weight form: after that rung it is the ladder a plain call
            # of the module descends (a second, unopted look for W_e cannot succeed where the opted one did not)
            lin = ops.mlp_linears(conv.nn)
            weights, biases = [l.weight for l in lin], [l.bias for l in lin]
            with ops.ver_scope():
                csr = ops.csr_for(edge_index, x.size(0))
                outs[k] = conv._infer_64(x, csr, _rows(edge_attr), ops.pack_mlp(weights, biases), weights, biases, conv.root, conv.bias,
                                         residual, activation == "relu", explicit=True, batch=batch)
            if outs[k] is None:
                where.append(k)
        else:
            outs[k] = conv(x, edge_index, edge_attr, residual=residual, activation=activation)
    for k, o in zip(where, ops.nnconv_forward_edgeweights_group(batch)):
        outs[k] = o
    return outs
