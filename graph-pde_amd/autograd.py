"""`torch.autograd.Function` around the fused NNConv (libgpde.so): forward = one gpde_nnconv_fwd
call, backward = one gpde_nnconv_bwd call (include/gpde.h).  Nothing but the inputs is saved: the
backward recomputes the hidden activations chunk by chunk.

Cross-depth reuse: `HiddenFunction` materialises the hidden
activations H(edge_attr; hidden layers) once, `NNConvHiddenFunction` is the operator given H.  When a
module is applied `depth` times with the same edge_attr and weights, all `depth` applications share
one H node: autograd sums their dL/dH and `HiddenFunction.backward` runs the MLP backward once.

Depth-deferred backward: when H does not fit memory (the 241^2 graph: 391 GB) the same sharing is done
WITHOUT the tensor.  `DeferredHiddenFunction` returns a one-element "virtual H" tensor that every application of the module
takes as an input (`NNConvDeferredFunction`); their backward passes compute grad_x and the node-side gradients only
(gpde_nnconv_bwd_light) and leave (x, grad_out) on the shared token; autograd runs the virtual node's backward after all of
them, and that ONE gpde_nnconv_bwd_deferred pass forms the hidden layers' gradients of all applications.
"""
from __future__ import annotations

import os

import torch
from torch.autograd.function import once_differentiable

from . import ops


def _save_attr(ctx, edge_attr):
    """The tensor to put into save_for_backward for `edge_attr`: itself, or - for an ops.NodeAttr (attributes read from node
    data) - its node table, the descriptor riding on ctx."""
    if isinstance(edge_attr, ops.NodeAttr):
        ctx.node_attr = edge_attr
        return edge_attr.table
    ctx.node_attr = None
    return edge_attr


def _saved_attr(ctx, t):
    return t if ctx.node_attr is None else ctx.node_attr


# dL/dH of the applications of a module sharing H: summed inside the per-edge kernel (NNConvHiddenFunction.backward) unless "0"
ACCUMULATE_GRAD_HIDDEN = os.environ.get("GPDE_ACCUMULATE_DLDH", "1") != "0"


CAN_TELL_BACKWARD_PASS = hasattr(torch._C, "_current_graph_task_id")


def backward_pass() -> int:
    """The autograd graph task id of the backward pass the caller runs in; -1 outside one, and where this torch cannot tell."""
    return torch._C._current_graph_task_id() if CAN_TELL_BACKWARD_PASS else -1


def in_backward_pass() -> bool:
    """Whether the caller runs inside an autograd backward pass - a forward does when torch.utils.checkpoint recomputes a segment.
    The running sums and (x, grad_out) pairs that the applications of a module leave on their shared token then belong to the pass
    in flight: forward-time housekeeping must not clear them.
    On a torch without `torch._C._current_graph_task_id` the question cannot be answered (`CAN_TELL_BACKWARD_PASS` is False, this
    returns False): the in-place sums on the H / W_e tokens are off there anyway (`HiddenToken.start` needs a pass to key on,
    nothing is ever in flight on them), and hidden_cache.lookup_deferred hands out no virtual-H node - the one place where a
    forward inside a backward pass would lose work - so such calls take the direct operator."""
    return backward_pass() >= 0


def saved_tensor_hooks_active() -> bool:
    """Whether what a forward saves for its backward goes through saved-tensor hooks right now: a segment under
    torch.utils.checkpoint(use_reentrant=False) - in its forward AND in its recomputation -, torch.autograd.graph.save_on_cpu.
    A node built there saves placeholders that belong to that segment; unknown (an older torch) counts as no."""
    top = getattr(torch._C._autograd, "_top_saved_tensors_default_hooks", None)
    if top is None:
        return False
    try:
        return top(False) is not None
    except TypeError:
        return top() is not None


class NNConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, edge_index, edge_attr, root, bias, aggr, n_layers, *params):
        weights = list(params[:n_layers])
        biases = list(params[n_layers:])
        ops._require_cuda(x, "x")
        # a prebuilt ops.Csr (message() / update(): one-off graphs that must not enter the CSR cache) or edge_index
        csr = edge_index if isinstance(edge_index, ops.Csr) else ops.csr_for(edge_index, x.size(0))
        pm = ops.pack_mlp(weights, biases)
        per_edge = ops.per_edge_association(csr, pm.dims, aggr)
        # training: keep Z for the backward's dW_3 (ops.z_buffer: None when it does not pay / fit)
        ctx.z = ops.z_buffer(csr, pm.dims, x.device) if any(ctx.needs_input_grad) and aggr in ("add", "mean") and not per_edge else None
        ctx.h = None
        if ctx.z is not None and not edge_attr.requires_grad and ops.keep_hidden(csr, pm.dims, x.device):
            # round 5: the last hidden activations are WRITTEN by the forward (store kernel), aggregated from there, and handed to
            # the backward, which then does not recompute them (ops.keep_hidden: when 4 KiB per edge fit)
            try:
                ctx.h, hmax = ops.hidden_forward_raw(csr, edge_attr.detach(), pm, weights, biases)
            except torch.OutOfMemoryError:
                ctx.h = None
        if per_edge:
            out = ops.nnconv_forward_per_edge_raw(x.detach(), csr, edge_attr, pm, weights, biases, root, bias, aggr)
        elif ctx.h is not None:
            ops.n_kept_hidden += 1
            out = ops.nnconv_forward_hidden_raw(x.detach(), csr, ctx.h, pm, root, bias, aggr, hmax=hmax, z_keep=ctx.z)
        else:
            out = ops.nnconv_forward_raw(x.detach(), csr, edge_attr.detach(), pm, root, bias, aggr, z_keep=ctx.z)
        ctx.csr, ctx.aggr, ctx.n_layers = csr, aggr, n_layers
        ctx.has_bias = bias is not None
        ctx.attr_needs_grad = edge_attr.requires_grad
        ctx.save_for_backward(x, _save_attr(ctx, edge_attr), root, *params)
        return out

    @staticmethod
    @once_differentiable        # the native backward is not itself differentiable: create_graph=True raises
    def backward(ctx, grad_out):
        x, edge_attr, root, *params = ctx.saved_tensors
        edge_attr = _saved_attr(ctx, edge_attr)
        n = ctx.n_layers
        weights, biases = list(params[:n]), list(params[n:])
        res = ops.nnconv_backward_raw(
            x, ctx.csr, edge_attr, weights, biases, root, ctx.aggr, grad_out,
            need_root=root is not None, need_bias=ctx.has_bias, z_saved=ctx.z, need_attr=ctx.attr_needs_grad, hidden_saved=ctx.h)
        gx, gW, gb, groot, gbias = res[:5]
        ctx.z = ctx.h = None
        # dL/d edge_attr (round 4): only this direct operator differentiates the attributes - the cached paths step aside for an
        # edge_attr that requires a gradient (hidden_cache.lookup)
        return (gx, None, res[5] if ctx.attr_needs_grad else None, groot, gbias if ctx.has_bias else None, None, None, *gW, *gb)


class HiddenToken:
    """Validity flag shared between a cached H and its autograd node: once the node's backward has
    run, the graph behind H is gone and the cached tensor must not be reused for a new forward."""
    __slots__ = ("valid", "hmax", "gh_acc", "gh_tid", "gh_adds", "side_acc", "side_in")

    def __init__(self):
        self.valid = True
        self.hmax = None        # device scalar max |H| when the fused kernel recorded it
        self.gh_acc = None      # the running sum of dL/dH of the applications of ONE backward pass (NNConvHiddenFunction.backward)
        self.gh_tid = -1        # ... and that pass (autograd graph task id)
        self.gh_adds = 0        # ... and how many applications added to it in place
        self.side_acc = None    # (W_e token) the (grad_root, grad_bias) the applications of that pass add to in place as well
        self.side_in = None     # (W_e token) (root, bias) behind SharedParamFunction: private nodes only WeConvFunction consumes

    # The in-place gradient sums of the applications sharing this node (dL/dH; on a W_e token dL/dW_e with grad_root, grad_bias).
    # The invariant: ONE backward pass owns ONE set of running tensors - the first application of the pass hands autograd its
    # own (`start`), the others add to them inside their kernels (`find`, `added`) and return nothing, and nobody else
    # contributes, which the node's backward verifies when autograd hands it the sum (`taken`).  Another pass (retain_graph, a
    # checkpointed segment, a pass abandoned half way) never finds them: it starts new ones.
    def find(self, shape):
        """The running tensors of the pass in flight, (sum,) or (sum, grad_root, grad_bias), when it has started them in this
        shape; else None."""
        tid = backward_pass()
        if tid < 0 or self.gh_acc is None or self.gh_tid != tid or self.gh_acc.shape != shape:
            return None
        return (self.gh_acc, *(self.side_acc or ()))

    def start(self, acc, *side):
        """The first application of a pass hands over its tensors (no pass to key on: nothing is remembered, nothing is ever added)."""
        tid = backward_pass()
        if tid >= 0:
            self.gh_acc, self.gh_tid, self.gh_adds, self.side_acc = acc, tid, 0, (side or None)

    def added(self):
        """An application added in place to the tensors `find` gave it."""
        self.gh_adds += 1

    def drop(self):
        """Forget the running tensors: forward time outside a backward pass, a released cache, the end of the node's backward."""
        self.gh_acc, self.gh_adds, self.side_acc = None, 0, None

    def check(self, grad, lost: str, which=None):
        """`grad` arrives at a node's backward: RuntimeError(`lost`) when the applications of this pass added in place to ANOTHER
        buffer (a second kind of consumer contributed and autograd formed the sum out of place: the additions are not in `grad`).
        `which`: 0 / 1 for grad_root / grad_bias instead of the sum itself."""
        if self.gh_acc is None or self.gh_adds == 0 or self.gh_tid != backward_pass():
            return
        mine = self.gh_acc if which is None else self.side_acc[which]
        if mine is not None and grad.data_ptr() != mine.data_ptr():
            raise RuntimeError(lost)

    def taken(self, grad, lost: str):
        """`check`, then `drop`: `grad` IS the running sum when the applications summed in place, held by autograd from here."""
        self.check(grad, lost)
        self.drop()


class HiddenFunction(torch.autograd.Function):
    """H [E, K2P] = relu(L_{n-1}(... relu(L_1(edge_attr)))) in CSR row order (gpde_hidden_fwd)."""

    @staticmethod
    def forward(ctx, edge_attr, csr, pm, precision, token, n_hidden, *params):
        weights = list(params[:n_hidden])
        biases = list(params[n_hidden:])
        h, token.hmax = ops.hidden_forward_raw(csr, edge_attr.detach(), pm, weights + [None], biases + [None],
                                               precision)
        ctx.csr, ctx.dims, ctx.n_hidden, ctx.token = csr, tuple(pm.dims), n_hidden, token
        ctx.attr_needs_grad = edge_attr.requires_grad
        ctx.save_for_backward(_save_attr(ctx, edge_attr), *params)
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_h):
        if ctx.attr_needs_grad:
            raise NotImplementedError(
                "gradient with respect to edge_attr is not built (no reference script needs it)")
        tok = ctx.token
        tok.valid = False
        tok.taken(grad_h, "graph_pde_amd: the in-place sum of dL/dH lost its buffer (H has a consumer outside NNConvHiddenFunction); "
                          "set GPDE_ACCUMULATE_DLDH=0")
        edge_attr, *params = ctx.saved_tensors
        edge_attr = _saved_attr(ctx, edge_attr)
        n = ctx.n_hidden
        gW, gb = ops.hidden_backward_raw(ctx.csr, edge_attr, ctx.dims, list(params[:n]), list(params[n:]), grad_h)
        return (None, None, None, None, None, None, *gW, *gb)


class NNConvHiddenFunction(torch.autograd.Function):
    """The operator given H: aggregation of x_j (x) H_e, last Linear, update() (gpde_nnconv_fwd_hidden /
    gpde_nnconv_bwd in its `hidden` form)."""

    @staticmethod
    def forward(ctx, x, hidden, csr, pm, w_last, b_last, root, bias, aggr, hmax=None, token=None):
        ctx.z = ops.z_buffer(csr, pm.dims, x.device) if any(ctx.needs_input_grad) else None
        out = ops.nnconv_forward_hidden_raw(x.detach(), csr, hidden.detach(), pm, root, bias, aggr, hmax=hmax, z_keep=ctx.z)
        ctx.csr, ctx.dims, ctx.aggr = csr, tuple(pm.dims), aggr
        ctx.token = token           # the HiddenToken of the shared H (None: H is the caller's own tensor)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, hidden, w_last, b_last, root)
        return out

    @staticmethod
    @once_differentiable        # the native backward is not itself differentiable: create_graph=True raises
    def backward(ctx, grad_out):
        x, hidden, w_last, b_last, root = ctx.saved_tensors
        # The applications of a module that shares H each produce dL/dH [E, K2P]; autograd would keep the first and add the others
        # to it one by one (at s=61, depth 6: 4 of a 38 ms step; at s=121 five 72 GB passes).  Here the first application of a
        # backward pass hands autograd its tensor and remembers it on the H token; the others ADD to it inside the per-edge
        # kernel (same additions, same order: the same bits) and return nothing (the transitions: HiddenToken).
        tok = ctx.token
        share = tok is not None and ACCUMULATE_GRAD_HIDDEN and ctx.needs_input_grad[1] and ctx.csr.n_edges >= 32 * ctx.csr.n_nodes
        acc = tok.find(hidden.shape) if share else None
        gx, gh, gw, gb, groot, gbias = ops.nnconv_backward_hidden_raw(
            x, ctx.csr, hidden, ctx.dims, w_last, b_last, root, ctx.aggr, grad_out,
            need_root=root is not None, need_bias=ctx.has_bias, z_saved=ctx.z, grad_hidden_acc=None if acc is None else acc[0])
        ctx.z = None
        if acc is not None:
            gh = None                       # added in place to the tensor the first application returned
            tok.added()
            ops.n_grad_hidden_accumulated += 1
        elif share:
            tok.start(gh)
        return (gx, gh, None, None, gw, gb, groot, gbias if ctx.has_bias else None, None, None, None)


class DeferredToken:
    """Shared by the virtual-H node and the applications hanging on it: the (input, output gradient) pairs the light
    backward passes leave for the deferred pass, and the validity flag of the cached virtual H (as HiddenToken)."""
    __slots__ = ("valid", "stash", "hpart", "serial")

    def __init__(self):
        self.valid = True
        # application serial -> (x, grad_out), in the order the light passes ran.  Keyed, not appended: an application whose
        # backward runs twice before the deferred pass (torch.autograd.grad(out, x, retain_graph=True), then loss.backward())
        # contributes its LAST output gradient once; and `drop_stale` empties it when a new forward finds pairs a finished
        # backward left behind (a pass abandoned by an exception, or one that asked for input gradients only - the virtual
        # node's backward, the only consumer, never ran: ADVICE r4)
        self.stash = {}
        self.serial = 0
        self.hpart = None       # (H rows of the in-edges of nodes [0, hn), max |H| scalar, hn): the cache's partial H, or None.
                                # Read at call time and droppable at any moment (hidden_cache.release_all): without it
                                # everything is recomputed - same mathematics

    def drop_stale(self) -> int:
        """Called at FORWARD time (hidden_cache.lookup_deferred, NNConvDeferredFunction.forward): pairs on the stash now belong
        to a backward pass whose deferred step never ran.  Returns how many were dropped."""
        n = len(self.stash)
        if n:
            self.stash = {}
        return n


class DeferredHiddenFunction(torch.autograd.Function):
    """The "virtual H" of a module whose hidden activations do not fit memory: a one-element tensor standing for
    H(edge_attr; hidden layers).  Its backward - run by autograd after every application's backward - is ONE
    gpde_nnconv_bwd_deferred pass over the edges for all applications."""

    @staticmethod
    def forward(ctx, edge_attr, csr, aggr, token, n_layers, *params):
        ctx.csr, ctx.aggr, ctx.token, ctx.n_layers = csr, aggr, token, n_layers
        ctx.attr_needs_grad = edge_attr.requires_grad
        ctx.save_for_backward(_save_attr(ctx, edge_attr), *params)
        return torch.zeros(1, dtype=torch.float32, device=edge_attr.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_virtual):
        if ctx.attr_needs_grad:
            raise NotImplementedError(
                "gradient with respect to edge_attr is not built (no reference script needs it)")
        token = ctx.token
        token.valid = False
        stash, token.stash = list(token.stash.values()), {}
        hp, token.hpart = token.hpart, None       # the cache builds its next partial H before this token is replaced
        edge_attr, *params = ctx.saved_tensors
        edge_attr = _saved_attr(ctx, edge_attr)
        n = ctx.n_layers
        weights, biases = list(params[:n]), list(params[n:])
        if not stash:                   # no application took part in this backward: the hidden layers get zero
            gW = [torch.zeros_like(w) for w in weights[:-1]]
            gb = [None if b is None else torch.zeros_like(b) for b in biases[:-1]]
        else:
            gW, gb = ops.nnconv_backward_deferred_raw([s[0] for s in stash], [s[1] for s in stash], ctx.csr, edge_attr,
                                                      weights, biases, ctx.aggr, hidden_part=None if hp is None else hp[0],
                                                      hidden_nodes=0 if hp is None else hp[2])
        return (None, None, None, None, None, *gW, None, *gb, None)


class NNConvDeferredFunction(torch.autograd.Function):
    """One application of a depth-shared module whose hidden layers are differentiated by the shared virtual-H node:
    forward = gpde_nnconv_fwd (as NNConvFunction), backward = gpde_nnconv_bwd_light."""

    @staticmethod
    def forward(ctx, x, virtual_h, csr, edge_attr, root, bias, aggr, token, n_layers, *params):
        # params: the Linear layers' weights then biases (the module's own tensors: the pack cache recognises them).  This
        # node returns a gradient for the LAST Linear only; the hidden layers' flows through virtual_h.
        weights = list(params[:n_layers])
        biases = list(params[n_layers:])
        ops._require_cuda(x, "x")
        pm = ops.pack_mlp(weights, biases)
        hp = token.hpart
        ctx.z = ops.z_buffer(csr, pm.dims, x.device) if aggr in ("add", "mean") else None
        if hp is not None:          # the in-edges of the leading nodes from the kept partial H, the rest through the fused kernel
            out = ops.nnconv_forward_mixed_raw(x.detach(), csr, edge_attr.detach(), hp[0], hp[1], hp[2], pm, root, bias, aggr,
                                               z_keep=ctx.z)
        else:
            out = ops.nnconv_forward_raw(x.detach(), csr, edge_attr.detach(), pm, root, bias, aggr, z_keep=ctx.z)
        ctx.csr, ctx.aggr, ctx.n_layers, ctx.token = csr, aggr, n_layers, token
        if token.valid and not in_backward_pass():
            token.drop_stale()
        token.serial += 1
        ctx.serial = token.serial
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, _save_attr(ctx, edge_attr), root, *params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, edge_attr, root, *params = ctx.saved_tensors
        edge_attr = _saved_attr(ctx, edge_attr)
        n = ctx.n_layers
        weights, biases = list(params[:n]), list(params[n:])
        hp = ctx.token.hpart
        gx, gw, gb, groot, gbias = ops.nnconv_backward_light_raw(
            x, ctx.csr, edge_attr, weights, biases, root, ctx.aggr, grad_out,
            need_root=root is not None, need_bias=ctx.has_bias, z_saved=ctx.z,
            hidden_part=None if hp is None else hp[0], hidden_nodes=0 if hp is None else hp[2])
        ctx.z = None
        ctx.token.stash[ctx.serial] = (x, grad_out.detach().contiguous())
        gv = torch.zeros(1, dtype=torch.float32, device=x.device)        # the virtual H carries no numbers, only the dependency
        return (gx, gv, None, None, groot, gbias if ctx.has_bias else None, None, None, None,
                *([None] * (n - 1)), gw, *([None] * (n - 1)), gb)


class EdgeWeightsFunction(torch.autograd.Function):
    """W_e [E, 4096] = view(nn(pseudo_e), 64, 64) flattened (nn_conv.py:274) from the hidden activations
    (gpde_edge_weights_fwd) as an autograd node: the `depth` applications of a module share it, autograd sums their dL/dW_e and
    the backward below runs the two 4096 x k2 products per edge ONCE per step (gpde_edge_weights_bwd)."""

    @staticmethod
    def forward(ctx, hidden, pm, w_last, b_last, token):
        we = ops.edge_weights_raw(hidden.detach(), pm, w_last, b_last)
        ctx.dims, ctx.token, ctx.has_b = tuple(pm.dims), token, b_last is not None
        ctx.save_for_backward(hidden, w_last)
        return we

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_we):
        tok = ctx.token
        tok.valid = False
        tok.taken(grad_we, "graph_pde_amd: the in-place sum of dL/dW_e lost its buffer (W_e has a consumer outside WeConvFunction); "
                           "set GPDE_ACCUMULATE_DLDH=0")
        hidden, w_last = ctx.saved_tensors
        gh, gw, gb = ops.edge_weights_backward_raw(grad_we, hidden, ctx.dims, w_last, need_b=ctx.has_b)
        return gh, None, gw, gb, None


class SharedParamFunction(torch.autograd.Function):
    """Identity on a parameter (root / bias) of a module whose applications share W_e: a PRIVATE autograd node between the leaf
    and the WeConvFunction calls of one step.  The in-place sum of the applications' gradients (WeConvFunction.backward) needs a
    tensor that nothing else contributes to - a leaf's gradient buffer also collects whatever else the user's loss does with the
    parameter, and an out-of-place sum there would silently drop the later in-place additions.  Here the only consumers are
    ours, and the backward checks that what arrives IS the tensor the applications added to."""

    @staticmethod
    def forward(ctx, p, token, which):
        ctx.token, ctx.which = token, which
        return p.view_as(p)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        # (checked, not dropped: the W_e node's backward - before or after this one - drops, after its own check)
        ctx.token.check(g, "graph_pde_amd: the in-place sum of a root / bias gradient lost its buffer; set GPDE_ACCUMULATE_DLDH=0", ctx.which)
        return g, None, None


class WeConvFunction(torch.autograd.Function):
    """The operator given the per-edge weights (gpde_nnconv_fwd_edgeweights_group: gather, message, add / mean, update in one
    streaming kernel), differentiable in x, W_e, root and bias (gpde_nnconv_bwd_edgeweights)."""

    @staticmethod
    def forward(ctx, x, we, csr, root, bias, aggr, token=None):
        out = ops.nnconv_forward_edgeweights_raw(x.detach(), csr, we.detach(), root, bias, aggr)
        ctx.csr, ctx.aggr, ctx.has_bias = csr, aggr, bias is not None
        ctx.token = token           # the HiddenToken of the shared W_e node (None: W_e is the caller's own tensor)
        ctx.save_for_backward(x, we, root)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, we, root = ctx.saved_tensors
        # The applications of a module that share W_e each produce dL/dW_e [E, 4096] (and grad_root, grad_bias of the same
        # parameters); autograd would keep the first and add the others with one elementwise kernel per application and tensor
        # (MGKN training steps: 190 - 220 such launches, 2.3 - 2.6 ms of a 20 - 28 ms step).  As NNConvHiddenFunction does for
        # dL/dH: the first application of a backward pass hands autograd its tensors and remembers them on the W_e token, the
        # and return nothing (the transitions: HiddenToken).
        tok, needs = ctx.token, ctx.needs_input_grad
        share = tok is not None and tok.side_in is not None and ACCUMULATE_GRAD_HIDDEN and needs[1] and \
            (root is None or needs[3]) and (not ctx.has_bias or needs[4])
        acc = tok.find(we.shape) if share else None
        gx, gwe, groot, gbias = ops.nnconv_backward_edgeweights_raw(x, ctx.csr, we, root, ctx.aggr, grad_out,
                                                                    need_root=root is not None, need_bias=ctx.has_bias, acc=acc)
        if acc is not None:
            tok.added()
            ops.n_grad_hidden_accumulated += 1
            return gx, None, None, None, None, None, None
        if share:
            tok.start(gwe, groot, gbias)
        return gx, gwe, None, groot, gbias if ctx.has_bias else None, None, None


def _root_term(x_dst, root):
    """PyG: `if x_r is not None and root_weight: out += lin(x_r)` - a call without destination features has no root term."""
    return None if x_dst is None else root


class WeConvAnyFunction(torch.autograd.Function):
    """The operator given the per-edge weights at ANY width 1 .. 256 (gpde_nnconv_fwd_edgeweights_any / _bip: gather, message, add /
    mean, update in one streaming kernel), differentiable in x_src, x_dst, W_e [E, in_src * out], root [in_dst, out] and bias
    (gpde_nnconv_bwd_edgeweights_any / _bip).  x_src [n_src, in_src] is gathered along the edges of `csr`, x_dst [n_dst, in_dst]
    enters `x_dst . root`, out is [n_dst, out].  `x_dst` None: no root term.  `x_dst` ops._ONE_SET: ONE node set - x_src is the table
    of the root term too, through the `_any` entry points (whose grad_x holds both terms in one ordered sum; the same tensor in both
    slots would have autograd add two partial gradients, with other bits).  The sibling of WeConvFunction for modules whose widths
    are not (64, 64): W_e is the caller's own tensor (`nn(pseudo)`), nothing is shared between applications."""

    @staticmethod
    def forward(ctx, x_src, x_dst, we, csr, root, bias, aggr):
        root = _root_term(x_dst, root)
        ctx.one, ctx.has_dst = x_dst is ops._ONE_SET, torch.is_tensor(x_dst)
        if ctx.one:
            out = ops.nnconv_forward_edgeweights_any_raw(x_src.detach(), csr, we.detach(), root, bias, aggr)
        else:
            out = ops.nnconv_forward_edgeweights_bip_raw(x_src.detach(), x_dst.detach() if ctx.has_dst else None, csr, we.detach(), root, bias, aggr)
        ctx.csr, ctx.aggr, ctx.has_bias, ctx.has_root = csr, aggr, bias is not None, root is not None
        ctx.save_for_backward(x_src, x_dst if ctx.has_dst else None, we, root)
        return out

    @staticmethod
    @once_differentiable        # the native backward is not itself differentiable: create_graph=True raises
    def backward(ctx, grad_out):
        x_src, x_dst, we, root = ctx.saved_tensors
        need = ctx.needs_input_grad
        kw = dict(need_root=ctx.has_root and need[4], need_bias=ctx.has_bias and need[5])
        if ctx.one:         # (this entry point always writes grad_x; no x_dst input, no gradient in its slot)
            gxd = None
            gxs, gwe, groot, gbias = ops.nnconv_backward_edgeweights_any_raw(x_src, ctx.csr, we, root, ctx.aggr, grad_out, **kw)
        else:
            gxs, gxd, gwe, groot, gbias = ops.nnconv_backward_edgeweights_bip_raw(
                x_src, x_dst, ctx.csr, we, root, ctx.aggr, grad_out, need_x_src=need[0], need_x_dst=ctx.has_dst and need[1], **kw)
        return gxs, gxd, (gwe if need[2] else None), None, groot, gbias, None


class HiddenAnyFunction(torch.autograd.Function):
    """The RE-ASSOCIATED operator at any width 1 .. 256 (gpde_nnconv_fwd_hidden_any / _bip: aggregation of x_j (x) h_e per
    destination, the last Linear per destination, update()), differentiable in x_src, x_dst, the last hidden activations H [E, K],
    the last Linear (w_last [in_src * out, K], b_last [in_src * out]), root [in_dst, out] and bias (gpde_nnconv_bwd_hidden_any /
    _bip).  `x_dst`: as WeConvAnyFunction takes it.  H is the caller's own tensor - relu(L_{n-1}(...)) evaluated by torch, rows in
    CSR slot order -, so dL/dH flows on through the caller's earlier layers by ordinary autograd; [E, in * out] is never formed."""

    @staticmethod
    def forward(ctx, x_src, x_dst, hidden, w_last, b_last, csr, root, bias, aggr):
        root = _root_term(x_dst, root)
        ctx.one, ctx.has_dst = x_dst is ops._ONE_SET, torch.is_tensor(x_dst)
        if ctx.one:
            out = ops.nnconv_forward_hidden_any_raw(x_src.detach(), csr, hidden.detach(), w_last, b_last, root, bias, aggr)
        else:
            out = ops.nnconv_forward_hidden_bip_raw(x_src.detach(), x_dst.detach() if ctx.has_dst else None, csr, hidden.detach(), w_last, b_last,
                                                    root, bias, aggr)
        ctx.csr, ctx.aggr, ctx.has_bias = csr, aggr, bias is not None
        ctx.has_b_last, ctx.has_root = b_last is not None, root is not None
        ctx.save_for_backward(x_src, x_dst if ctx.has_dst else None, hidden, w_last, b_last, root)
        return out

    @staticmethod
    @once_differentiable        # the native backward is not itself differentiable: create_graph=True raises
    def backward(ctx, grad_out):
        x_src, x_dst, hidden, w_last, b_last, root = ctx.saved_tensors
        need = ctx.needs_input_grad
        kw = dict(need_w_last=need[3], need_b_last=ctx.has_b_last and need[4], need_root=ctx.has_root and need[6],
                  need_bias=ctx.has_bias and need[7])
        if ctx.one:         # (no x_dst input, no gradient in its slot)
            gxd = None
            gxs, gh, gwl, gbl, groot, gbias = ops.nnconv_backward_hidden_any_raw(x_src, ctx.csr, hidden, w_last, b_last, root, ctx.aggr, grad_out,
                                                                                 need_x=need[0], **kw)
        else:
            gxs, gxd, gh, gwl, gbl, groot, gbias = ops.nnconv_backward_hidden_bip_raw(
                x_src, x_dst, ctx.csr, hidden, w_last, b_last, root, ctx.aggr, grad_out, need_x_src=need[0],
                need_x_dst=ctx.has_dst and need[1], **kw)
        return gxs, gxd, (gh if need[2] else None), gwl, gbl, None, groot, gbias, None


class ChainAnyFunction(torch.autograd.Function):
    """The STREAMED any-width operator (gpde_nnconv_fwd_chain_any / gpde_nnconv_bwd_chain_any): from the edge attributes and the
    weights of a Linear / ReLU chain, the hidden rows generated by block of destination nodes - neither [E, K] nor [E, in * out]
    is formed, in either direction.  Differentiable in x_src, x_dst, edge_attr, root, bias and every weight and bias of the chain.
    `x_dst`: as WeConvAnyFunction takes it.  `edge_attr` [E, k0] comes in the CALLER's edge order and its gradient goes back in
    that order.  Only the inputs are saved: the backward recomputes every activation block by block.
    `acts`: None (a Linear / ReLU chain) or one (kind, p0, p1) per hidden layer (ops.mlp_chain: gpde_nnconv_*_chain_act), not a tensor.
    `params`: the chain's weights, then its biases (None for a Linear without one)."""

    @staticmethod
    def forward(ctx, x_src, x_dst, edge_attr, csr, root, bias, aggr, acts, *params):
        root = _root_term(x_dst, root)
        nl = len(params) // 2
        ctx.one, ctx.has_dst, ctx.nl = x_dst is ops._ONE_SET, torch.is_tensor(x_dst), nl
        ctx.identity = bool(getattr(csr, "_perm_is_identity", False))
        ea = edge_attr.detach().float().contiguous()
        ea_s = ea if ctx.identity or csr.n_edges == 0 else ops.gather_rows(ea, csr.perm)
        xd = ops._ONE_SET if ctx.one else x_dst.detach() if ctx.has_dst else None
        out = ops.nnconv_forward_chain_any_raw(x_src.detach(), xd, csr, ea_s, params[:nl], params[nl:], root, bias, aggr, acts=acts)
        ctx.csr, ctx.aggr, ctx.has_bias, ctx.has_root, ctx.acts = csr, aggr, bias is not None, root is not None, acts
        ctx.save_for_backward(x_src, x_dst if ctx.has_dst else None, edge_attr, root, *params)
        return out

    @staticmethod
    @once_differentiable        # the native backward is not itself differentiable: create_graph=True raises
    def backward(ctx, grad_out):
        x_src, x_dst, edge_attr, root, *params = ctx.saved_tensors
        need, nl, csr = ctx.needs_input_grad, ctx.nl, ctx.csr
        ea = edge_attr.detach().float().contiguous()
        ea_s = ea if ctx.identity or csr.n_edges == 0 else ops.gather_rows(ea, csr.perm)
        xd = ops._ONE_SET if ctx.one else x_dst if ctx.has_dst else None
        gxs, gxd, gea, gw, gb, groot, gbias = ops.nnconv_backward_chain_any_raw(
            x_src, xd, csr, ea_s, params[:nl], params[nl:], root, ctx.aggr, grad_out, need_x_src=need[0], need_x_dst=ctx.has_dst and need[1],
            need_w=list(need[8:8 + nl]), need_b=[params[nl + l] is not None and need[8 + nl + l] for l in range(nl)],
            need_root=ctx.has_root and need[4], need_bias=ctx.has_bias and need[5], need_edge_attr=need[2], acts=ctx.acts)
        if gea is not None and not ctx.identity:            # slot order -> the caller's edge order (an edge the CSR dropped: 0)
            gea = torch.zeros(edge_attr.shape, dtype=gea.dtype, device=gea.device).index_copy_(0, csr.perm.long(), gea)
        if gea is not None:
            gea = gea.to(edge_attr.dtype)
        return (gxs, gxd, gea, None, groot, gbias, None, None, *gw, *gb)


class GCNFunction(torch.autograd.Function):
    """GCNConv: out = (A x) W + bias, A = the normalised adjacency of an `ops.GcnNorm` (gpde_gcn_fwd), differentiable in x, W and
    bias.  With G = A^T grad_out (one launch of the aggregation kernel on the reversed graph): grad_x = G W^T, grad_W = x^T G
    (torch.mm), grad_bias = grad_out.sum(0).  Under the forced route 'aggregate_first' the SAME launch also multiplies by W^T -
    the fused kernel with `agg_out` = G leaves grad_x and G together; it is not the default because the fused kernel measured
    slower than aggregation + torch.mm (ops.gcn_route).  Only x and W are saved (no activation besides the input); the kernel is
    skipped when neither x nor W needs a gradient.  No atomics anywhere: two backward passes give the same bits."""

    @staticmethod
    def forward(ctx, x, weight, bias, norm, route):
        out = ops.gcn_forward_raw(x.detach(), norm, weight.detach(), None if bias is None else bias.detach(), route=route)
        ctx.norm, ctx.has_bias, ctx.fused = norm, bias is not None, route == "aggregate_first"
        ctx.save_for_backward(x, weight)
        return out

    @staticmethod
    @once_differentiable        # the native backward is not itself differentiable: create_graph=True raises
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx = gw = gb = None
        if need[0] and ctx.fused:
            # (weight.t() is a strided view: the operand gate hands the kernel a dense copy of W^T)
            gx, g_agg = ops.gcn_forward_raw(grad_out, ctx.norm, weight.detach().t(), None, route="aggregate_first", agg_out=True, reverse=True)
        elif need[0] or need[1]:
            g_agg = ops.gcn_forward_raw(grad_out, ctx.norm, None, None, reverse=True)
            if need[0]:
                gx = torch.mm(g_agg, weight.detach().t())
        if need[1]:
            gw = torch.mm(x.detach().t(), g_agg)
        if ctx.has_bias and need[2]:
            gb = grad_out.sum(0)
        return gx, gw, gb, None, None


class DiagConvFunction(torch.autograd.Function):
    """The DIAGONAL-kernel operator (gpde_diagconv_fwd: gather, x_j (.) k_e, add / mean, update() in one streaming kernel),
    differentiable in x_src, x_dst, the per-edge kernel k [E, w] (CSR slot order), root [in_dst, w] and bias (gpde_diagconv_bwd).
    `x_dst`: as WeConvAnyFunction takes it - a tensor, None (no root term) or ops._ONE_SET (one node set: grad_x_src then holds the
    source sum and g . root^T, added in the library).  k is the caller's own tensor (`nn(pseudo)`, a Gaussian, ...): dL/dk flows
    on into whatever produced it by ordinary autograd."""

    @staticmethod
    def forward(ctx, x_src, x_dst, k, csr, root, bias, aggr):
        root = _root_term(x_dst, root)
        ctx.one, ctx.has_dst = x_dst is ops._ONE_SET, torch.is_tensor(x_dst)
        xd = x_dst.detach() if ctx.has_dst else x_dst
        out = ops.diagconv_forward_raw(x_src.detach(), xd, csr, k.detach(), root, bias, aggr)
        ctx.csr, ctx.aggr, ctx.has_bias, ctx.has_root = csr, aggr, bias is not None, root is not None
        ctx.save_for_backward(x_src, x_dst if ctx.has_dst else None, k, root)
        return out

    @staticmethod
    @once_differentiable        # the native backward is not itself differentiable: create_graph=True raises
    def backward(ctx, grad_out):
        x_src, x_dst, k, root = ctx.saved_tensors
        need = ctx.needs_input_grad
        gxs, gxd, gk, groot, gbias = ops.diagconv_backward_raw(
            x_src, ops._ONE_SET if ctx.one else x_dst, ctx.csr, k, root, ctx.aggr, grad_out, need_x_src=need[0],
            need_x_dst=ctx.has_dst and need[1], need_root=ctx.has_root and need[4], need_bias=ctx.has_bias and need[5])
        return gxs, gxd, (gk if need[2] else None), None, groot, gbias, None
