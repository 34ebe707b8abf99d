"""Cross-depth reuse of the kernel-MLP hidden activations.

The reference applies one NNConv module `depth` times per forward with the same `edge_attr` and
the same weights (/root/reference/graph-neural-operator/UAI1_full_resolution.py:29-30; the MGKN
V-cycle, multipole-graph-neural-operator/MGKN_general_darcy2d.py:76-90), so
H = relu(L_{n-1}(... relu(L_1(edge_attr)))) -- 94 % of the operator's FLOPs at [6,1024,1024,4096] -- is
the same tensor in every one of those calls.  This module decides, per NNConv instance, when to
materialise H (one `HiddenFunction` node) and serve the remaining calls from it
(`NNConvHiddenFunction`): the hidden layer and its backward then run once per step.

Policy (`GPDE_HIDDEN_CACHE` = auto | on | off, default auto; budget `GPDE_HIDDEN_CACHE_GB`, default: sized to the device -
70 % of its HBM, at most what is free now minus a 48 GB reserve for workspaces, i.e. ~200 GB on an idle 288 GB MI355X):
  * a call whose (edge_attr memory + version, CSR, hidden-layer parameter versions, precision, grad
    mode) matches the cached H is a hit;
  * "auto" materialises H only for a module that has been SEEN repeating a key (the second call of
    the first forward, then the first call of every later forward); a module that stops repeating
    goes back to the direct fused path.  "on" always materialises, "off" never does;
  * H is E x K2P x 4 bytes; larger than the budget -> direct path, or, for inference
    (`GPDE_HIDDEN_CACHE_PARTIAL`, default on), a PARTIAL H: the in-edges of the first `hn` nodes that fit
    the budget are cached and served by the mixed forward (gpde_nnconv_fwd_mixed_keepz), the other nodes run
    the fused kernel.  G241 at k2 = 1024 needs 391 GB for the full H.
The entry holds `edge_attr` (so its memory cannot be recycled for other data while the key is
alive) and is invalidated when the backward of its H node has run.  Nothing is stored on the
module itself: modules pickle as before.
"""
from __future__ import annotations

import os
import weakref
from typing import List, Optional

import torch

from . import autograd as _ag
from . import ops
from .autograd import DeferredHiddenFunction, DeferredToken, EdgeWeightsFunction, HiddenFunction, HiddenToken, in_backward_pass

MODE = os.environ.get("GPDE_HIDDEN_CACHE", "auto")
_env_gb = os.environ.get("GPDE_HIDDEN_CACHE_GB", "")
# None = sized to the device at the moment H is built (budget_bytes); a number pins it (tests / A-B runs set this variable)
BUDGET_BYTES: Optional[int] = None if _env_gb in ("", "auto") else int(float(_env_gb) * (1 << 30))
AUTO_FRACTION = 0.7                  # of the device's HBM.  Round 6 tried 0.8 on the 241^2 training step (30 GiB more of H instead of two kept Z:
                                     # 7.02 -> 6.79 s pinned, 6.95 s under this policy) - and the distinct-samples step ran out of memory
                                     # on its 26.9 GiB workspace with 15.7 GiB free: left at 0.7 (profiles/r06_g241_memory_budget.txt)
AUTO_RESERVE_BYTES = 48 << 30        # left free for workspaces (Z of the 241^2 graph: 15 GB), the caller's tensors, RCCL


def budget_bytes(device=None, releasing: int = 0) -> int:
    """Bytes the hidden activations of ONE module may take.  With GPDE_HIDDEN_CACHE_GB unset the budget follows the
    device: min(70 % of its memory, free now + `releasing` (the H about to be dropped) - reserve).  On the 241^2 graph
    (H = 391 GB) that caches the in-edges of ~44 % of the nodes instead of none, 1.64 x on a depth-6 inference forward
    (scripts/time_g241_depth6_reuse.py)."""
    if BUDGET_BYTES is not None:
        return BUDGET_BYTES
    dev = None if device is None else torch.device(device)
    if dev is None or dev.type != "cuda":
        return 32 << 30
    free, total = ops.device_free_bytes(dev)
    return max(0, min(int(AUTO_FRACTION * total), free + releasing - AUTO_RESERVE_BYTES))
PARTIAL = os.environ.get("GPDE_HIDDEN_CACHE_PARTIAL", "1") != "0"
# Depth-deferred backward: a module that repeats (edge_attr, weights) within a forward, needs gradients and
# whose H does NOT fit the budget shares one "virtual H" autograd node - its applications run the light backward and ONE
# deferred pass differentiates the hidden layers for all of them (autograd.DeferredHiddenFunction).  auto | off.
DEFER_MODE = os.environ.get("GPDE_DEFERRED_BWD", "auto")
# Per-edge weight cache: for calls on low in-degree / small graphs the whole
# W_e = view(nn(edge_attr_e), 64, 64) tensor is kept ([E, 4096] fp32 = 16 KiB per edge) and a call is one streaming
# kernel; with gradients W_e is an autograd node shared by the module's applications (autograd.EdgeWeightsFunction /
# WeConvFunction: the MGKN scripts TRAIN, MGKN_general_darcy2d.py:260-282).  Its summation order differs from the fused
# kernels' (same accuracy, other last bits) - like the hidden-activation cache it makes a module's output depend on its call
# history at the 1e-7 level; GPDE_HIDDEN_CACHE=off (which also disables this cache: W_e derives from H) gives
# history-independent bits.  Used by (a) nn_conv.nnconv_group - the explicit grouped API, from the first call;
# (b) aggr='max', which has no other path; (c) plain module calls of a module SEEN repeating (edge_attr, weights):
# GPDE_EDGE_WEIGHT_CACHE=auto, the default since round 4 (rounds 1-3: off); "off" keeps (a) and (b) only.
# Budget per module: GPDE_EDGE_WEIGHT_CACHE_GB (default 4).
WE_MODE = os.environ.get("GPDE_EDGE_WEIGHT_CACHE", "auto")
WE_BUDGET_BYTES = int(float(os.environ.get("GPDE_EDGE_WEIGHT_CACHE_GB", "4")) * (1 << 30))
WE_SMALL_EDGES = 8192          # calls up to this many edges qualify whatever their in-degree

stats = {"hits": 0, "builds": 0, "direct": 0, "we_hits": 0, "we_builds": 0}       # counters for tests / bench


def _param_refs(params) -> tuple:
    """Weak references to the parameter objects a key was built from, kept next to the key (as ops.pack_mlp does).  A key names a
    parameter by (data_ptr, version); a NEW tensor object - `conv.nn = new_mlp.to(dev)`, the device copy ops.stage_const makes
    again after its cache evicted the last one - starts at version 0 and often at the address the old one just freed.  A live
    object keeps its address, a dead one fails `_same_params`: equal keys then really mean the same parameters."""
    return tuple(None if p is None else weakref.ref(p) for p in params)


def _same_params(refs, params) -> bool:
    return refs is not None and len(refs) == len(params) and \
        all((p is None) if r is None else (r() is p) for r, p in zip(refs, params))


class _Slot(ops.Cached):
    """One cached value of a module: the record with the `key` it was built for, `refs` - weak references to the parameter OBJECTS
    the key names (_param_refs) - and the validity `token` its autograd node clears (None where the value has none)."""
    __slots__ = ("key", "refs", "token")

    def __init__(self):
        super().__init__()
        self.key = self.refs = self.token = None

    def holds(self, key, params) -> bool:        # is the value still the one for this call?
        return self.value is not None and self.key == key and (self.token is None or self.token.valid) and \
            _same_params(self.refs, params)

    def store(self, value, key, params, pins, token=None, extra_buffers=()):
        self.value, self.key, self.refs, self.token = value, key, _param_refs(params), token
        self.buffers, self.pins = (value,) + tuple(extra_buffers), tuple(pins)
        self.stamp(value.device)

    def clear(self):
        self.__init__()


def _field(slot: str, attr: str):
    return property(lambda ent: getattr(getattr(ent, slot), attr))


class _Entry:
    __slots__ = ("h", "hn", "w", "tw", "d", "dcount", "last_key", "repeats", "hits_on_hidden", "big_key", "last_partial")
    # READ-ONLY views under the names the slots' fields had on the entry itself: the benchmark (hidden, hn) and the call-history
    # tests read them.  Nothing is written through them - a value enters a slot through `store` alone.
    hidden, token, we, dvirtual = _field("h", "value"), _field("h", "token"), _field("w", "value"), _field("d", "value")
    twe, twe_token, dtoken = _field("tw", "value"), _field("tw", "token"), _field("d", "token")
    csr = property(lambda ent: ent.h.pins[1] if ent.h.pins else None)

    def __init__(self):
        # h: H, pins (edge_attr, csr), its token's hmax is a buffer too; w: per-edge weights [E, 4096] (inference), pins (edge_attr, csr);
        # tw: training, W_e as an autograd node shared by the applications of a step, pin: the H it was built from;
        # d: depth-deferred backward, the current virtual H, pins (edge_attr, csr)
        self.h, self.w, self.tw, self.d = _Slot(), _Slot(), _Slot(), _Slot()
        # hn: nodes whose in-edges the cached H covers (all of them unless partial); dcount: applications hanging on the virtual H
        self.hn, self.dcount = 0, 0
        # policy state - what was learnt about the module: last_key; repeats: it has been seen repeating a key; hits_on_hidden; big_key:
        # key of the last call whose H was wanted but exceeded the budget; last_partial: (n_edges, hn) of the last PARTIAL H built - the
        # next build keeps that size while it still fits (see lookup)
        self.last_key = self.big_key = self.last_partial = None
        self.repeats, self.hits_on_hidden = False, 0


_entries: "weakref.WeakKeyDictionary[torch.nn.Module, _Entry]" = weakref.WeakKeyDictionary()


def clear():
    _entries.clear()
    for k in stats:
        stats[k] = 0


def release_all() -> bool:
    """Drop every cached H / W_e tensor (the entries and what they learnt about their modules stay): called by
    ops._alloc_ws when a workspace does not fit.  Returns whether anything was released."""
    freed = False
    for ent in list(_entries.values()):
        freed = freed or ent.h.value is not None or ent.w.value is not None
        if ent.h.token is not None:
            ent.h.token.drop()
        # On purpose: the virtual-H node `d` stays (it owns no H of its own, only `hpart`), and no policy state is reset
        for slot in (ent.h, ent.w, ent.tw):        # (nodes of a live graph keep their own references)
            slot.clear()
        if ent.d.token is not None:
            ent.d.token.hpart = None         # applications still hanging on the virtual H recompute instead (same mathematics)
    if freed:
        stats["released"] = stats.get("released", 0) + 1
    return freed


def snapshot() -> list:
    """Strong references to every tensor the entries hold right now (capture.py: a recorded graph reads H / W_e / the virtual
    node's partial H at the addresses they had at recording time; `clear()`, `release_all()` and rebuilt entries must not free
    them under it - ADVICE r5)."""
    pins = []
    for ent in list(_entries.values()):
        pins.extend(slot.held() for slot in (ent.h, ent.w, ent.tw, ent.d))
        pins.append(None if ent.d.token is None else ent.d.token.hpart)
    return pins


def _pkey(p: Optional[torch.Tensor]) -> tuple:
    return (0, 0) if p is None else (p.data_ptr(), ops._ver(p))


def _key(edge_attr, csr, hidden_params: List[Optional[torch.Tensor]], precision: str):
    node = isinstance(edge_attr, ops.NodeAttr)   # attributes described by node data: keyed on the table's memory + version + slots
    t = edge_attr.table if node else edge_attr
    ops.watch(t, *hidden_params)
    grad = torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in hidden_params)
    return (str(t.device),) + ops.mem_key(t) + ((tuple(edge_attr.sel),) if node else ()) + \
        (id(csr), tuple(_pkey(p) for p in hidden_params), precision, grad)


def lookup(module: torch.nn.Module, edge_attr: torch.Tensor, csr, pm, weights, biases,
           precision: Optional[str] = None, mode: Optional[str] = None, allow_partial: bool = False):
    """Returns (H, hmax, hn) for this call (cached or freshly built; hmax = device scalar max |H| or None;
    hn = number of leading nodes whose in-edges H covers, = N unless partial), or None when the direct
    fused path should run.  `allow_partial`: the caller needs no gradient at all."""
    mode = MODE if mode is None else mode
    if mode == "off":
        stats["direct"] += 1
        return None
    if torch.is_grad_enabled() and _ag.saved_tensor_hooks_active():
        # a checkpointed segment (forward or recomputation): a shared node built here would save that segment's placeholders and
        # poison every later step that hangs on it, and a segment must take the same route both times whatever the cache holds
        # by then - it takes the direct operator and leaves the entry alone
        stats["direct"] += 1
        stats["hooked_direct"] = stats.get("hooked_direct", 0) + 1
        return None
    precision = ops.DEFAULT_PRECISION if precision is None else precision
    hw, hb = list(weights[:-1]), list(biases[:-1])
    key = _key(edge_attr, csr, hw + hb, precision)
    ent = _entries.get(module)
    if ent is None:
        ent = _entries[module] = _Entry()
    h = ent.h
    if h.holds(key, hw + hb):
        ent.hits_on_hidden += 1
        # a backward pass that never reached the H node (input gradients only, an exception) left its running dL/dH sum on the
        # token: [E, K2P], 24 GB at s=121.  Dropped at forward time - unless this forward runs INSIDE a backward pass
        # (a checkpointed segment recomputing): the sum then belongs to the pass in flight
        if not in_backward_pass():
            h.token.drop()
        if ent.hn == csr.n_nodes or allow_partial:
            stats["hits"] += 1
            if ent.hn < csr.n_nodes:
                ent.big_key = key
            h.hit("hidden")
            return h.value, h.token.hmax, ent.hn
    repeated = ent.last_key == key
    if repeated:
        ent.repeats = True
    elif h.value is not None and h.key != key and ent.hits_on_hidden == 0:
        ent.repeats = False          # the last H was built and never reused: stop speculating
    ent.last_key = key
    row_bytes = ops.hidden_width(pm.dims) * 4
    nbytes = csr.n_edges * row_bytes
    want = mode == "on" or (mode == "auto" and ent.repeats)
    hn = csr.n_nodes
    budget = budget_bytes(edge_attr.device, 0 if h.value is None else h.value.numel() * h.value.element_size()) if want else 0
    if want and nbytes > budget and PARTIAL and allow_partial and len(pm.dims) == 4:
        # the leading nodes whose in-edges fit the budget, in whole 64-node tiles; worth it from 1/8 on
        rp = csr.rowptr_host
        hn = int(torch.searchsorted(rp.to(torch.int64), torch.tensor(budget // row_bytes), right=True)) - 1
        hn = hn // 64 * 64
        # Keep the previous build's size while it still fits and is within 10 % of what the budget allows now: the budget follows
        # the free memory of the moment, and a partial H a few MiB LARGER than the last one cannot reuse the block the allocator
        # just got back - on the 241^2 graph a second 230 GiB request that ends in the allocator's out-of-memory retry (round 6,
        # with the budget's free-memory term binding instead of the fixed fraction: every other training step took 14.8 s instead of 6.7)
        lp = ent.last_partial
        if lp is not None and lp[0] == csr.n_edges and lp[1] <= hn and lp[1] >= 0.9 * hn:
            hn = lp[1]
        nbytes = int(rp[hn]) * row_bytes if hn >= csr.n_nodes // 8 and hn > 0 else budget + 1
    if not want or nbytes > budget or csr.n_edges == 0 or edge_attr.requires_grad:
        h.clear()                    # (on purpose: last_partial and repeats stay, big_key is set anew)
        ent.big_key = key if (want and nbytes > budget and csr.n_edges > 0 and not edge_attr.requires_grad) else None
        stats["direct"] += 1
        return None
    token, old = HiddenToken(), h.token
    h.clear()                        # release the previous H before allocating the next one
    if ent.d.token is not None:
        ent.d.token.hpart = None     # ... also where a finished virtual-H node still points at it
    try:
        if hn < csr.n_nodes:         # partial: no autograd node (inference, or training on the virtual-H node: lookup_deferred)
            hidden, token.hmax = ops.hidden_forward_raw(csr, edge_attr.detach(), pm, list(weights[:-1]) + [None],
                                                        list(biases[:-1]) + [None], precision, n_nodes_limit=hn)
        else:
            hidden = HiddenFunction.apply(edge_attr, csr, pm, precision, token, len(hw), *hw, *hb)
    except torch.OutOfMemoryError:
        # the budget was measured a moment ago; another module's cache, another process or the caller's own tensors may have
        # taken the room since.  H is an optimisation: drop everything cached and run the direct path.
        if old is not None:
            old.drop()        # (as release_all does for the token of an H still in its slot)
        release_all()
        torch.cuda.empty_cache()
        stats["oom_fallbacks"] = stats.get("oom_fallbacks", 0) + 1
        stats["direct"] += 1
        return None
    h.store(hidden, key, hw + hb, (edge_attr, csr), token, (token.hmax,))      # (hmax: a device scalar the hidden forward reads)
    ent.hn, ent.hits_on_hidden = hn, 0
    if hn < csr.n_nodes:
        ent.big_key = key            # the whole H does not fit: a training call shares a virtual-H node (lookup_deferred)
        ent.last_partial = (csr.n_edges, hn)
    stats["builds"] += 1
    return hidden, token.hmax, hn


def defer_possible(edge_attr: torch.Tensor, pm, weights, biases, aggr: str) -> bool:
    """A call that needs gradients could hang on a virtual-H node (lookup_deferred): then `lookup` may hand it a PARTIAL H."""
    return DEFER_MODE != "off" and aggr in ("add", "mean") and torch.is_grad_enabled() and not edge_attr.requires_grad and \
        any(p is not None and p.requires_grad for p in list(weights[:-1]) + list(biases[:-1])) and ops.deferred_supported(pm.dims)


def token_of(module: torch.nn.Module, hidden: torch.Tensor, csr=None):
    """The HiddenToken of `hidden` if that is the module's cached full H (the applications sharing it sum their dL/dH on it:
    autograd.NNConvHiddenFunction.backward), else None.  None too for a graph on which the per-edge weight form may run
    (edge_weights_qualify): there W_e's backward is a second kind of consumer of H, and an application can fall from one form to the
    other when memory is short - the in-place sum wants NNConvHiddenFunction to be H's only consumer."""
    ent = _entries.get(module)
    if ent is None or ent.h.value is not hidden or ent.h.token is None or not ent.h.token.valid:
        return None
    if csr is not None and WE_MODE != "off" and edge_weights_qualify(csr, explicit=True):
        return None
    return ent.h.token


def lookup_deferred(module: torch.nn.Module, edge_attr: torch.Tensor, csr, pm, weights, biases, aggr: str,
                    precision: Optional[str] = None, hpart=None):
    """(virtual H tensor, token) for a call that needs gradients, right after `lookup` returned None (or a PARTIAL H: `hpart`
    = its (H, hmax, hn) - the applications then read those rows instead of recomputing them) for it - or None when
    the plain operator (autograd.NNConvFunction: its own full backward) should run.  Deferred when: the module has been seen
    repeating this (edge_attr, weights) key, its H was wanted but does not fit the budget, the hidden layers require a
    gradient and the kernel MLP is in the deferred form (ops.deferred_supported).  All applications of one forward share the
    returned node until its backward has run."""
    if DEFER_MODE == "off" or aggr not in ("add", "mean") or not torch.is_grad_enabled() or not _ag.CAN_TELL_BACKWARD_PASS or \
            _ag.saved_tensor_hooks_active():
        return None         # (a torch that cannot tell a forward inside a backward pass: autograd.in_backward_pass; a checkpointed segment: lookup)
    ent = _entries.get(module)
    if ent is None:
        return None
    precision = ops.DEFAULT_PRECISION if precision is None else precision
    hw, hb = list(weights[:-1]), list(biases[:-1])
    if not any(p is not None and p.requires_grad for p in hw + hb) or edge_attr.requires_grad:
        return None
    key = _key(edge_attr, csr, hw + hb, precision)
    # the virtual node also saved the LAST Linear (its deferred pass forms dL/dH through it): a node built before a write to that
    # layer - by a forward whose backward never ran - must not serve the next step
    w_last, b_last = weights[-1], biases[-1]
    dkey = (key, _pkey(w_last), _pkey(b_last))
    named = hw + hb + [w_last, b_last]
    d = ent.d
    if d.holds(dkey, named):
        ent.dcount += 1
        d.token.hpart = hpart
        # (not from a forward that runs inside a backward pass - a checkpointed segment: the pairs are that pass's own)
        if not in_backward_pass() and d.token.drop_stale():      # a backward over this (still valid) node ended without its deferred pass
            stats["deferred_stale_dropped"] = stats.get("deferred_stale_dropped", 0) + 1
        stats["deferred_hits"] = stats.get("deferred_hits", 0) + 1
        d.hit("deferred")
        return d.value, d.token
    if d.token is not None and ent.dcount <= 1:
        ent.repeats = False             # the last virtual H served a single application: stop speculating
    if d.token is not None:
        d.token.hpart = None
    d.clear()                           # (dcount is read only while the slot holds a token: the next store sets it)
    if not ent.repeats or ent.big_key != key or not ops.deferred_supported(pm.dims):
        return None
    token = DeferredToken()
    token.hpart = hpart
    n = len(weights)
    virtual = DeferredHiddenFunction.apply(edge_attr, csr, aggr, token, n, *hw, w_last.detach(),
                                           *hb, None if b_last is None else b_last.detach())
    d.store(virtual, dkey, named, (edge_attr, csr), token)
    ent.dcount = 1
    stats["deferred_builds"] = stats.get("deferred_builds", 0) + 1
    return virtual, token


def edge_weights_qualify(csr, force: bool = False, explicit: bool = False) -> bool:
    """The per-edge weight form pays where the re-association of DESIGN.md §2 does not: mean in-degree <= 4, or a call
    of at most WE_SMALL_EDGES edges (launch-bound anyway).  `explicit`: the caller opted in (nnconv_group) - WE_MODE is
    not consulted; `force` (aggr='max': no other path) only needs the budget."""
    e, n = csr.n_edges, csr.n_nodes
    if e == 0:
        return False
    if force:
        return e * ops.EDGE_WEIGHT_BYTES <= max(WE_BUDGET_BYTES, budget_bytes(getattr(getattr(csr, "rowptr", None), "device", None)))
    # (plain module calls: only while the hidden-activation cache it derives from is on - GPDE_HIDDEN_CACHE=off is the ONE switch
    # for history-independent bits)
    return (explicit or (WE_MODE == "auto" and MODE != "off")) and (e <= 4 * n or e <= WE_SMALL_EDGES) and \
        e * ops.EDGE_WEIGHT_BYTES <= WE_BUDGET_BYTES


def we_token_of(module: torch.nn.Module, we: torch.Tensor):
    """The token of the module's shared W_e node when `we` is that node (WeConvFunction sums the applications' gradients in place
    on it), else None."""
    ent = _entries.get(module)
    return ent.tw.token if ent is not None and ent.tw.value is we else None


def lookup_edge_weights_train(module: torch.nn.Module, hidden: torch.Tensor, csr, pm, weights, biases):
    """W_e [E, 4096] as an AUTOGRAD node for a call that needs gradients and was just handed the module's full cached H
    (`hidden`: the HiddenFunction output `lookup` returned) - or None when the graph does not qualify / the policy is off.
    All applications of the step share the node (autograd sums their dL/dW_e; EdgeWeightsFunction.backward runs the
    4096 x k2 products once) until its backward has run or H was rebuilt."""
    if WE_MODE != "auto" or not edge_weights_qualify(csr) or not torch.is_grad_enabled():
        return None
    ent = _entries.get(module)
    if ent is None or ent.h.value is not hidden:
        return None
    w_last, b_last = weights[-1], biases[-1]
    key = (id(hidden), _pkey(w_last), _pkey(b_last))       # (the H it was built from: pinned by the slot, so its id names it)
    twe = ent.tw
    if twe.holds(key, [w_last, b_last]):
        stats["we_hits"] += 1
        # (a backward pass that never reached the W_e node left its running sums on the token; a forward inside a backward pass -
        # a checkpointed segment - leaves them alone, as `lookup` does)
        if not in_backward_pass():
            twe.token.drop()
        twe.hit("edge_weights")
        return twe.value
    twe.clear()
    # memory of the training form: W_e, one dL/dW_e per application in flight and autograd's running sum of them - 16 KiB per
    # edge each (the budget bounded W_e only).  When three of them do not fit what is free, the H path runs.
    free, _ = ops.device_free_bytes(hidden.device)
    if 3 * csr.n_edges * 4096 * 4 > free:
        stats["we_train_no_room"] = stats.get("we_train_no_room", 0) + 1
        return None
    token = HiddenToken()
    try:
        we = EdgeWeightsFunction.apply(hidden, pm, w_last, b_last, token)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        stats["oom_fallbacks"] = stats.get("oom_fallbacks", 0) + 1
        return None
    twe.store(we, key, [w_last, b_last], (hidden,), token)
    stats["we_builds"] += 1
    return we


def lookup_edge_weights(module: torch.nn.Module, edge_attr: torch.Tensor, csr, pm, weights, biases,
                        precision: Optional[str] = None, force: bool = False, explicit: bool = False):
    """W_e [E, 4096] for this call, or None when another path should run.  ONLY for calls that need no gradient at
    all.  `force` / `explicit`: built at once (H too).  Otherwise (GPDE_EDGE_WEIGHT_CACHE=auto) it is derived from the
    module's cached hidden activations the first time they are served without gradient - i.e. only for a module that
    has been seen repeating (edge_attr, weights)."""
    if not edge_weights_qualify(csr, force, explicit) or edge_attr.requires_grad:
        return None
    precision = ops.DEFAULT_PRECISION if precision is None else precision
    ent = _entries.get(module)
    w_last, b_last = weights[-1], biases[-1]
    hparams = list(weights[:-1]) + list(biases[:-1])
    key = (_key(edge_attr, csr, hparams, precision)[:-1], _pkey(w_last), _pkey(b_last))
    params = list(weights) + list(biases)
    if ent is not None and ent.w.holds(key, params):
        stats["we_hits"] += 1
        ent.w.hit("edge_weights")
        return ent.w.value
    now = force or explicit
    if not now:
        # peek only: the H policy (who repeats, who gets built) is driven by ONE lookup() per call, made by the caller's
        # ordinary path.  W_e is derived from an H that is already there - i.e. from the call after H was built.
        if ent is None or not ent.h.holds(_key(edge_attr, csr, hparams, precision), hparams) or ent.hn != csr.n_nodes:
            return None
    hit = lookup(module, edge_attr, csr, pm, weights, biases, precision, mode="on" if now else None, allow_partial=False)
    ent = _entries.get(module)
    if ent is not None:
        ent.w.clear()                   # (a hit on H: release the previous tensor before allocating the next one)
    if hit is None or hit[2] != csr.n_nodes:
        return None
    try:
        we = ops.edge_weights_raw(hit[0].detach(), pm, w_last, b_last)
    except torch.OutOfMemoryError:      # 16 KiB per edge: an optimisation like H - on OOM the ordinary path runs
        torch.cuda.empty_cache()
        stats["oom_fallbacks"] = stats.get("oom_fallbacks", 0) + 1
        return None
    ent.w.store(we, key, params, (edge_attr, csr))
    stats["we_builds"] += 1
    return we
