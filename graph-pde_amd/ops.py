"""Host side of the NNConv hot path: CSR / packed-weight caches and the forward call.

PyTorch is used for device memory, the caching allocator and the current HIP stream only; all
arithmetic happens in libgpde.so (hand-written HIP, include/gpde.h).  Everything here refuses to
run on CPU tensors: there is no non-HIP path.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

WIDTH = _lib.GPDE_WIDTH


# ----------------------------------------------------------------------------------------------
# cached device buffers and streams (DESIGN.md "Streams"): what the library cached itself, the library orders
# ----------------------------------------------------------------------------------------------
cross_stream_hits: "dict[str, int]" = {}    # cache name -> hits from another stream than the entry's builder that were ordered (tests)


def _current_stream(dev):
    return torch.cuda.current_stream(dev)


def _capturing() -> bool:
    return torch.cuda.is_current_stream_capturing()


class StreamTag:
    """Where a cached entry was built: made right after its LAST build kernel was launched.  `stream`: the stream current then;
    `event`: recorded on it at that point (None for an entry built while the stream was being captured - nothing ran - or
    `synced`: the builder waited on the host for the device after the build, as build_csr does when it reads the bad-edge count
    back - such an entry cannot be read unfinished and needs no event); `ordered`: the other streams that have already been
    queued behind the build."""
    __slots__ = ("dev", "stream", "event", "synced", "ordered")

    def __init__(self, dev, synced: bool = False):
        self.dev, self.synced, self.ordered = dev, synced, None
        self.stream = _current_stream(dev)
        self.event = None
        if not synced and not _capturing():
            self.event = torch.cuda.Event()
            self.event.record(self.stream)


def stream_tag(dev, synced: bool = False) -> Optional[StreamTag]:
    """The StreamTag of an entry just built on `dev` (None off the GPU: the host tier builds entries from CPU stand-ins)."""
    return StreamTag(dev, synced) if torch.device(dev).type == "cuda" else None


def order_hit(tag: Optional[StreamTag], cache: str, buffers=()):
    """A cache hit: called before the entry's device buffers go to a native call.  On the stream the entry was built on - every
    training loop - this compares two stream handles and returns: no event call, no allocation.  From another stream, once per
    entry and stream: the stream waits for the build's event and every buffer is `record_stream`ed on it, so that the caching
    allocator does not hand the block out again (after `clear_caches()`, an LRU eviction, a replaced pack) while that stream may
    still read it.  While the stream is being captured nothing is issued: capture.py warms up, synchronises the device and records
    on one stream, and pins what the graph reads."""
    if tag is None or _current_stream(tag.dev) == tag.stream:
        return
    _order_cross_stream(tag, _current_stream(tag.dev), cache, buffers)


def _wait_for_build(tag: StreamTag, stream):
    if tag.event is not None:
        stream.wait_event(tag.event)
    elif not tag.synced:                     # built during a capture: no event exists - behind everything queued on the builder
        stream.wait_stream(tag.stream)


def _keep_for(t: torch.Tensor, stream):
    t.detach().record_stream(stream)


def _order_cross_stream(tag: StreamTag, stream, cache: str, buffers):
    if _capturing() or (tag.ordered is not None and stream in tag.ordered):
        return
    _wait_for_build(tag, stream)
    for t in buffers:
        if t is not None:
            _keep_for(t, stream)
    if tag.ordered is None:
        tag.ordered = set()
    tag.ordered.add(stream)
    cross_stream_hits[cache] = cross_stream_hits.get(cache, 0) + 1


class Cached:
    """One cached device value, declared ONCE where it is built.  `value`: what the cache hands out; `buffers`: the device tensors a
    native call will read; `pins`: other objects kept alive only so that the key stays meaningful (the tensor or storage whose address
    is in it, the `Csr`); `tag`: the StreamTag `stamp` makes right after the LAST build kernel was launched; `nbytes`: for byte bounds."""
    __slots__ = ("value", "buffers", "pins", "tag", "nbytes")

    def __init__(self, value=None, buffers=(), pins=(), nbytes: int = 0):
        self.value, self.buffers, self.pins, self.tag, self.nbytes = value, buffers, pins, None, nbytes

    def stamp(self, dev, synced: bool = False):
        self.tag = stream_tag(dev, synced)
        return self

    def hit(self, cache: str):               # the only way a hit is ordered
        tag = self.tag                       # (order_hit's own first test, made here too: on the builder's stream - every training
        if tag is not None and _current_stream(tag.dev) != tag.stream:      # loop - the call is spared, 5 % of a csr_for hit)
            order_hit(tag, cache, self.buffers)

    def held(self) -> tuple:                 # the only thing a snapshot collects
        return self.buffers + self.pins


class Lru:
    """Records by key in an insertion-ordered dict, least recently used first; `name`: what the cache is called in `cross_stream_hits`.  Over
    `max_entries`, or over `max_bytes` in the running sum of the records' `nbytes`, the oldest go - the byte bound spares the last one."""

    def __init__(self, name: str, max_entries: Optional[int] = None, max_bytes: Optional[int] = None):
        self.name, self.max_entries, self.max_bytes = name, max_entries, max_bytes
        self._d, self.nbytes = {}, 0

    def get(self, key) -> Optional[Cached]:
        d = self._d
        rec = d.pop(key, None)
        if rec is not None:
            d[key] = rec                         # move to the MRU end
        return rec

    def put(self, key, rec: Cached):
        self.pop(key)
        self._d[key] = rec
        self.nbytes += rec.nbytes
        while (self.max_entries is not None and len(self._d) > self.max_entries) or \
                (self.max_bytes is not None and len(self._d) > 1 and self.nbytes > self.max_bytes):
            self.pop(next(iter(self._d)))

    def pop(self, key) -> Optional[Cached]:
        rec = self._d.pop(key, None)
        self.nbytes -= 0 if rec is None else rec.nbytes
        return rec

    def clear(self):
        self._d, self.nbytes = {}, 0

    def __len__(self):
        return len(self._d)

    def __iter__(self):
        return iter(self._d)

    def values(self):
        return self._d.values()


class Pair(Cached):
    """A record that still reads as the pair its cache held before, (pins[0], value): (source tensor, slot-ordered copy) in
    `Csr._attr_sorted`, (weak references to the parameters, PackedMlp) in `_pack_cache`."""

    def __getitem__(self, i):
        return (self.pins[0], self.value)[i]


def mem_key(t: torch.Tensor) -> tuple:       # the core of every cache key on a tensor's memory: where it lies, its layout, `_ver`
    return (t.untyped_storage().data_ptr(), t.storage_offset(), t.shape, t.stride(), _ver(t))      # (Size and stride: tuples already)


# ----------------------------------------------------------------------------------------------
# destination-sorted CSR, cached per edge_index tensor
# ----------------------------------------------------------------------------------------------
@dataclass
class Csr:
    n_nodes: int
    n_edges: int
    rowptr: torch.Tensor   # int32 [N+1]
    src: torch.Tensor      # int32 [E]  source node of each CSR slot
    dst: torch.Tensor      # int32 [E]  target node of each CSR slot (sorted ascending)
    perm: torch.Tensor     # int32 [E]  CSR slot -> original edge id (stable within a target)
    _rowptr_host: Optional[torch.Tensor] = None
    _src_order: Optional[tuple] = None       # (src_rowptr, src_slots) - `src_order` - and the record that declares them
    _src_order_rec: Optional[Cached] = None
    _attr_sorted: Optional[dict] = None      # edge_attr tensors gathered into CSR slot order (attr_in_slot_order)
    _identity: Optional[Cached] = None       # value: the identity permutation (attr_in_slot_order)
    _perm_is_identity: bool = False
    _max_in_degree: Optional[int] = None
    n_src_nodes: Optional[int] = None        # a RECTANGULAR graph: `src` indexes this many source nodes, `n_nodes` counts the destination
    #                                          rows (rowptr has n_nodes + 1 entries); None: square, one node set
    _flow_flipped: bool = False              # built from edge_index with its rows swapped (flow='target_to_source' of the module)
    _chain_blocks: Optional[dict] = None         # block tables of the streamed any-width route (chain_any_blocks), host only

    @property
    def n_src(self) -> int:
        """Number of SOURCE nodes: `n_src_nodes` of a rectangular graph, `n_nodes` of a square one."""
        return self.n_nodes if self.n_src_nodes is None else int(self.n_src_nodes)

    @property
    def max_in_degree(self) -> int:
        """Largest in-degree of a node (build_csr records it with its one sync; other CSRs read rowptr_host once)."""
        if self._max_in_degree is None:
            rp = self.rowptr_host.to(torch.int64)
            self._max_in_degree = int((rp[1:] - rp[:-1]).max()) if self.n_nodes > 0 else 0
        return self._max_in_degree

    @property
    def src_order(self):
        """(src_rowptr int32 [N+1], src_slots int32 [E]): the CSR slots regrouped by SOURCE node
        (gpde_csr_source_order), built on first use and kept with the CSR.  The backward sums dx_j over the out-edges
        of j in this order instead of by atomics: gradients are bit-reproducible.  GPDE_BWD_DX=atomic skips it."""
        if DX_MODE == "atomic":
            return None, None
        if self._src_order is None:
            lib = _lib.lib()
            dev = self.rowptr.device
            n_src = self.n_src                    # (a rectangular graph: the order runs over its source nodes)
            srp = torch.empty(n_src + 1, dtype=torch.int32, device=dev)
            ssl = torch.empty(max(self.n_edges, 1), dtype=torch.int32, device=dev)
            nbytes = int(lib.gpde_csr_workspace_bytes(self.n_edges, n_src))
            ws = _alloc_ws(nbytes, dev)
            with torch.cuda.device(dev):
                rc = lib.gpde_csr_source_order(self.src.data_ptr(), self.n_edges, n_src, srp.data_ptr(),
                                               ssl.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
            _lib.check(rc, "gpde_csr_source_order")
            self._src_order, self._src_order_rec = (srp, ssl), Cached(buffers=(srp, ssl)).stamp(dev)
        elif self._src_order_rec is not None:        # (none: a source order that was handed in, not built here)
            self._src_order_rec.hit("src_order")
        return self._src_order

    def records(self) -> list:               # of what was built on this graph on first use (cache_snapshot)
        return [r for r in (self._src_order_rec, self._identity, *(self._attr_sorted or {}).values()) if r is not None]

    @property
    def edge_index(self) -> torch.Tensor:
        """int64 [2, E] (source, target) in CSR SLOT order - the edge list to build per-edge tensors from when the graph
        came from `radius_csr` (perm = identity: edge_attr rows are addressed by CSR slot)."""
        return torch.stack([self.src.long(), self.dst.long()])

    @property
    def rowptr_host(self) -> torch.Tensor:
        """Host copy of rowptr (int32, pinned lifetime = the CSR): the backward plans its edge
        chunks on the host.  One device->host copy per graph."""
        if self._rowptr_host is None:
            self._rowptr_host = self.rowptr.cpu().contiguous()
        return self._rowptr_host


DX_MODE = os.environ.get("GPDE_BWD_DX", "ordered")     # "ordered" (bit-reproducible grad_x) | "atomic"


def _stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def _call(name: str, dev, *args, label: Optional[str] = None, calls: int = 1):
    """One counted native call: entry point `name` with `args` and, last, the current stream of `dev`, under the device guard; a
    refusal is raised under `label` (default: the entry point's name); `calls`: operator calls the launch stands for."""
    with torch.cuda.device(dev):
        rc = getattr(_lib.lib(), name)(*args, _stream_ptr(dev))
    _lib.check(rc, label or name)
    _lib.n_native_calls += calls


_ver_memo: "dict | None" = None          # content checksums of inference tensors computed during the current operator call


class ver_scope:
    """Within one operator call an inference tensor's checksum is computed once and reused by every cache key that needs it
    (CSR, slot-order attributes, hidden activations: up to six lookups per call, each two device passes + a host sync
    before - ADVICE r3).  Across calls nothing is remembered: such tensors can change in place without a trace."""

    def __enter__(self):
        global _ver_memo
        self.outer = _ver_memo
        if _ver_memo is None:
            _ver_memo = {}
        return self

    def __exit__(self, *exc):
        global _ver_memo
        _ver_memo = self.outer
        return False


_HASH_W = None


def _content_hash(t: torch.Tensor) -> int:
    """Position-sensitive checksum of a tensor's bytes: 32-bit words in rows of 4096, every word weighted by a fixed odd
    multiplier of its column, every row sum by an odd multiplier of its row number (float64 arithmetic on the device: exact
    products, deterministic sums).  A permutation of rows or a sum-preserving edit changes it; one pass, one host sync."""
    global _HASH_W
    c = t.contiguous()
    nb = c.numel() * c.element_size()
    raw = c.view(torch.uint8).reshape(-1)
    if nb % 4:
        raw = torch.cat([raw, raw.new_zeros(4 - nb % 4)])
    words = raw.view(torch.int32)
    cols = 4096
    if _HASH_W is None or _HASH_W.device != words.device:
        g = torch.Generator().manual_seed(0x9E3779B9)
        _HASH_W = (torch.randint(1, 1 << 20, (cols,), generator=g, dtype=torch.int64) * 2 + 1).to(torch.float64).to(words.device)
    total, row0 = 0.0, 0
    step = cols << 12                                   # 16 Mi words (64 MB) per piece: bounds the float64 temporary
    for lo in range(0, words.numel(), step):
        w = words[lo:lo + step]
        pad = (-w.numel()) % cols
        if pad:
            w = torch.cat([w, w.new_zeros(pad)])
        rows = w.view(-1, cols).to(torch.float64) @ _HASH_W
        mult = (torch.arange(row0, row0 + rows.numel(), device=rows.device, dtype=torch.float64) * 2 + 1) % 1048573.0
        total = total + (rows % 2147483647.0 * mult).sum()
        row0 += rows.numel()
    return int(float(total) % 9007199254740881.0) ^ (nb << 1)


def _ver(t: torch.Tensor):
    """Cache-key component that changes whenever the tensor's contents may have changed.  Normal tensors: the
    in-place version counter.  Inference tensors track none (reading `_version` raises) yet CAN be modified in place
    inside torch.inference_mode() - an `edge_attr.mul_()` between two forwards of an eval loop would hit the CSR /
    staging / hidden-activation caches with an identical key.  For them the key carries a position-sensitive
    content checksum instead (`_content_hash`: one pass + one device->host scalar), computed once per operator call
    (`ver_scope`): inference tensors only."""
    if not t.is_inference():
        return t._version
    if t.numel() == 0:
        return ("inference", 0)
    memo = _ver_memo
    k = (t.data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)
    if memo is not None and k in memo:
        return memo[k]
    v = ("inference", _content_hash(t))
    if memo is not None:
        memo[k] = v
    return v


def staging_device() -> torch.device:
    """Where CPU tensors are staged: the current HIP device.  There is ONE execution path - the HIP kernels
    of libgpde.so; a model moved back with `model.cpu()` (UAI1_full_resolution.py:287-303) has its inputs and
    parameters copied to the GPU for the call and the result copied back.  Without a GPU this raises."""
    if not torch.cuda.is_available():
        raise RuntimeError(
            "the NNConv hot path runs only on an MI355X through libgpde.so: CPU tensors are staged to the "
            "current HIP device, and no HIP device is visible (no CPU / composite fallback exists by design)")
    return torch.device("cuda", torch.cuda.current_device())


_stage_cache = Lru("stage_const", max_entries=16)      # constant inputs (edge_index, edge_attr) staged once per tensor; pins: the CPU storage


def stage_const(t: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """Device copy of a CPU tensor that is not differentiated (edge_index, edge_attr), cached on the tensor's
    storage + version so that the `depth` applications of one forward share the copy (and its CSR)."""
    if t.is_cuda:
        return t
    key = mem_key(t) + (t.dtype, str(dev))
    hit = _stage_cache.get(key)
    if hit is None:
        copy = t.detach().to(dev)
        hit = Cached(copy, (copy,), (t.untyped_storage(),))
        _stage_cache.put(key, hit)
    return hit.value


def gather_rows(rows: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """out[s] = rows[perm[s]] (gpde_gather_rows): one native pass, no int64 index temporaries, no torch advanced indexing
    (unreliable above 2^26 rows on this torch / ROCm build: synth.darcy_edge_attr)."""
    _require_cuda(rows, "rows")
    _require_cuda(perm, "perm")
    if rows.dtype != torch.float32 or rows.dim() != 2 or perm.dtype != torch.int32:
        raise ValueError("gather_rows: float32 [rows, k] and an int32 permutation")
    rows = _operand(rows, "rows", (None, None), rows.device)
    perm = _operand(perm, "perm", (None,) * perm.dim(), rows.device, dtype=torch.int32)
    n = int(perm.numel())
    out = torch.empty(n, rows.size(1), dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        rc = _lib.lib().gpde_gather_rows(rows.data_ptr(), int(rows.size(1)), perm.data_ptr(), n, out.data_ptr(),
                                         _stream_ptr(rows.device))
    _lib.check(rc, "gpde_gather_rows")
    return out


ATTR_SLOT_ORDER = os.environ.get("GPDE_ATTR_SLOT_ORDER", "1") != "0"
_ATTR_SLOT_ORDER_MIN_EDGES = 32768


def identity_probe(e: int, device=None, k: int = 4096) -> torch.Tensor:
    """min(e, k) slot indices spread evenly over [0, e - 1], int64, first 0 and last e - 1, built in integers.  (A float32
    linspace rounds its end point above 2^24: for e = 95,530,006 the last index came out as 95,530,008, past the end.)"""
    k = min(int(e), int(k))
    return (torch.arange(k, dtype=torch.int64, device=device) * (int(e) - 1)) // max(k - 1, 1)


def attr_in_slot_order(csr: "Csr", edge_attr: torch.Tensor):
    """(edge_attr rows gathered into CSR slot order, identity perm) - cached on the CSR per edge_attr memory + version.

    The fused kernels address attributes as edge_attr[perm[slot]].  For a graph given in the reference's source-major edge
    order, the in-edges of one destination are ~in-degree rows scattered over the whole [E, k0] tensor: every edge costs a
    cache line per column slice (8 per forward at k2 = 1024) instead of 24 bytes of a stream.  Like the CSR itself, the
    gathered copy is built once per (graph, edge_attr) and serves every later call (`depth` applications, every epoch):
    the side loads become sequential and `perm` an identity.  Same values, same summation order: bit-identical results.
    GPDE_ATTR_SLOT_ORDER=0 keeps the indirect addressing (A/B); graphs built by `radius_csr` already are in slot order."""
    e = csr.n_edges
    if not ATTR_SLOT_ORDER or e < _ATTR_SLOT_ORDER_MIN_EDGES or edge_attr.requires_grad or edge_attr.dtype != torch.float32:
        return edge_attr, csr.perm
    if csr._identity is None:
        ident = torch.arange(e, dtype=torch.int32, device=csr.perm.device)
        csr._identity = Cached(ident, (ident,)).stamp(ident.device, synced=True)      # (complete: the probe below waits for the device)
        csr._attr_sorted = {}
        # is `perm` the identity (a graph already in slot order)?  A full comparison is a pass over 95.5 M indices plus a byte mask
        # of the same length on the headline graph - 21 of the 23 ms a NEW sample's first call spent here (profiles/
        # r06_attr_reorder_probe.txt; the gather itself is 2.2 ms).  A graph in the reference's source-major order fails the
        # comparison at almost every slot: 4096 sampled slots decide it; only a sample that passes is followed by the full check.
        probe = identity_probe(e, csr.perm.device)
        csr._perm_is_identity = bool(torch.equal(csr.perm[probe], probe.to(torch.int32))) and bool(torch.equal(csr.perm, ident))
    if csr._perm_is_identity:
        return edge_attr, csr.perm
    key = mem_key(edge_attr)
    hit = csr._attr_sorted.get(key)
    if hit is None:
        out = gather_rows(edge_attr.detach(), csr.perm)
        while len(csr._attr_sorted) >= 2:
            csr._attr_sorted.pop(next(iter(csr._attr_sorted)))
        hit = csr._attr_sorted[key] = Pair(out, (out,), (edge_attr,)).stamp(out.device)  # the source tensor is kept alive: its address is part of the key
    else:
        hit.hit("attr_slot_order")
    # the identity permutation serves every entry of this CSR, built or hit: kept for a stream other than the one it was made on
    csr._identity.hit("attr_identity")
    return hit.value, csr._identity.value


def _require_cuda(t, name: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: the NNConv hot path runs only on an MI355X through libgpde.so "
            "(no CPU / composite fallback exists by design)")


def _ptr(t):
    """`t.data_ptr()`, NULL for an operand that is not there."""
    return None if t is None else t.data_ptr()


def _ptr_array(ts):
    """The `void*` array of a native call over a list of tensors (NULL for a None entry)."""
    return (ctypes.c_void_p * len(ts))(*[_ptr(t) for t in ts])


def _dense16(t: torch.Tensor) -> torch.Tensor:
    """`t` itself when it is dense (contiguous) and starts on a 16-byte boundary, else a fresh dense copy (the allocators of
    torch hand out blocks aligned far beyond 16 bytes).  The 64-wide kernels read their operands with 16-byte vector accesses."""
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    t = t.detach()
    return torch.empty_like(t, memory_format=torch.contiguous_format).copy_(t)


def _operand(t: Optional[torch.Tensor], name: str, shape, dev, *, writable: bool = False, dtype: torch.dtype = torch.float32,
             exc=ValueError) -> Optional[torch.Tensor]:
    """The one gate between a tensor and `data_ptr()` of a native call (DESIGN.md "Operand layouts").  `shape`: the exact
    shape, None = any extent in that dimension; `dev`: the call's device.  A wrong dtype, shape or device raises `exc` naming
    the operand.  A READ-ONLY operand may come in any layout: it is returned as the tensor itself when that is dense and
    16-byte aligned (no copy, the same object and `data_ptr` for the caches), else as a detached dense aligned copy.  A WRITTEN operand
    (`writable`: out, z_keep, acc, ws) is never copied - the caller would not see the result: it must be dense and aligned
    as it is, or ValueError.  None passes through."""
    if t is None:
        return None
    want = tuple(shape)
    ok_shape = t.dim() == len(want) and all(w is None or int(w) == int(s) for w, s in zip(want, t.shape))
    if t.dtype != dtype or not ok_shape or t.device != dev:
        dims = ",".join("*" if w is None else str(int(w)) for w in want)
        raise exc(f"{name} must be {str(dtype).replace('torch.', '')} [{dims}] on {dev}, got {str(t.dtype).replace('torch.', '')} "
                  f"{tuple(t.shape)} on {t.device}")
    if writable:
        if not t.is_contiguous() or t.data_ptr() % 16 != 0:
            raise ValueError(f"{name} is written by the kernels in place: it must be contiguous and 16-byte aligned, got strides "
                             f"{tuple(t.stride())} at an address = {t.data_ptr() % 16} mod 16 (pass a dense tensor; views are not copied)")
        return t
    return _dense16(t)


def _operands(ts, name: str, shapes, dev):
    """`_operand` over the per-layer weights or biases of a kernel MLP (None entries pass through)."""
    return [_operand(t, f"{name}[{l}]", s, dev) for l, (t, s) in enumerate(zip(ts, shapes))]


def _mlp_shapes(dims: Sequence[int]):
    """([weight shapes], [bias shapes]) of the Linear layers of widths `dims`."""
    return [(dims[l + 1], dims[l]) for l in range(len(dims) - 1)], [(dims[l + 1],) for l in range(len(dims) - 1)]


def _mlp_dims(weights) -> List[int]:
    """The layer widths of a kernel MLP, read off ALL its weights."""
    return [int(weights[0].size(1))] + [int(w.size(0)) for w in weights]


def _mlp_operands(weights, biases, dev, dims: Optional[Sequence[int]] = None):
    """The kernel MLP of a native call: (dims, dims_c, weights, biases) with every given layer checked as an operand (None
    entries pass through).  `dims`: all layer widths where `weights` holds only the first layers; else read off the weights."""
    if dims is None:
        dims = _mlp_dims(weights)
    w_shapes, b_shapes = _mlp_shapes(dims)
    return (dims, _lib.dims_array(dims), _operands([None if w is None else w.detach() for w in weights], "weights", w_shapes, dev),
            _operands([None if b is None else b.detach() for b in biases], "biases", b_shapes, dev))


def _update_grads(root, need_root: bool, need_bias: bool, dev):
    """(grad_root [64, 64] or None, grad_bias [64] or None): the update() gradients a 64-wide backward call writes."""
    return (torch.empty(WIDTH, WIDTH, dtype=torch.float32, device=dev) if (need_root and root is not None) else None,
            torch.empty(WIDTH, dtype=torch.float32, device=dev) if need_bias else None)


def _queried_ws(query: str, dev, *args) -> torch.Tensor:
    """A workspace of the size the library's `query` names for `args` (0 = the query refused the shape: its message is raised)."""
    nbytes = int(getattr(_lib.lib(), query)(*args))
    if nbytes == 0:
        _lib.check(-2, query)
    return _alloc_ws(nbytes, dev)


def build_csr(edge_index: torch.Tensor, n_nodes: int, n_src: Optional[int] = None, flip: bool = False) -> Csr:
    """gpde_csr_from_coo on the current stream. `edge_index` int64 [2,E], any strides.
    `n_src`: the graph is RECTANGULAR - row 0 indexes n_src source nodes, row 1 the n_nodes destinations (gpde_csr_from_coo2).
    `flip`: the rows swapped (row 1 = sources, row 0 = destinations: flow='target_to_source') - the library reads the same
    memory through a negative row stride, no copy is made."""
    _require_cuda(edge_index, "edge_index")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must be int64 [2,E], got {edge_index.dtype} {tuple(edge_index.shape)}")
    if n_src is not None or flip:
        return _build_csr_general(edge_index, int(n_nodes), None if n_src is None else int(n_src), bool(flip))
    lib = _lib.lib()
    dev = edge_index.device
    e = int(edge_index.size(1))
    if e == 0:                     # a graph without edges (update() of the module surface): nothing to sort
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return Csr(n_nodes, 0, torch.zeros(n_nodes + 1, dtype=torch.int32, device=dev), z, z.clone(), z.clone())
    rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    src = torch.empty(e, dtype=torch.int32, device=dev)
    dst = torch.empty(e, dtype=torch.int32, device=dev)
    perm = torch.empty(e, dtype=torch.int32, device=dev)
    n_bad = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.gpde_csr_workspace_bytes(e, n_nodes))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gpde_csr_from_coo(edge_index.data_ptr(), edge_index.stride(0), edge_index.stride(1),
                                   e, n_nodes, rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                   perm.data_ptr(), n_bad.data_ptr(), ws.data_ptr(), ws_bytes,
                                   _stream_ptr(dev))
    _lib.check(rc, "gpde_csr_from_coo")
    # one sync per *new* graph (the result is cached): the bad-edge count and the largest in-degree together
    bad, max_deg = (int(v) for v in torch.stack([n_bad[0], (rowptr[1:] - rowptr[:-1]).max()]).cpu())
    if bad:
        raise IndexError(f"edge_index has {bad} edges with an endpoint outside [0, {n_nodes})")
    return Csr(n_nodes, e, rowptr, src, dst, perm, _max_in_degree=max_deg)


def _build_csr_general(edge_index: torch.Tensor, n_dst: int, n_src: Optional[int], flip: bool) -> Csr:
    """build_csr of a rectangular graph and / or of edge_index with its rows swapped (gpde_csr_from_coo2)."""
    lib = _lib.lib()
    dev = edge_index.device
    e = int(edge_index.size(1))
    ns = n_dst if n_src is None else n_src
    if e == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return Csr(n_dst, 0, torch.zeros(n_dst + 1, dtype=torch.int32, device=dev), z, z.clone(), z.clone(), n_src_nodes=n_src,
                   _flow_flipped=flip)
    rowptr = torch.empty(n_dst + 1, dtype=torch.int32, device=dev)
    src, dst, perm = (torch.empty(e, dtype=torch.int32, device=dev) for _ in range(3))
    n_bad = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.gpde_csr_workspace_bytes(e, max(ns, n_dst)))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    # rows swapped: start at row 1 and step back one row - the strides of the C call are signed
    base, s_row = edge_index.data_ptr(), edge_index.stride(0)
    if flip:
        base, s_row = base + s_row * edge_index.element_size(), -s_row
    with torch.cuda.device(dev):
        rc = lib.gpde_csr_from_coo2(base, s_row, edge_index.stride(1), e, ns, n_dst, rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                    perm.data_ptr(), n_bad.data_ptr(), ws.data_ptr(), ws_bytes, _stream_ptr(dev))
    _lib.check(rc, "gpde_csr_from_coo2")
    bad, max_deg = (int(v) for v in torch.stack([n_bad[0], (rowptr[1:] - rowptr[:-1]).max() if n_dst > 0 else n_bad[0] * 0]).cpu())
    if bad:
        r_src, r_dst = (1, 0) if flip else (0, 1)
        bs = int(((edge_index[r_src] < 0) | (edge_index[r_src] >= ns)).sum())
        bd = int(((edge_index[r_dst] < 0) | (edge_index[r_dst] >= n_dst)).sum())
        sides = ([f"{bs} edges with a source (row {r_src}) outside [0, {ns})"] if bs else []) + \
                ([f"{bd} edges with a destination (row {r_dst}) outside [0, {n_dst})"] if bd else [])
        raise IndexError("edge_index has " + " and ".join(sides))
    return Csr(n_dst, e, rowptr, src, dst, perm, _max_in_degree=max_deg, n_src_nodes=n_src, _flow_flipped=flip)


_csr_cache = Lru("csr", max_entries=64, max_bytes=8 << 30)      # value: the Csr; pins: the index storage, nbytes: its size


def csr_for(edge_index: torch.Tensor, n_nodes: int, n_src: Optional[int] = None, flip: bool = False) -> Csr:
    """Cached CSR (`n_src`: a rectangular graph of n_src sources and n_nodes destinations; `flip`: rows swapped - build_csr;
    both are part of the key, and a `Csr` handed in is checked against both node counts):: the reference calls the same conv `depth` times with the same edge_index
    (UAI1_full_resolution.py:29-30), and MGKN re-slices the same tensors every V-cycle
    (MGKN_general_darcy2d.py:79-89).  Key = storage pointer, offset, shape, strides, in-place
    version counter, node count.  The entry keeps the index storage alive so that its address
    cannot be recycled for a different graph while cached; the cache is a byte-bounded LRU."""
    if isinstance(edge_index, Csr):          # a graph that already is a destination CSR (radius_csr, parallel.partition_rows_by_position)
        if edge_index.n_nodes != n_nodes:
            raise ValueError(f"the CSR was built for {edge_index.n_nodes} nodes, x has {n_nodes} rows")
        if edge_index.n_src != (n_nodes if n_src is None else int(n_src)):
            raise ValueError(f"the CSR was built for {edge_index.n_src} source nodes, the call has {n_nodes if n_src is None else int(n_src)}")
        return edge_index
    watch(edge_index)
    key = (str(edge_index.device), *mem_key(edge_index), n_nodes)
    if n_src is not None or flip:
        key = key + (None if n_src is None else int(n_src), bool(flip))
    hit = _csr_cache.get(key)
    if hit is not None:
        hit.hit(_csr_cache.name)
        return hit.value
    csr = build_csr(edge_index, n_nodes, n_src, flip)
    storage = edge_index.untyped_storage()
    # (build_csr read the bad-edge count back: the arrays are complete - a hit from another stream only keeps them from being recycled)
    arrays = (csr.rowptr, csr.src, csr.dst, csr.perm) if edge_index.is_cuda else ()      # (off the GPU `csr` may be a stand-in without them)
    _csr_cache.put(key, Cached(csr, arrays, (csr, storage), storage.nbytes()).stamp(edge_index.device, synced=int(edge_index.size(1)) > 0))
    return csr


_capture_watch: "list | None" = None      # capture.py: while a call is being recorded, the tensors cache keys were built from


def watch(*tensors):
    """capture.py's staleness check: a recorded call replays what the caches held at recording time (packed weights, hidden
    activations, CSRs) - every tensor such a cache key is built from is noted while `_capture_watch` is a list, with its version."""
    if _capture_watch is not None:
        for t in tensors:
            if isinstance(t, torch.Tensor) and not t.is_inference():
                _capture_watch.append((t, t._version))


def cache_snapshot() -> list:
    """Strong references to every device buffer the caches of this module own right now (CSRs with their source-order arrays
    and slot-ordered attribute copies, packed weights, staged constants): capture.py pins them for the lifetime of a recorded
    graph, whose kernels read those addresses whatever the LRU policies do afterwards."""
    recs = [r for cache in (_csr_cache, _pack_cache, _stage_cache, _gcn_norm_cache) for r in cache.values()]
    for owner in [r.value for r in recs if isinstance(r.value, (Csr, GcnNorm))]:       # what a graph / a normalisation built on first use
        recs.extend(owner.records())
    return [r.held() for r in recs]


def clear_param_caches():
    """Drop the packed-weight cache only (capture.py: a recorded optimizer step rewrote the weights without moving their
    version counters; the graphs - CSR cache - are untouched)."""
    _pack_cache.clear()
    _pack_by_ptr.clear()


def clear_caches():
    """Drop the CSR / packed-weight / staging caches.  REQUIRED after writing a parameter or an index tensor
    through `.data` (`p.data.add_(..)`, `p.data.clamp_()`, `dist.broadcast(p.data)`): such writes do not bump
    the version counter the cache keys are built on (tests/test_host_logic.py pins this contract)."""
    for cache in (_csr_cache, _pack_cache, _stage_cache, _gcn_norm_cache):
        cache.clear()
    _pack_by_ptr.clear()
    cross_stream_hits.clear()


# ----------------------------------------------------------------------------------------------
# kernel MLP: parameter extraction and MFMA-order packing, cached per parameter version
# ----------------------------------------------------------------------------------------------
def mlp_linears(mlp: torch.nn.Module) -> List[torch.nn.Linear]:
    """The Linear layers of a DenseNet-style kernel MLP (Linear, ReLU, ..., Linear):
    /root/reference/graph-neural-operator/utilities.py:201-227.  Anything else is rejected loudly."""
    if hasattr(mlp, "layers") and isinstance(mlp.layers, torch.nn.ModuleList):
        layers = list(mlp.layers)
    elif isinstance(mlp, torch.nn.Sequential):
        layers = list(mlp)
    elif isinstance(mlp, torch.nn.Linear):
        layers = [mlp]
    else:
        raise NotImplementedError(
            f"kernel network of type {type(mlp).__name__} is not a Linear/ReLU chain; the fused "
            "MI355X operator implements the DenseNet kernels used by the reference scripts")
    lin: List[torch.nn.Linear] = []
    expect_linear = True
    for l in layers:
        if isinstance(l, torch.nn.Linear):
            if not expect_linear:
                raise NotImplementedError("two Linear layers without ReLU between them")
            lin.append(l)
            expect_linear = False
        elif isinstance(l, torch.nn.ReLU):
            if expect_linear:
                raise NotImplementedError("ReLU without a preceding Linear layer")
            expect_linear = True
        else:
            raise NotImplementedError(f"kernel network layer {type(l).__name__} is not supported "
                                      "(Linear/ReLU chains only)")
    if expect_linear or len(lin) < 2:
        raise NotImplementedError("kernel network must be Linear,(ReLU,Linear)+ ending in Linear")
    return lin


class Sin(torch.nn.Module):
    """`torch.sin` as a module: `DenseNet(layers, graph_pde_amd.Sin)` is the sine kernel network `mlp_chain` reads (the reference's
    `DenseNet_sin` applies torch.sin inside its forward, which no parser of layers can see)."""

    def forward(self, x):
        return torch.sin(x)


# GPDE_ACT_* of include/gpde.h: the hidden activations of the streamed any-width route (csrc/gpde_chain_any.hip)
ACT_RELU, ACT_LEAKY_RELU, ACT_ELU, ACT_TANH, ACT_SIGMOID, ACT_GELU, ACT_GELU_TANH, ACT_SILU, ACT_SIN = range(9)
ACT_NAMES = ("relu", "leaky_relu", "elu", "tanh", "sigmoid", "gelu", "gelu_tanh", "silu", "sin")
ACT_FROM_U = frozenset((ACT_GELU, ACT_GELU_TANH, ACT_SILU, ACT_SIN))      # act' needs the pre-activation: the backward keeps U_l too


def _act_of(layer) -> Optional[Tuple[int, float, float]]:
    """(kind, p0, p1) of one activation module, or None.  Exact classes only: a subclass may override `forward`."""
    t, nn = type(layer), torch.nn
    if t is nn.ReLU:
        return (ACT_RELU, 0.0, 0.0)
    if t is nn.LeakyReLU:            # (act' is read from the value: a negative slope would make the value's sign ambiguous)
        s = float(layer.negative_slope)
        return (ACT_LEAKY_RELU, s, 0.0) if s >= 0.0 and s != float("inf") else None
    if t is nn.ELU:
        a = float(layer.alpha)
        return (ACT_ELU, a, 0.0) if 0.0 < a < float("inf") else None
    if t is nn.Tanh:
        return (ACT_TANH, 0.0, 0.0)
    if t is nn.Sigmoid:
        return (ACT_SIGMOID, 0.0, 0.0)
    if t is nn.GELU:
        approx = getattr(layer, "approximate", "none")
        return (ACT_GELU, 0.0, 0.0) if approx == "none" else (ACT_GELU_TANH, 0.0, 0.0) if approx == "tanh" else None
    if t is nn.SiLU:
        return (ACT_SILU, 0.0, 0.0)
    if t is Sin:
        return (ACT_SIN, 0.0, 0.0)
    return None


def mlp_chain(mlp: torch.nn.Module):
    """(linears, acts) of a kernel network `Linear, (act, Linear)+` - a Sequential or a DenseNet-style `.layers` ModuleList -, `acts`
    one (kind, p0, p1) per hidden layer (ACT_*; `inplace` is irrelevant); None for anything else: BatchNorm, an output nonlinearity,
    a LeakyReLU of negative slope, an activation the library does not generate, a subclass of Linear or of an activation (it may
    override `forward`).  The chains `mlp_linears` takes are the all-ReLU ones of these."""
    if hasattr(mlp, "layers") and isinstance(mlp.layers, torch.nn.ModuleList):
        layers = list(mlp.layers)
    elif type(mlp) is torch.nn.Sequential:
        layers = list(mlp)
    else:
        return None
    if len(layers) < 3 or len(layers) % 2 == 0:
        return None
    lin, acts = [], []
    for i, l in enumerate(layers):
        if i % 2 == 0:
            if type(l) is not torch.nn.Linear:
                return None
            lin.append(l)
        else:
            a = _act_of(l)
            if a is None:
                return None
            acts.append(a)
    if any(u.out_features != v.in_features for u, v in zip(lin[:-1], lin[1:])):
        return None
    return lin, acts


def acts_all_relu(acts) -> bool:
    return acts is None or all(int(a[0]) == ACT_RELU for a in acts)


def acts_key(acts):
    """`acts` as a hashable key; None for an all-ReLU chain (the `_chain_any` entry points)."""
    return None if acts_all_relu(acts) else _acts_tuple(acts)


def _acts_tuple(acts):
    return tuple((int(a[0]), float(a[1]) if len(a) > 1 else 0.0, float(a[2]) if len(a) > 2 else 0.0) for a in acts)


def acts_arrays(acts):
    """The two host arrays of the `_chain_act` entry points: int32 kinds [n], float params [n][2]."""
    key = _acts_tuple(acts)
    kinds = (ctypes.c_int32 * len(key))(*[a[0] for a in key])
    params = (ctypes.c_float * (2 * len(key)))(*[v for a in key for v in a[1:3]])
    return kinds, params


@dataclass
class PackedMlp:
    dims: Tuple[int, ...]
    packed: torch.Tensor            # float32 flat buffer in libgpde layout
    dims_c: object                  # ctypes int32 array (kept alive)


_pack_cache = Lru("pack_mlp", max_bytes=1 << 30)      # value: the PackedMlp; pins: (weak references to the parameters - a hit's liveness check,)
_pack_by_ptr: "dict[tuple, tuple]" = {}      # parameter addresses -> current key (older versions are evicted)


def pack_mlp(weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]]) -> PackedMlp:
    """gpde_mlp_pack, cached per parameter set and version.  An optimizer step bumps the versions: the new
    pack REPLACES the entry of the same parameter addresses (no dead packs pile up: one [6,1024,1024,4096]
    pack is 24 MB), and the cache is a byte-bounded LRU."""
    lib = _lib.lib()
    n = len(weights)
    for w in weights:
        _require_cuda(w, "kernel-network weight")
        if w.dtype != torch.float32:
            raise NotImplementedError(f"kernel-network weights must be float32, got {w.dtype}")
    dims = tuple([int(weights[0].size(1))] + [int(w.size(0)) for w in weights])
    watch(*weights, *biases)
    ptrs = tuple(w.data_ptr() for w in weights) + tuple(0 if b is None else b.data_ptr() for b in biases) + (dims,)
    key = tuple((w.data_ptr(), _ver(w)) for w in weights) + \
        tuple((0, 0) if b is None else (b.data_ptr(), _ver(b)) for b in biases) + (dims,)
    hit = _pack_cache.get(key)
    # same parameter objects still alive => the addresses were not recycled
    if hit is not None and all(r() is t for r, t in zip(hit.pins[0], list(weights) + [b for b in biases if b is not None])):
        hit.hit(_pack_cache.name)
        return hit.value
    dims_c = _lib.dims_array(dims)
    nbytes = int(lib.gpde_mlp_pack_bytes(n, dims_c))
    if nbytes == 0:
        _lib.check(-2, "gpde_mlp_pack_bytes")      # message was set by the failed layout query
    dev = weights[0].device
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    w_shapes, b_shapes = _mlp_shapes(dims)
    ws = _operands([w.detach() for w in weights], "kernel-network weight", w_shapes, dev)
    bs = _operands([None if b is None else b.detach() for b in biases], "kernel-network bias", b_shapes, dev)
    wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    bp = (ctypes.c_void_p * n)(*[None if b is None else b.data_ptr() for b in bs])
    with torch.cuda.device(dev):
        rc = lib.gpde_mlp_pack(n, dims_c, wp, bp, packed.data_ptr(), nbytes, _stream_ptr(dev))
    _lib.check(rc, "gpde_mlp_pack")
    refs = tuple(weakref.ref(t) for t in list(weights) + [b for b in biases if b is not None])
    pm = PackedMlp(dims, packed, dims_c)
    _pack_cache.pop(_pack_by_ptr.get(ptrs))      # the same parameters at an older version, if there
    _pack_cache.put(key, Pair(pm, (packed,), (refs,), packed.numel() * 4).stamp(dev))
    _pack_by_ptr[ptrs] = key
    if len(_pack_by_ptr) > 4096:
        live = set(_pack_cache)
        for k in [k for k, v in _pack_by_ptr.items() if v not in live]:
            _pack_by_ptr.pop(k)
    return pm


# ----------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------
_AGGR = {"add": _lib.GPDE_AGGR_ADD, "mean": _lib.GPDE_AGGR_MEAN}
# arithmetic of the hidden k1 x k2 layer: "f32" = fp32 MFMA (exact fmaf chains); "f16split" = f16
# MFMA on two-term split operands with fp32 accumulation (include/gpde.h GPDE_FWD_F16SPLIT)
_PRECISION = {"f32": _lib.GPDE_FWD_DEFAULT, "f16split": _lib.GPDE_FWD_F16SPLIT,
              "f16split_8wave": _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_F16SPLIT_8WAVE,   # force the 8-wave kernel (small-graph path) everywhere
              "f16split_static": _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_STATIC_RANGES,  # v6 with static per-wave ranges instead of the block queue
              "f16split_agg16": _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_AGG_F16,  # aggregation on split f16 regardless of size
              "f16split_agg32": _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_AGG_F32,  # aggregation on fp32 MFMA regardless of size
              "f16split_noedge": _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_NO_EDGE_PATH,  # never the per-edge last layer of low in-degree graphs
              "f16split_noimage": _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_NO_ATTR_IMAGE}  # v6 forms its attribute operands per tile, not from the per-call image
# Names that choose no arithmetic of their own: "f16split_noimage" gives the bytes of "f16split" by construction (it only moves
# where the kernel's attribute operands are formed).  It is accepted, and left out of the choices an error message offers.
_SAME_BYTES_SWITCHES = ("f16split_noimage",)
DEFAULT_PRECISION = os.environ.get("GPDE_PRECISION", "f16split")


def _precision_choices() -> list:
    return sorted(k for k in _PRECISION if k not in _SAME_BYTES_SWITCHES)
# The per-edge last layer of low in-degree graphs forms W_e = W3 h_e on split-f16 operands (2^-22 of a block's
# largest magnitude where fp32 carries 2^-24): each message carries ~4 x the reference's rounding, and a node that sums many of
# them cancels it up.  Measured on the MI355X (mean in-degree <= 4, the in-edges gathered on a few destinations, no root / bias):
# err / e32 = 1.4 at a largest in-degree of ~11, 2.3 at ~50, 2.9 at ~85, 3.5 at ~157, 4.1 at ~290, 4.3 - 5.6 at 630 - 1040, where
# the re-associated path stays at 1.0 - 1.8.  With the default precision a call takes the per-edge last layer only up to
# EDGE_PATH_MAX_IN_DEGREE (the largest in-degree is recorded by build_csr: no device sync per call).
EDGE_PATH_MAX_IN_DEGREE = 64


def _fwd_flags(csr: "Csr", precision: Optional[str]) -> int:
    """GPDE_FWD_* flags of a forward call: the precision's, plus GPDE_FWD_NO_EDGE_PATH under the default precision when a node
    has more than EDGE_PATH_MAX_IN_DEGREE in-edges."""
    name = DEFAULT_PRECISION if precision is None else precision
    if name not in _PRECISION:
        raise ValueError(f"precision must be one of {_precision_choices()}, got {name!r}")
    flags = _PRECISION[name]
    if precision is None and (flags & _lib.GPDE_FWD_F16SPLIT) and csr.n_edges > 0 and csr.max_in_degree > EDGE_PATH_MAX_IN_DEGREE:
        flags |= _lib.GPDE_FWD_NO_EDGE_PATH
    return flags


def workspace_bytes(n_nodes: int, n_edges: int, pm: PackedMlp) -> int:
    return int(_lib.lib().gpde_nnconv_fwd_workspace_bytes(n_nodes, n_edges, len(pm.dims) - 1, pm.dims_c))


SAVE_Z_BYTES = int(float(os.environ.get("GPDE_SAVE_Z_GB", "16")) * (1 << 30))     # per call; 0 disables
SAVE_Z_RESERVE_BYTES = int(float(os.environ.get("GPDE_SAVE_Z_RESERVE_GB", "48")) * (1 << 30))   # device memory left free by a kept Z
SAVE_H_BYTES = int(float(os.environ.get("GPDE_SAVE_H_GB", "32")) * (1 << 30))     # kept hidden activations per call (keep_hidden); 0 disables
SAVE_H_MIN_EDGES = 262144                                                          # below: one fused launch beats store + aggregation


# Fraction of the free device memory a full backward's workspace may take for the ONE-CHUNK plan.  Default 0 = the library's default
# plan (~26 GB at k = 1024) since round 6: at s=121 one chunk asks for 125 GiB to be 2.5 % faster (105.5 vs 108.2 ms) - the wrong default
# on a device that also holds a DDP replica's optimizer state and 32 samples' graphs.  Opt in: GPDE_BWD_WS_FRACTION=0.6
BWD_WS_FRACTION = float(os.environ.get("GPDE_BWD_WS_FRACTION", "0"))


def bwd_workspace_bytes(lib, n: int, e: int, nl: int, dims_c, dev, h_given_bytes: int = 0) -> int:
    """Workspace of a full backward (gpde_nnconv_bwd*): the library's default (~26 GB at k = 1024: node-aligned chunks of
    ~640 k edges), or - opt-in, GPDE_BWD_WS_FRACTION > 0 - its one-chunk size when that is below that fraction of what the device has free - one chunk =
    fewer launches, GEMM tile rounds and split-K reductions (s=121, 5.9 M edges: 139.4 -> 135.5 ms).  All or nothing: sizes
    in between were tried (G241: one NNConv backward 2.57 -> 2.11 s with 0.6 of the free memory) and dropped - in a training
    run on a graph whose hidden activations take most of the device an odd-sized 40 GB block fragments torch's cache until
    the 27 GB workspace of the next application no longer fits (scripts/time_deferred.py g241: OOM in step 1)."""
    nbytes = int(lib.gpde_nnconv_bwd_workspace_bytes(n, e, nl, dims_c))
    if nbytes == 0:
        _lib.check(-2, "gpde_nnconv_bwd_workspace_bytes")
    if BWD_WS_FRACTION > 0:
        # (`h_given_bytes`: the last hidden activations come from the forward - gpde_nnconv_bwd's plan then leaves their
        # per-chunk buffer, E * K2P * 4 bytes in one chunk, out of the workspace)
        one = int(lib.gpde_nnconv_bwd_workspace_bytes_one_chunk(n, e, nl, dims_c)) - int(h_given_bytes)
        free, _ = device_free_bytes(dev)
        if nbytes < one <= int(BWD_WS_FRACTION * free):
            nbytes = one
    return nbytes


def bwd_plan(n_nodes: int, n_edges: int, dims: Sequence[int], ws_bytes: int, n_defer: int = 0, h_given: bool = False) -> dict:
    """The node chunking the native backward plans for `ws_bytes` of workspace (gpde_nnconv_bwd_plan, host only): edges and nodes
    per node-aligned chunk.  `n_defer` > 0: gpde_nnconv_bwd_deferred of that many applications; `h_given`: the last hidden
    activations of every edge come from the forward (nnconv_backward_raw's `hidden_saved`)."""
    ec, nc = ctypes.c_int64(), ctypes.c_int64()
    rc = _lib.lib().gpde_nnconv_bwd_plan(int(n_nodes), int(n_edges), len(dims) - 1, _lib.dims_array(dims), int(ws_bytes),
                                         int(n_defer), int(bool(h_given)), ctypes.byref(ec), ctypes.byref(nc))
    _lib.check(rc, "gpde_nnconv_bwd_plan")
    return {"edges_per_chunk": ec.value, "nodes_per_chunk": nc.value}


def device_free_bytes(dev):
    """(bytes an allocation can still get, device total): what the driver reports free PLUS what torch's caching allocator
    holds in freed blocks (it returns them to the driver when a large request needs the room) - after a training step the
    freed Z buffers and workspaces of the 241^2 graph are ~120 GB of such blocks, invisible to mem_get_info alone."""
    free, total = torch.cuda.mem_get_info(dev)
    cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    return free + max(0, cached), total


def alloc_bwd_ws(lib, n: int, e: int, nl: int, dims_c, dev, h_given_bytes: int = 0) -> torch.Tensor:
    """Workspace of a full backward.  The one-chunk size (`bwd_workspace_bytes`) is an optimisation worth ~3 %: its estimate of
    the free memory is racy (other ranks / processes on the device, torch's cached blocks), so when that allocation fails the
    library's default plan (~26 GB) is taken instead - BEFORE any cache is dropped; only the default size goes through
    `_alloc_ws`'s release-and-retry (a run that fitted with the default plan must keep fitting)."""
    nbytes = bwd_workspace_bytes(lib, n, e, nl, dims_c, dev, h_given_bytes)
    default = int(lib.gpde_nnconv_bwd_workspace_bytes(n, e, nl, dims_c))
    if nbytes > default:
        try:
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)
        except torch.OutOfMemoryError:
            global n_bwd_ws_fallbacks
            n_bwd_ws_fallbacks += 1
    return _alloc_ws(default, dev)


n_grad_hidden_accumulated = 0   # backward passes of applications sharing H that ADDED their dL/dH in the per-edge kernel (tests)
n_kept_hidden = 0           # training forwards that kept their last hidden activations for the backward (keep_hidden; tests)
n_bwd_ws_fallbacks = 0      # times the one-chunk workspace did not fit and the default plan ran (tests / diagnostics)


def _alloc_ws(nbytes: int, dev) -> torch.Tensor:
    """Workspace of a native call.  The hidden-activation / per-edge-weight caches may hold most of the device (their
    budget follows the HBM size: hidden_cache.budget_bytes) - they are recomputable, a workspace is not optional: when the
    allocation fails they are dropped and it is retried once."""
    try:
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    except torch.OutOfMemoryError:
        from . import hidden_cache
        if not hidden_cache.release_all():
            raise
        torch.cuda.empty_cache()
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def z_buffer(csr: Csr, dims: Sequence[int], device) -> Optional[torch.Tensor]:
    """Zeroed [N, 64 * K2P] buffer for the keep-Z forward (gpde_nnconv_fwd_keepz), or None when it does not pay / fit:
    the forward forms Z_i = sum_e x_j (x) h_e anyway and the backward's dW_3 needs exactly that - keeping it
    (256 KiB per node at k2 = 1024: 15 GB on the 241^2 graph) saves the backward one aggregation pass over the 4 KiB-per-edge
    hidden activations.  Graphs of low in-degree (the per-edge last layer, §3e) and buffers above GPDE_SAVE_Z_GB are skipped, and
    (round 4) large buffers are kept only while GPDE_SAVE_Z_RESERVE_GB of the device stay free afterwards.  Precision note: with
    a kept Z, dW_3 = sum_i gT_i (x) Z_i uses the forward's Z (split-f16 aggregation from 32768 edges on, ~2^-21 per product);
    without it the backward re-aggregates on fp32 MFMA - both inside the gradient tolerance (tests/test_gpu_bwd.py)."""
    nbytes = csr.n_nodes * WIDTH * hidden_width(dims) * 4
    if SAVE_Z_BYTES <= 0 or nbytes > SAVE_Z_BYTES or csr.n_edges < 32 * csr.n_nodes:
        return None
    if nbytes > (1 << 30):
        # large buffers (15 GB per call on the 241^2 graph, one per layer until its backward ran): kept only while the device
        # still has room for the backward's workspace afterwards - keeping Z is an optimisation, the workspace is not
        free, _ = device_free_bytes(device)
        if free - nbytes < SAVE_Z_RESERVE_BYTES:
            return None
    try:
        return torch.zeros(csr.n_nodes, WIDTH * hidden_width(dims), dtype=torch.float32, device=device)
    except torch.OutOfMemoryError:       # keeping Z is an optimisation: without it the backward re-aggregates
        return None


def keep_hidden(csr: Csr, dims: Sequence[int], device) -> bool:
    """Whether a training forward should KEEP the last hidden activations H_2 [E, K2P] (4 KiB per edge at k2 = 1024) for its own
    backward (round 5): forward = store kernel + aggregation from H (gpde_hidden_fwd, gpde_nnconv_fwd_keepz(hidden)), backward =
    gpde_nnconv_bwd with `hidden` - the hidden layer's K loop runs once per step instead of twice (s=121: forward 34.8 -> ~41 ms,
    backward 137 -> ~105 ms).  Only 3-Linear kernel MLPs on the split-f16 store kernel, graphs large enough for two launches not
    to matter, tensors up to GPDE_SAVE_H_GB (default 32) and only while GPDE_SAVE_Z_RESERVE_GB of the device stay free
    afterwards (the backward's workspace needs the room; keeping H is an optimisation)."""
    nbytes = csr.n_edges * hidden_width(dims) * 4
    if SAVE_H_BYTES <= 0 or nbytes > SAVE_H_BYTES or len(dims) != 4 or csr.n_edges < SAVE_H_MIN_EDGES or \
            DEFAULT_PRECISION != "f16split" or not 1 <= dims[0] <= 8 or (int(dims[1]) + 31) // 32 < 8 or \
            csr.n_edges < 32 * csr.n_nodes:          # (>= 8 k1 chunks: the one-wave-per-SIMD store kernel; low in-degree: §3e's path)
        return False
    free, _ = device_free_bytes(device)
    return free - nbytes >= SAVE_Z_RESERVE_BYTES


def _check_residual(residual, x, n):
    if residual is None:
        return None
    _require_cuda(residual, "residual")
    if residual.dtype != torch.float32 or tuple(residual.shape) != (n, WIDTH):
        raise ValueError(f"residual must be float32 [{n},{WIDTH}], got {residual.dtype} {tuple(residual.shape)}")
    return _operand(residual, "residual", (n, WIDTH), x.device)


def _root_bias(root, bias, dev):
    """The 64-wide update() parameters as operands: root float32 [64, 64], bias float32 [64]."""
    return (_operand(None if root is None else root.detach(), "root", (WIDTH, WIDTH), dev),
            _operand(None if bias is None else bias.detach(), "bias", (WIDTH,), dev))


def _out_ws(out, ws, n, dev):
    """A caller-given `out` [n, 64] / `ws` checked as written operands (None: the wrapper allocates)."""
    return (_operand(out, "out", (n, WIDTH), dev, writable=True),
            _operand(ws, "ws", (None,), dev, writable=True, dtype=torch.uint8))


def _attr_source(csr: "Csr", edge_attr, keep_rows: bool = False):
    """The attribute source of a native call: (`edge_attr` pointer, `node_attr` reference, `perm` pointer, what must stay alive
    during the call).  A NodeAttr goes by reference (GpdeNodeAttr) and leaves both pointers NULL; a tensor (already detached
    where the caller does not differentiate it) goes in CSR slot order with its permutation (`attr_in_slot_order`), or -
    `keep_rows` - in the caller's row order with the CSR's own `perm`; None: a call that reads no attributes."""
    if edge_attr is None:
        return None, None, None, None
    if isinstance(edge_attr, NodeAttr):
        nas = edge_attr.c_struct()
        return None, ctypes.byref(nas), None, (edge_attr, nas)
    if keep_rows:
        attr, perm = _dense16(edge_attr), csr.perm
    else:
        attr, perm = attr_in_slot_order(csr, _dense16(edge_attr))
    return attr.data_ptr(), None, perm.data_ptr(), (attr, perm)


def _forward64(label: str, x: torch.Tensor, csr: Csr, pm: PackedMlp, root, bias, aggr: str, flags: int, attr=None,
               hidden: Optional[torch.Tensor] = None, hmax: Optional[torch.Tensor] = None, hidden_nodes: Optional[int] = None,
               residual: Optional[torch.Tensor] = None, relu: bool = False, z_keep: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The one body of the 64-wide forward wrappers: one native call on the current stream.  `x` has passed its wrapper's own
    gate, `flags` is the wrapper's GPDE_FWD_* word, `label` its name in a library error.  `attr`: the attribute source - an
    [E, k0] tensor, a NodeAttr, or None (every node aggregates from H).  `hidden` / `hmax`: the last hidden activations and
    their max |H| scalar - with `hidden_nodes` None H of EVERY edge, with `hidden_nodes` = k the rows of the in-edges of
    nodes [0, k) only (the general entry point; k = 0: no H).  `residual` / `relu`: out = act(residual + NNConv(x)) in the
    last kernel; `z_keep` (zeros [N, 64 * K2P]): Z of every node is left there for the backward (`z_buffer`)."""
    _require_cuda(x, "x")
    if aggr not in _AGGR:
        raise NotImplementedError(f"aggr={aggr!r}: 'add' and 'mean' only")
    n, e, dev, k2p = csr.n_nodes, csr.n_edges, x.device, hidden_width(pm.dims)
    x = _operand(x, "x", (n, WIDTH), dev)
    if isinstance(attr, NodeAttr):
        _require_cuda(attr.table, "node table")
        if attr.table.size(0) != n or attr.k0 != pm.dims[0]:
            raise ValueError(f"node table must have {n} rows and {pm.dims[0]} slots")
    elif attr is not None:
        _require_cuda(attr, "edge_attr")
        if attr.dim() != 2 or attr.size(0) != e or attr.size(1) != pm.dims[0]:
            raise ValueError(f"edge_attr must be [{e},{pm.dims[0]}], got {tuple(attr.shape)}")
        if attr.device != dev:
            raise ValueError(f"edge_attr is on {attr.device}, x on {dev}")
        if attr.dtype != torch.float32:
            raise NotImplementedError(f"float32 only (got x {x.dtype}, edge_attr {attr.dtype})")
    general = hidden_nodes is not None or isinstance(attr, NodeAttr)         # gpde_nnconv_fwd_mixed_keepz
    if hidden_nodes is not None:             # a partial H: its rows end where the in-edges of node `hidden_nodes` begin
        hidden_nodes = max(int(hidden_nodes), 0)
        hidden = hidden if hidden_nodes > 0 else None
    if hidden is not None:
        _require_cuda(hidden, "hidden")
        hidden = _operand(hidden, "hidden", (e if hidden_nodes is None else int(csr.rowptr_host[hidden_nodes]), k2p), dev)
    attr_p, na_ref, perm_p, _alive = _attr_source(csr, attr)
    root_c, bias_c = _root_bias(root, bias, dev)
    out, ws = _out_ws(out, ws, n, dev)
    z_keep = _operand(z_keep, "z_keep", (n, WIDTH * k2p), dev, writable=True)
    residual = _check_residual(residual, x, n)
    glue = residual is not None or relu
    if z_keep is not None and glue:
        raise ValueError("z_keep cannot be combined with the fused glue")
    if general and glue:
        raise NotImplementedError("the fused glue with node-table attributes or a partial H is not built")
    if out is None:
        out = torch.empty(n, WIDTH, dtype=torch.float32, device=dev)
    if ws is None:
        ws = _alloc_ws(workspace_bytes(n, e, pm), dev)
    # the runs of arguments every entry point shares, in the header's order
    head = (x.data_ptr(), n)
    graph = (csr.rowptr.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr())
    mlp = (len(pm.dims) - 1, pm.dims_c, pm.packed.data_ptr(), _ptr(root_c), _ptr(bias_c), _AGGR[aggr])
    tail = (out.data_ptr(), ws.data_ptr(), ws.numel())
    act = (_ptr(residual), 1 if relu else 0)
    if general:
        name, args = "gpde_nnconv_fwd_mixed_keepz", (*head, attr_p, na_ref, _ptr(hidden), _ptr(hmax), hidden_nodes or 0, e, *graph, perm_p,
                                                     *mlp, flags, _ptr(z_keep), *tail)
    elif z_keep is not None:
        name, args = "gpde_nnconv_fwd_keepz", (*head, attr_p, _ptr(hidden), _ptr(hmax), e, *graph, perm_p, *mlp, flags, z_keep.data_ptr(), *tail)
    elif hidden is not None:
        name, args = "gpde_nnconv_fwd_hidden_act", (*head, hidden.data_ptr(), _ptr(hmax), e, *graph, *mlp, *act, *tail)
    elif glue:
        name, args = "gpde_nnconv_fwd_act", (*head, attr_p, e, *graph, perm_p, *mlp, flags, *act, *tail)
    else:
        name, args = "gpde_nnconv_fwd", (*head, attr_p, e, *graph, perm_p, *mlp, flags, *tail)
    _call(name, dev, *args, label=label)
    return out


def nnconv_forward_raw(x: torch.Tensor, csr: Csr, edge_attr: torch.Tensor, pm: PackedMlp,
                       root: Optional[torch.Tensor], bias: Optional[torch.Tensor], aggr: str,
                       out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                       precision: Optional[str] = None, residual: Optional[torch.Tensor] = None,
                       relu: bool = False, z_keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One gpde_nnconv_fwd call on the current stream. x [N,64] f32, edge_attr [E,k0] f32.
    `residual` / `relu` (opt-in): out = act(residual + NNConv(x)) in the last kernel
    (gpde_nnconv_fwd_act).  `z_keep` (zeros [N, 64 * K2P]): gpde_nnconv_fwd_keepz - Z of every node is left there for
    the backward (`z_buffer`)."""
    if isinstance(edge_attr, NodeAttr):         # attributes from node data (row f3): the training-side forward entry point
        if residual is not None or relu:
            raise NotImplementedError("the fused glue with node-table attributes is not built")
        return nnconv_forward_mixed_raw(x, csr, edge_attr, None, None, 0, pm, root, bias, aggr, precision=precision, z_keep=z_keep,
                                        out=out, ws=ws)
    if aggr not in _AGGR:
        raise NotImplementedError(
            f"aggr={aggr!r}: the fused MI355X operator implements 'add' and 'mean' (every reference "
            "script uses 'mean'); 'max' cannot use the re-associated contraction")
    flags = _fwd_flags(csr, precision)
    if x.dtype != torch.float32 or edge_attr.dtype != torch.float32:
        raise NotImplementedError(f"float32 only (got x {x.dtype}, edge_attr {edge_attr.dtype})")
    if x.dim() != 2 or x.size(1) != WIDTH:
        raise NotImplementedError(f"node features must be [N,{WIDTH}] (in_channels = out_channels = "
                                  f"{WIDTH}), got {tuple(x.shape)}")
    if x.size(0) != csr.n_nodes:
        raise ValueError(f"x has {x.size(0)} rows, CSR was built for {csr.n_nodes} nodes")
    return _forward64("gpde_nnconv_fwd", x, csr, pm, root, bias, aggr, flags, attr=edge_attr, residual=residual, relu=relu,
                      z_keep=z_keep, out=out, ws=ws)


class NodeAttr:
    """Edge attributes described by node data instead of an [E, k0] tensor (SURVEY.md §8 row f3,
    opt-in): slot d of edge (j -> i) is table[(i if endpoint_d else j), column_d].
    `NodeAttr.darcy(pos, a)` is the reference's recipe edge_attr = [pos_src, pos_dst, a_src, a_dst]
    (graph-neural-operator/utilities.py:274-277)."""

    def __init__(self, table: torch.Tensor, sel: Sequence[Tuple[int, int]]):
        if table.dim() != 2 or table.dtype != torch.float32:
            raise ValueError("node table must be float32 [N, columns]")
        if not 1 <= len(sel) <= 7:
            raise NotImplementedError("1..7 attribute slots")
        for ep, col in sel:
            if ep not in (0, 1) or not 0 <= col < table.size(1) or col > 255:
                raise ValueError(f"slot ({ep}, {col}): endpoint 0 = source / 1 = target, column < {table.size(1)}")
        if table.requires_grad and torch.is_grad_enabled():
            # a table that wants a gradient stays in the autograd graph (the module materialises the differentiable gather from
            # `self.table`): a view or an unaligned tensor is copied by a differentiable clone, never detached
            dense = table.is_contiguous() and table.data_ptr() % 16 == 0
            self.table = table if dense else table.clone(memory_format=torch.contiguous_format)
        else:
            self.table = _dense16(table)
        self.sel = [(int(ep), int(col)) for ep, col in sel]

    @staticmethod
    def darcy(pos: torch.Tensor, a: torch.Tensor) -> "NodeAttr":
        d = pos.size(1)
        table = torch.cat([pos.float(), a.float().reshape(-1, 1)], dim=1)
        sel = [(0, c) for c in range(d)] + [(1, c) for c in range(d)] + [(0, d), (1, d)]
        return NodeAttr(table, sel)

    @property
    def k0(self) -> int:
        return len(self.sel)

    # the little of a tensor's surface the module code asks of `edge_attr` (so that a NodeAttr travels the same code paths)
    dtype = torch.float32
    requires_grad = False

    def dim(self) -> int:
        return 2

    def detach(self) -> "NodeAttr":
        return self

    def contiguous(self) -> "NodeAttr":
        return self

    @property
    def is_cuda(self) -> bool:
        return self.table.is_cuda

    @property
    def device(self):
        return self.table.device

    def c_struct(self):
        """include/gpde.h GpdeNodeAttr, the `node_attr` argument of the entry points (keeps nothing alive: hold `self` during the call)."""
        na = _lib.GpdeNodeAttr()
        na.table, na.stride, na.n_slots = self.table.data_ptr(), int(self.table.size(1)), self.k0
        for d in range(8):
            ep, col = self.sel[min(d, self.k0 - 1)]
            na.sel[d] = (ep << 8) | col
        return na

    def materialize(self, edge_index: torch.Tensor) -> torch.Tensor:
        """The [E, k0] tensor the reference would have built (torch gather; for training / checks)."""
        cols = [self.table[edge_index[ep].long(), col] for ep, col in self.sel]
        return torch.stack(cols, dim=1)


def nnconv_forward_nodeattr_raw(x: torch.Tensor, csr: Csr, na: NodeAttr, pm: PackedMlp,
                                root: Optional[torch.Tensor], bias: Optional[torch.Tensor], aggr: str,
                                out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                                precision: Optional[str] = None) -> torch.Tensor:
    """The forward with edge attributes read from a node table (`node_attr` of gpde_nnconv_fwd_mixed_keepz, no kept H, no kept Z):
    nnconv_forward_mixed_raw without a partial H."""
    if na.table.size(0) != csr.n_nodes or na.k0 != pm.dims[0]:
        raise ValueError(f"node table must have {csr.n_nodes} rows and {pm.dims[0]} slots, got {na.table.size(0)} / {na.k0}")
    return nnconv_forward_mixed_raw(x, csr, na, None, None, 0, pm, root, bias, aggr, precision=precision, out=out, ws=ws)


# Precision policy of the forward: which ASSOCIATION a call's sum is computed in.  The fused operator re-associates
# sum_e x_j . (W3 h_e + b3) as (sum_e x_j (x) h_e) . W3: Z_i sums x_j h_e over the in-edges of node i.  When a
# node has more in-edges than the graph has nodes, its edges repeat sources, the Z sums of one source's positive
# activations grow with the in-degree instead of cancelling, and the fp32 rounding of Z, which the contraction with W3 then
# cancels down, reaches 4 - 18 x the reference's own fp32 error on the same inputs at in-degrees 1,000 - 8,000.  The
# arithmetic is not the cause: the fp32 MFMA kernel and the split-f16 kernels give the same error, and so does an fp32 CPU
# restatement of the re-associated sum.  Such calls take the reference's association instead: the per-edge weights
# W_e = nn(pseudo_e) (gpde_edge_weights_fwd) and one streaming message / aggregate / update kernel over them
# (gpde_nnconv_fwd_edgeweights).  Radius graphs have in-degrees far below their node count (the 241^2 grid:
# 1,793 of 58,081) and keep the fused kernels; the per-edge weights take 16 KiB per edge, so calls above
# PER_EDGE_MAX_EDGES edges keep them too.
PER_EDGE_MAX_EDGES = 1 << 17


def per_edge_association(csr: Csr, dims: Sequence[int], aggr: str) -> bool:
    """Whether a forward call of this graph and kernel MLP takes the reference's association (see above).  Host only:
    the in-degree was recorded when the CSR was built."""
    return aggr in ("add", "mean") and 0 < csr.n_edges <= PER_EDGE_MAX_EDGES and csr.max_in_degree > csr.n_nodes


def nnconv_forward_per_edge_raw(x: torch.Tensor, csr: Csr, edge_attr: torch.Tensor, pm: PackedMlp,
                                weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
                                root: Optional[torch.Tensor], bias: Optional[torch.Tensor], aggr: str) -> torch.Tensor:
    """The forward in the reference's association: hidden activations on fp32 MFMA (gpde_hidden_fwd), W_e = W3 h_e + b3
    per CSR slot (gpde_edge_weights_fwd), m_e = x_j . W_e summed per destination (gpde_nnconv_fwd_edgeweights)."""
    hidden, _ = hidden_forward_raw(csr, edge_attr.detach().contiguous(), pm, list(weights[:-1]) + [None],
                                   list(biases[:-1]) + [None], "f32")
    we = edge_weights_raw(hidden, pm, weights[-1], biases[-1])
    del hidden
    return nnconv_forward_edgeweights_raw(x.detach().contiguous(), csr, we, root, bias, aggr)


def forward_route(csr: Csr, pm: PackedMlp, aggr: str = "mean", precision: Optional[str] = None,
                  ws_bytes: Optional[int] = None) -> dict:
    """How NNConvFunction's forward of this graph runs (host-side queries, no device work): "association" is
    "per_edge" (per_edge_association) or "node" (the fused operator); for the latter "kernel" names the fused edge
    kernel, "edge_path" says whether the per-edge last layer of low in-degree graphs runs instead, "n_chunks" is
    the node chunking of the plan for `ws_bytes` (default: the recommended workspace), "attr_image" whether the fused
    kernel reads the per-call attribute operand image.  `precision` None: the default precision with its routing
    (EDGE_PATH_MAX_IN_DEGREE), as nnconv_forward_raw applies it."""
    if per_edge_association(csr, pm.dims, aggr):
        return {"association": "per_edge"}
    flags = _fwd_flags(csr, precision)
    precision = DEFAULT_PRECISION if precision is None else precision
    n, e = csr.n_nodes, csr.n_edges
    ws_bytes = workspace_bytes(n, e, pm) if ws_bytes is None else int(ws_bytes)
    rc = _lib.lib().gpde_nnconv_fwd_edge_path(n, e, len(pm.dims) - 1, pm.dims_c, flags, ws_bytes)
    if rc < 0:
        _lib.check(rc, "gpde_nnconv_fwd_edge_path")
    nch = ctypes.c_int32()
    img = _lib.lib().gpde_nnconv_fwd_attr_image(n, e, len(pm.dims) - 1, pm.dims_c, flags, ws_bytes, ctypes.byref(nch))
    if img < 0:
        _lib.check(img, "gpde_nnconv_fwd_attr_image")
    return {"association": "node", "kernel": fused_kernel_name(n, e, pm, precision), "edge_path": rc == 1,
            "n_chunks": nch.value, "attr_image": img == 1}


def launch_plan(n_nodes: int, n_edges: int, pm: PackedMlp, ws_bytes: int):
    lib = _lib.lib()
    nch, npc, wgs, mode = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    rc = lib.gpde_nnconv_fwd_plan(n_nodes, n_edges, len(pm.dims) - 1, pm.dims_c, ws_bytes,
                                  ctypes.byref(nch), ctypes.byref(npc), ctypes.byref(wgs),
                                  ctypes.byref(mode))
    _lib.check(rc, "gpde_nnconv_fwd_plan")
    img = lib.gpde_nnconv_fwd_attr_image(n_nodes, n_edges, len(pm.dims) - 1, pm.dims_c, _PRECISION[DEFAULT_PRECISION], ws_bytes, None)
    return {"n_chunks": nch.value, "nodes_per_chunk": npc.value, "fused_workgroups": wgs.value,
            "mode": mode.value, "attr_image": img == 1}


def fused_kernel_name(n_nodes: int, n_edges: int, pm: PackedMlp, precision: Optional[str] = None) -> str:
    """Symbol of the fused edge kernel a forward call of this size / arithmetic launches
    (gpde_nnconv_fwd_kernel).  `n_nodes` is accepted for symmetry with launch_plan and unused."""
    precision = DEFAULT_PRECISION if precision is None else precision
    return _lib.lib().gpde_nnconv_fwd_kernel(n_edges, len(pm.dims) - 1, pm.dims_c, _PRECISION[precision]).decode()


# ----------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------
_BWD64 = {          # phase (the names of _lib.BWD_TRACE_CODES["phase"]) -> (entry point, its label in a library error)
    "full": ("gpde_nnconv_bwd", None), "conv": ("gpde_nnconv_bwd", "gpde_nnconv_bwd (hidden given)"), "mlp": ("gpde_hidden_bwd", None),
    "light": ("gpde_nnconv_bwd_light", None), "deferred": ("gpde_nnconv_bwd_deferred", None)}


def _backward64(phase: str, csr: Csr, W, b, *, dims=None, x=None, edge_attr=None, keep_rows: bool = False, root=None, aggr=None,
                grad_out=None, grad_hidden_in=None, z_saved=None, hidden=None, hpart=None, hpart_nodes: int = 0, grad_hidden_out=None,
                n_defer: int = 0, x_stack=None, g_stack=None, need_root: bool = False, need_bias: bool = False, need_attr: bool = False,
                ws=None):
    """The one body of the 64-wide backward wrappers: one native call on the current stream.  `phase` names the stage of
    `bwd_impl` that runs, the keywords are the fields of `BwdArgs` (csrc/gpde_bwd.hip) a wrapper gives; each wrapper has raised
    its own refusals.  `W` / `b`: the Linear layers the phase reads - all of them ("full", "light", "deferred"), the hidden ones
    ("mlp"), or None in front of the last ("conv": `hidden` is H of every edge); `dims`: all widths where `W` does not tell them.
    `hidden` of "full" is the H its forward kept, `hpart` / `hpart_nodes` the partial H of the mixed forward, `grad_hidden_out` a
    tensor dL/dU is ADDED to ("conv").  Gradients are written for the last Linear ("light", "conv"), the hidden ones ("deferred",
    "mlp") or every layer ("full").  Returns (grad_x, grad_hidden, grad_attr, [grad_W], [grad_b], grad_root, grad_bias), None for
    what the phase does not write.

    The workspace: a caller-given `ws` ("full" takes one); else "full" allocates by `alloc_bwd_ws` for (n, e) less the bytes of a
    given H, "mlp" by `alloc_bwd_ws` for (0, e) - both may take the opt-in one-chunk size -, "light" and "conv" the size
    gpde_nnconv_bwd_workspace_bytes names and "deferred" that of gpde_nnconv_bwd_deferred_workspace_bytes for `n_defer`."""
    lib = _lib.lib()
    name, label = _BWD64[phase]
    for t, nm in ((x, "x"), (edge_attr, "edge_attr"), (hidden, "hidden"), (grad_out, "grad_out"), (grad_hidden_in, "grad_hidden")):
        if t is not None:
            _require_cuda(t, nm)
    n, e, dev = csr.n_nodes, csr.n_edges, (edge_attr if x is None else x).device
    x = _operand(None if x is None else x.detach(), "x", (n, WIDTH), dev)
    grad_out = _operand(None if grad_out is None else grad_out.detach().float(), "grad_out", (n, WIDTH), dev)
    if phase == "conv":                                    # the arrays carry their LAST entries only, under their own names
        dims_c = _lib.dims_array(dims)
        front = [None] * (len(dims) - 2)
        W = front + [_operand(W[-1].detach(), "w_last", (WIDTH * WIDTH, dims[-2]), dev)]
        b = front + [_operand(None if b[-1] is None else b[-1].detach(), "b_last", (WIDTH * WIDTH,), dev)]
    else:
        dims, dims_c, W, b = _mlp_operands(W, b, dev, dims)
    nl, k2p = len(dims) - 1, hidden_width(dims)
    W, b = W + [None] * (nl - len(W)), b + [None] * (nl - len(b))
    root_c, _ = _root_bias(root, None, dev)
    z_saved = _operand(z_saved, "z_saved", (n, WIDTH * k2p), dev)
    hidden = _operand(None if hidden is None else hidden.detach(), "hidden" if phase == "conv" else "hidden_saved", (e, k2p), dev)
    hpart = _operand(hpart, "hidden_part", (None, k2p), dev)
    grad_hidden_in = _operand(None if grad_hidden_in is None else grad_hidden_in.detach(), "grad_hidden", (e, k2p), dev)
    accumulate = grad_hidden_out is not None
    gh = _operand(grad_hidden_out, "grad_hidden_acc", (e, k2p), dev, writable=True)
    ws = _operand(ws, "ws", (None,), dev, writable=True, dtype=torch.uint8)
    attr_p, na_ref, perm_p, _alive = _attr_source(csr, None if edge_attr is None else edge_attr.detach(), keep_rows=keep_rows)
    # the gradients
    wanted = {"full": range(nl), "light": (nl - 1,), "conv": (nl - 1,), "deferred": range(nl - 1), "mlp": range(nl - 1)}[phase]
    gW = [torch.empty_like(W[l]) if l in wanted else None for l in range(nl)]
    gb = [torch.empty_like(b[l]) if l in wanted and b[l] is not None else None for l in range(nl)]
    gx = None if x is None else torch.empty(n, WIDTH, dtype=torch.float32, device=dev)
    if phase == "conv" and gh is None:
        gh = torch.empty_like(hidden)
    groot, gbias = _update_grads(root, need_root, need_bias, dev)
    ga = torch.zeros(e, dims[0], dtype=torch.float32, device=dev) if need_attr else None
    grads = (gx, gh, ga, gW, gb, groot, gbias)
    if phase == "full" and n == 0:
        # a graph without nodes (message() of an edgeless graph runs the operator on E = 0 one-edge graphs): every sum is empty
        for t in gW + gb + [groot, gbias]:
            if t is not None:
                t.zero_()
        return grads
    if ws is not None:
        pass
    elif phase in ("full", "mlp"):
        ws = alloc_bwd_ws(lib, n if phase == "full" else 0, e, nl, dims_c, dev, 0 if hidden is None else e * k2p * 4)
    elif phase == "deferred":
        ws = _queried_ws("gpde_nnconv_bwd_deferred_workspace_bytes", dev, n, e, nl, dims_c, n_defer)
    else:
        ws = _queried_ws("gpde_nnconv_bwd_workspace_bytes", dev, n, e, nl, dims_c)
    # the runs of arguments the entry points share, in the header's order
    attr = (attr_p, na_ref)
    mlp = (nl, dims_c, _ptr_array(W), _ptr_array(b))
    tail = (ws.data_ptr(), ws.numel())
    if phase == "mlp":
        args = (*attr, e, perm_p, csr.src.data_ptr(), csr.dst.data_ptr(), *mlp, grad_hidden_in.data_ptr(), _ptr_array(gW), _ptr_array(gb), *tail)
    else:
        graph = (e, csr.rowptr.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), perm_p, csr.rowptr_host.data_ptr())
        hp = (_ptr(hpart) if hpart_nodes > 0 else None, int(hpart_nodes) if hpart is not None else 0)
        if phase == "deferred":
            args = (x_stack.data_ptr(), g_stack.data_ptr(), n_defer, n, *attr, *graph, *mlp, _AGGR[aggr], *hp, _ptr_array(gW), _ptr_array(gb), *tail)
        else:
            srp, ssl = csr.src_order
            node = (_ptr(srp), _ptr(ssl), *mlp, _ptr(root_c), _AGGR[aggr], grad_out.data_ptr(), _ptr(z_saved))
            if phase == "light":
                args = (x.data_ptr(), n, *attr, *graph, *node, *hp, gx.data_ptr(), gW[-1].data_ptr(), _ptr(gb[-1]), _ptr(groot), _ptr(gbias), *tail)
            else:
                args = (x.data_ptr(), n, *attr, _ptr(hidden), *graph, *node, gx.data_ptr(), _ptr(gh), _ptr(ga), _ptr_array(gW), _ptr_array(gb),
                        _ptr(groot), _ptr(gbias), _lib.GPDE_BWD_ACCUMULATE_GRAD_HIDDEN if accumulate else 0, *tail)
    _call(name, dev, *args, label=label)
    return grads


def nnconv_backward_raw(x: torch.Tensor, csr: Csr, edge_attr: torch.Tensor,
                        weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
                        root: Optional[torch.Tensor], aggr: str, grad_out: torch.Tensor,
                        need_root: bool = True, need_bias: bool = True,
                        ws: Optional[torch.Tensor] = None, z_saved: Optional[torch.Tensor] = None, need_attr: bool = False,
                        hidden_saved: Optional[torch.Tensor] = None):
    """One gpde_nnconv_bwd call on the current stream (`z_saved`: the keep-Z forward's buffer; `edge_attr`: a tensor or a NodeAttr;
    `hidden_saved`: the last hidden activations [E, K2P] the forward kept (hidden_forward_raw) - read instead of recomputed).
    Returns (grad_x, [grad_W_l], [grad_b_l or None], grad_root or None, grad_bias or None); with `need_attr` a sixth element,
    dL/d edge_attr [E, k0] in the caller's edge order (`grad_edge_attr` of the call)."""
    if aggr not in _AGGR:
        raise NotImplementedError(f"aggr={aggr!r}")
    dims = _mlp_dims(weights)
    if need_attr and (isinstance(edge_attr, NodeAttr) or dims[0] > 8):
        raise NotImplementedError("the edge-attribute gradient is built for attribute tensors of <= 8 slots")
    e, k2p = csr.n_edges, hidden_width(dims)
    if hidden_saved is not None and (need_attr or hidden_saved.dtype != torch.float32 or tuple(hidden_saved.shape) != (e, k2p)):
        raise ValueError(f"hidden_saved must be float32 [{e},{k2p}] (and excludes need_attr)")
    # (`need_attr`: the attributes stay in the caller's rows - the gradient goes back by perm)
    gx, _, ga, gW, gb, groot, gbias = _backward64("full", csr, weights, biases, x=x, edge_attr=edge_attr, keep_rows=need_attr, root=root,
                                                  aggr=aggr, grad_out=grad_out, z_saved=z_saved, hidden=hidden_saved, need_root=need_root,
                                                  need_bias=need_bias, need_attr=need_attr, ws=ws)
    return (gx, gW, gb, groot, gbias, ga) if need_attr else (gx, gW, gb, groot, gbias)


# ----------------------------------------------------------------------------------------------
# depth-deferred backward (include/gpde.h gpde_nnconv_bwd_light / gpde_nnconv_bwd_deferred)
# ----------------------------------------------------------------------------------------------
def deferred_supported(dims: Sequence[int]) -> bool:
    """Whether the kernel MLP `dims` = [k0, k1, k2, 4096] is in the depth-deferred form (gpde_nnconv_bwd_deferred_supported)."""
    return bool(_lib.lib().gpde_nnconv_bwd_deferred_supported(len(dims) - 1, _lib.dims_array(dims)))


def nodeattr_train_supported(dims: Sequence[int]) -> bool:
    """Training with node-table attributes (the `node_attr` argument): 3-Linear kernel MLPs on the one-wave-per-SIMD kernels
    (>= 8 chunks of 32 first-layer units), <= 7 attribute slots, and the split-f16 backward GEMMs (deferred_supported)."""
    return len(dims) == 4 and 1 <= dims[0] <= 7 and (int(dims[1]) + 31) // 32 >= 8 and deferred_supported(dims) and \
        DEFAULT_PRECISION == "f16split"


def deferred_layers_padded(n_defer: int) -> int:
    """Lp of include/gpde.h: layers of the x stack handed to gpde_nnconv_bwd_deferred (zero layers appended)."""
    return max(4, (n_defer + 1) // 2 * 2)


def nnconv_backward_light_raw(x: torch.Tensor, csr: Csr, edge_attr: torch.Tensor,
                              weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
                              root: Optional[torch.Tensor], aggr: str, grad_out: torch.Tensor,
                              need_root: bool = True, need_bias: bool = True, z_saved: Optional[torch.Tensor] = None,
                              hidden_part: Optional[torch.Tensor] = None, hidden_nodes: int = 0):
    """gpde_nnconv_bwd_light: one application of a depth-shared module - grad_x, the last Linear's gradients, grad_root,
    grad_bias; the hidden layers' gradients come from nnconv_backward_deferred_raw.  `hidden_part` / `hidden_nodes`: the
    partial H of the mixed forward (rows of the in-edges of nodes [0, hidden_nodes)): read instead of recomputed.
    Returns (grad_x, grad_w_last, grad_b_last or None, grad_root or None, grad_bias or None)."""
    if aggr not in _AGGR:
        raise NotImplementedError(f"aggr={aggr!r}")
    gx, _, _, gW, gb, groot, gbias = _backward64("light", csr, weights, biases, x=x, edge_attr=edge_attr, root=root, aggr=aggr,
                                                 grad_out=grad_out, z_saved=z_saved, hpart=hidden_part, hpart_nodes=hidden_nodes,
                                                 need_root=need_root, need_bias=need_bias)
    return gx, gW[-1], gb[-1], groot, gbias


def nnconv_backward_deferred_raw(xs: Sequence[torch.Tensor], gs: Sequence[torch.Tensor], csr: Csr, edge_attr: torch.Tensor,
                                 weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]], aggr: str,
                                 hidden_part: Optional[torch.Tensor] = None, hidden_nodes: int = 0):
    """gpde_nnconv_bwd_deferred: the hidden layers' gradients of ALL the applications (xs[l], gs[l]) = (input, output
    gradient) of a depth-shared module, in one pass over the edges.  `weights` / `biases`: ALL Linear layers (the last one
    is read, not differentiated).  Returns ([grad_W_l], [grad_b_l or None]) for the hidden layers."""
    L = len(xs)
    if L < 1 or len(gs) != L:
        raise ValueError("one (input, output gradient) pair per deferred application")
    n, dev = csr.n_nodes, edge_attr.device
    x_stack = torch.zeros(deferred_layers_padded(L), n, WIDTH, dtype=torch.float32, device=dev)      # (zero layers appended)
    g_stack = torch.empty(L, n, WIDTH, dtype=torch.float32, device=dev)
    for l in range(L):
        x_stack[l].copy_(_operand(xs[l].detach(), f"xs[{l}]", (n, WIDTH), dev))
        g_stack[l].copy_(_operand(gs[l].detach().float(), f"gs[{l}]", (n, WIDTH), dev))
    _, _, _, gW, gb, _, _ = _backward64("deferred", csr, weights, biases, edge_attr=edge_attr, aggr=aggr, hpart=hidden_part,
                                        hpart_nodes=hidden_nodes, n_defer=L, x_stack=x_stack, g_stack=g_stack)
    return gW[:-1], gb[:-1]



# ----------------------------------------------------------------------------------------------
# cross-depth reuse of the hidden activations (include/gpde.h gpde_hidden_*)
# ----------------------------------------------------------------------------------------------
def hidden_width(dims: Sequence[int]) -> int:
    """K2P: padded width of the last hidden layer (row stride of the hidden-activation tensor)."""
    return (int(dims[-2]) + 127) // 128 * 128


def hidden_forward_raw(csr: Csr, edge_attr: torch.Tensor, pm: PackedMlp,
                       weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
                       precision: Optional[str] = None, n_nodes_limit: Optional[int] = None) -> torch.Tensor:
    """gpde_hidden_fwd: H [E, K2P] (rows in CSR order) = all Linear+ReLU layers but the last one.
    Returns (H, hmax): hmax = device scalar max |H| when the fused kernel recorded it, else None."""
    lib = _lib.lib()
    _require_cuda(edge_attr, "edge_attr")
    precision = DEFAULT_PRECISION if precision is None else precision
    if precision not in _PRECISION:
        raise ValueError(f"precision must be one of {_precision_choices()}, got {precision!r}")
    e, dev, nl, flags = csr.n_edges, edge_attr.device, len(pm.dims) - 1, _PRECISION[precision]
    is_na = isinstance(edge_attr, NodeAttr)
    if not is_na and (edge_attr.dtype != torch.float32 or edge_attr.dim() != 2 or edge_attr.size(0) != e or
                      edge_attr.size(1) != pm.dims[0]):
        raise ValueError(f"edge_attr must be float32 [{e},{pm.dims[0]}], got {edge_attr.dtype} {tuple(edge_attr.shape)}")
    attr_p, na_ref, perm_p, _alive = _attr_source(csr, edge_attr.detach())
    n_lim = csr.n_nodes
    if n_nodes_limit is not None:           # H of the in-edges of nodes [0, n_nodes_limit) only (mixed forward)
        n_lim = int(n_nodes_limit)
        e = int(csr.rowptr_host[n_lim])
    hidden = torch.empty(e, hidden_width(pm.dims), dtype=torch.float32, device=dev)
    if is_na:
        # a node table runs the fused store kernel only: it reads the endpoints of every slot and the packed weights, no workspace
        fast, ends, wa, ba, ws = True, (csr.src.data_ptr(), csr.dst.data_ptr()), None, None, None
    else:
        _, _, ws_, bs_ = _mlp_operands(weights, biases, dev, pm.dims)       # last entry unused
        ends, wa, ba = (None, None), _ptr_array(ws_), _ptr_array(bs_)
        nbytes = int(lib.gpde_hidden_workspace_bytes(e, nl, pm.dims_c))
        fast = (flags & _lib.GPDE_FWD_F16SPLIT) and nl == 3
        ws = torch.empty(1 if fast else max(nbytes, 1), dtype=torch.uint8, device=dev)
    hmax = torch.zeros(1, dtype=torch.float32, device=dev) if fast else None

    def call(hmax, ws):
        return lib.gpde_hidden_fwd(attr_p, na_ref, e, csr.rowptr.data_ptr(), n_lim, perm_p, *ends, nl, pm.dims_c, pm.packed.data_ptr(),
                                   wa, ba, flags, hidden.data_ptr(), _ptr(hmax), _ptr(ws), 0 if ws is None else ws.numel(),
                                   _stream_ptr(dev))
    with torch.cuda.device(dev):
        rc = call(hmax, ws)
        if rc in (-1, -3) and fast and not is_na:    # shape not covered by the fused kernel: the general path needs ws
            hmax = None                              # ... and does not record max |H|
            rc = call(hmax, _alloc_ws(nbytes, dev))
    _lib.check(rc, "gpde_hidden_fwd (node table)" if is_na else "gpde_hidden_fwd")
    _lib.n_native_calls += 1
    return hidden, hmax


def nnconv_forward_hidden_raw(x: torch.Tensor, csr: Csr, hidden: torch.Tensor, pm: PackedMlp,
                              root: Optional[torch.Tensor], bias: Optional[torch.Tensor], aggr: str,
                              out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                              hmax: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                              relu: bool = False, z_keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gpde_nnconv_fwd_hidden: aggregation + last Linear + update() from given hidden activations
    (`hmax`: the max |H| scalar hidden_forward_raw returned; enables the split-f16 aggregation)."""
    n = csr.n_nodes
    if x.dtype != torch.float32 or x.dim() != 2 or x.size(1) != WIDTH or x.size(0) != n:
        raise ValueError(f"x must be float32 [{n},{WIDTH}], got {x.dtype} {tuple(x.shape)}")
    return _forward64("gpde_nnconv_fwd_hidden" if z_keep is None else "gpde_nnconv_fwd_keepz", x, csr, pm, root, bias, aggr, 0,
                      hidden=hidden, hmax=hmax, residual=residual, relu=relu, z_keep=z_keep, out=out, ws=ws)


# ----------------------------------------------------------------------------------------------
# the operator given the per-edge weights (include/gpde.h gpde_edge_weights_fwd / gpde_nnconv_fwd_edgeweights_group)
# ----------------------------------------------------------------------------------------------
EDGE_WEIGHT_BYTES = WIDTH * WIDTH * 4         # 16 KiB per edge


def edge_weights_raw(hidden: torch.Tensor, pm: PackedMlp, w_last: torch.Tensor, b_last: Optional[torch.Tensor]) -> torch.Tensor:
    """gpde_edge_weights_fwd: W_e = view(nn(pseudo_e), 64, 64) for every CSR slot ([E, 4096] fp32, the last Linear's
    bias folded in) from the hidden activations of hidden_forward_raw - the reference's nn_conv.py:274 tensor, built
    once per (edge_attr, weights) instead of once per call."""
    lib = _lib.lib()
    _require_cuda(hidden, "hidden")
    e, dev = int(hidden.size(0)), hidden.device
    if hidden.dim() != 2:
        raise ValueError(f"hidden must be float32 [E,{hidden_width(pm.dims)}]")
    hidden = _operand(hidden.detach(), "hidden", (e, hidden_width(pm.dims)), dev)
    w_c = _operand(w_last.detach(), "w_last", (WIDTH * WIDTH, pm.dims[-2]), dev)
    b_c = _operand(None if b_last is None else b_last.detach(), "b_last", (WIDTH * WIDTH,), dev)
    we = torch.empty(e, WIDTH * WIDTH, dtype=torch.float32, device=dev)
    nl = len(pm.dims) - 1
    ws = torch.empty(max(int(lib.gpde_edge_weights_workspace_bytes(e, nl, pm.dims_c)), 1), dtype=torch.uint8, device=dev)
    _call("gpde_edge_weights_fwd", dev, hidden.data_ptr(), e, nl, pm.dims_c, pm.packed.data_ptr(), w_c.data_ptr(), _ptr(b_c), we.data_ptr(),
          ws.data_ptr(), ws.numel())
    return we


_AGGR_WE = {"add": _lib.GPDE_AGGR_ADD, "mean": _lib.GPDE_AGGR_MEAN, "max": _lib.GPDE_AGGR_MAX}


def nnconv_forward_edgeweights_group(calls: Sequence[dict]) -> List[torch.Tensor]:
    """gpde_nnconv_fwd_edgeweights_group: INDEPENDENT NNConv calls, each given its per-edge weights, in one launch per
    16 calls.  Every call is a dict: x [N,64], csr, edge_weights [E,4096], root, bias, aggr ('add' | 'mean' | 'max'),
    optional residual [N,64], relu (bool), out.  Returns the outputs in order."""
    if not calls:
        return []
    dev = calls[0]["x"].device
    descs = (_lib.GpdeWeConvDesc * len(calls))()
    outs, keep = [], []
    for k, c in enumerate(calls):
        x, csr, we = c["x"], c["csr"], c["edge_weights"]
        _require_cuda(x, "x")
        n, e = csr.n_nodes, csr.n_edges
        if x.device != dev:
            raise ValueError("all calls of a group must live on one device")
        if x.dtype != torch.float32 or x.dim() != 2 or tuple(x.shape) != (n, WIDTH):
            raise ValueError(f"x must be float32 [{n},{WIDTH}], got {x.dtype} {tuple(x.shape)}")
        we = _operand(we.detach(), "edge_weights", (e, WIDTH * WIDTH), dev)
        aggr = c.get("aggr", "mean")
        if aggr not in _AGGR_WE:
            raise NotImplementedError(f"aggr={aggr!r}")
        x_c = _operand(x.detach(), "x", (n, WIDTH), dev)
        root_c, bias_c = _root_bias(c.get("root"), c.get("bias"), dev)
        res = _check_residual(c.get("residual"), x_c, n)
        out = _operand(c.get("out"), "out", (n, WIDTH), dev, writable=True)
        if out is None:
            out = torch.empty(n, WIDTH, dtype=torch.float32, device=dev)
        keep.append((x_c, root_c, bias_c, res, we, csr))
        outs.append(out)
        d = descs[k]
        d.x, d.edge_weights, d.rowptr, d.src = x_c.data_ptr(), we.data_ptr(), csr.rowptr.data_ptr(), csr.src.data_ptr()
        d.root, d.bias, d.residual = _ptr(root_c), _ptr(bias_c), _ptr(res)
        d.out, d.n_nodes, d.aggr, d.relu, d.reserved = out.data_ptr(), n, _AGGR_WE[aggr], 1 if c.get("relu") else 0, 0
    _call("gpde_nnconv_fwd_edgeweights_group", dev, descs, len(calls), calls=len(calls))
    return outs


def nnconv_forward_edgeweights_raw(x, csr, edge_weights, root, bias, aggr, residual=None, relu=False, out=None):
    """One call of the group entry point."""
    return nnconv_forward_edgeweights_group([dict(x=x, csr=csr, edge_weights=edge_weights, root=root, bias=bias, aggr=aggr,
                                                  residual=residual, relu=relu, out=out)])[0]


def nnconv_backward_edgeweights_raw(x: torch.Tensor, csr: Csr, edge_weights: torch.Tensor, root: Optional[torch.Tensor], aggr: str,
                                    grad_out: torch.Tensor, need_root: bool = True, need_bias: bool = True, acc=None):
    """gpde_nnconv_bwd_edgeweights(_acc): backward of the operator given the per-edge weights.  Returns (grad_x,
    grad_edge_weights [E, 4096], grad_root or None, grad_bias or None).  `acc` = (grad_edge_weights, grad_root or None, grad_bias
    or None) of an earlier application of the same backward pass: this call ADDS to them in the kernels and returns them."""
    lib = _lib.lib()
    for t, nm in ((x, "x"), (edge_weights, "edge_weights"), (grad_out, "grad_out")):
        _require_cuda(t, nm)
    if aggr not in _AGGR:
        raise NotImplementedError(f"aggr={aggr!r}: the gradient of the per-edge weight operator is built for 'add' and 'mean'")
    n, e, dev = csr.n_nodes, csr.n_edges, x.device
    x = _operand(x.detach(), "x", (n, WIDTH), dev)
    grad_out = _operand(grad_out.detach().float(), "grad_out", (n, WIDTH), dev)
    we = _operand(edge_weights.detach(), "edge_weights", (e, WIDTH * WIDTH), dev)
    root_c, _ = _root_bias(root, None, dev)
    gx = torch.empty(n, WIDTH, dtype=torch.float32, device=dev)
    want_root = need_root and root is not None
    bits = 0
    if acc is not None:
        gwe, groot, gbias = acc
        if (groot is not None) != want_root or (gbias is not None) != bool(need_bias):
            raise ValueError("acc: (grad_edge_weights [E,4096], grad_root, grad_bias) of an application of the same module expected")
        gwe = _operand(gwe, "acc[0] (grad_edge_weights)", (e, WIDTH * WIDTH), dev, writable=True)
        groot = _operand(groot, "acc[1] (grad_root)", (WIDTH, WIDTH), dev, writable=True)
        gbias = _operand(gbias, "acc[2] (grad_bias)", (WIDTH,), dev, writable=True)
        bits = _lib.GPDE_ACC_EDGE_WEIGHTS | (_lib.GPDE_ACC_ROOT if want_root else 0) | (_lib.GPDE_ACC_BIAS if need_bias else 0)
    else:
        gwe = torch.empty(e, WIDTH * WIDTH, dtype=torch.float32, device=dev)
        groot, gbias = _update_grads(root, need_root, need_bias, dev)
    ws = _alloc_ws(int(lib.gpde_nnconv_bwd_edgeweights_workspace_bytes(n, e)), dev)
    srp, ssl = csr.src_order
    _call("gpde_nnconv_bwd_edgeweights_acc", dev, x.data_ptr(), n, we.data_ptr(), e, csr.rowptr.data_ptr(), csr.src.data_ptr(), _ptr(srp), _ptr(ssl),
          _ptr(root_c), _AGGR[aggr], grad_out.data_ptr(), gx.data_ptr(), gwe.data_ptr(), _ptr(groot), _ptr(gbias), bits, ws.data_ptr(), ws.numel())
    return gx, gwe, groot, gbias


# ... at any width (include/gpde.h gpde_nnconv_fwd_edgeweights_any / gpde_nnconv_bwd_edgeweights_any; csrc/gpde_weconv_any.hip)
ANY_MAX_WIDTH = _lib.GPDE_WECONV_ANY_MAX_WIDTH


def width_supported(in_channels, out_channels) -> bool:
    """Whether `in_channels -> out_channels` is a width the native operator runs: 64 -> 64 on every path, any other pair of
    1 .. ANY_MAX_WIDTH (256) on the per-edge-weight kernels of gpde_weconv_any.hip."""
    try:
        i, o = int(in_channels), int(out_channels)
    except (TypeError, ValueError):
        return False
    return i == in_channels and o == out_channels and 1 <= i <= ANY_MAX_WIDTH and 1 <= o <= ANY_MAX_WIDTH


def any_width_plan(in_channels: int, out_channels: int, aligned: bool = True, aggr: str = "add") -> dict:
    """gpde_nnconv_edgeweights_any_plan: the lane tiling the any-width kernels run at these widths - V (floats per column access),
    LC (column lanes), R (row lanes), ES (edge slots per wave), B (x_j batches per pass: a pass is B * ES in-edges) and the lanes
    in use.  `aligned`: every buffer of the call is 16-byte aligned (else V = 1 at every width).  Host arithmetic, no device."""
    if aggr not in _AGGR_WE:
        raise NotImplementedError(f"aggr={aggr!r}")
    out = (ctypes.c_int32 * 6)()
    _lib.check(_lib.lib().gpde_nnconv_edgeweights_any_plan(int(in_channels), int(out_channels), 1 if aligned else 0, _AGGR_WE[aggr], out),
               "gpde_nnconv_edgeweights_any_plan")
    return dict(zip(("V", "LC", "R", "ES", "B", "lanes"), (int(v) for v in out)))


# ... re-associated at any width (include/gpde.h gpde_nnconv_fwd_hidden_any / gpde_nnconv_bwd_hidden_any; csrc/gpde_reassoc_any.hip):
# the last hidden activations [E, K] instead of the per-edge weights [E, in * out]
ANY_MAX_HIDDEN = _lib.GPDE_REASSOC_ANY_MAX_HIDDEN
ANY_REASSOC = os.environ.get("GPDE_ANY_REASSOC", "auto")      # auto | on | off | streamed: which any-width calls take the re-associated route
_ANY_PREF_Z_BYTES = 512 << 20        # Z' of the library's preferred node block (RA_PREF_Z_BYTES of gpde_reassoc_any.hip; tests/test_reassoc_host.py
#                                      holds the two together through the workspace query)
ANY_WS_FRACTION = 0.5                # a call of the re-associated route takes at most this share of the free memory as workspace
CHAIN_ANY_MIN_LINEAR, CHAIN_ANY_MAX_LINEAR, CHAIN_ANY_MAX_K0 = 2, 5, 64      # the chains gpde_chain_any.hip generates
CHAIN_ANY_PREF_BUDGET = 256 << 20    # per-edge buffers of one node block of the streamed route, when the free memory allows


def _hidden_any_ws_bytes(query, n: int, e: int, cin: int, cout: int, k: int, dev) -> int:
    """Workspace of a re-associated any-width call: the library's preferred size when ANY_WS_FRACTION of the free memory holds it,
    else that share (more node blocks of fewer nodes), never less than one node's worth.  `auto` takes this route only when memory
    is short, and the backward's workspace holds more than any_width_route's `bytes_reassociated` counts: P and dP (the last Linear,
    in * KP * out floats each) and the per-edge dx rows [E, in] next to Z' and dZ' of the node block."""
    pref, one = int(query(n, e, cin, cout, k)), int(query(1, e, cin, cout, k))
    free, _ = device_free_bytes(dev)
    return max(one, min(pref, int(free * ANY_WS_FRACTION)))


def chain_any_supported(dims) -> bool:
    """Whether a Linear / ReLU chain of widths `dims` = [k0, K_1, .., K_{n-1}, in * out] is one the streamed route generates
    (gpde_nnconv_*_chain_any: 2 .. 5 Linears, 1 <= k0 <= 64, hidden widths 1 .. ANY_MAX_HIDDEN)."""
    if dims is None:
        return False
    dims = [int(v) for v in dims]
    return CHAIN_ANY_MIN_LINEAR <= len(dims) - 1 <= CHAIN_ANY_MAX_LINEAR and 1 <= dims[0] <= CHAIN_ANY_MAX_K0 and \
        all(1 <= v <= ANY_MAX_HIDDEN for v in dims[1:-1])


def chain_edge_bytes(dims, acts=None) -> int:
    """Bytes per hidden row of a backward block of the streamed route (the plan's budget is spent in these): every kept H_l, the U_l
    of the layers whose act' needs it, dH and two dU buffers, rows padded to 4 floats."""
    kp = [(int(v) + 3) // 4 * 4 for v in dims[1:-1]]
    extra = 0 if acts is None else sum(p for p, a in zip(kp, acts) if int(a[0]) in ACT_FROM_U)
    return (sum(kp) + extra + kp[-1] + 2 * max(kp)) * 4


def _act_chain_route(n, e, cin, cout, k, free_bytes, mode, dims, acts) -> dict:
    """any_width_route for a chain with a hidden activation other than the ReLU (its docstring states the rule)."""
    bytes_m = e * cin * cout * 4
    zrow = cin * ((k + 1 + 3) // 4 * 4) * 4
    out = {"eligible": False, "eligible_streamed": dims is None or chain_any_supported(dims), "bytes_materialised": bytes_m,
           "bytes_reassociated": None, "node_block": None, "flops_materialised": 2 * e * k * cin * cout, "flops_reassociated": None,
           "bytes_streamed": None}
    fits_m = 2 * bytes_m <= free_bytes
    if out["eligible_streamed"]:
        out["bytes_streamed"] = e * cin * 4 + 2 * zrow * ((cout + 3) // 4 * 4)
        if dims is not None:
            per_edge = chain_edge_bytes(dims, acts)
            out["bytes_streamed"] += min(e, CHAIN_ANY_PREF_BUDGET // per_edge) * (per_edge - chain_edge_bytes(dims))
    if mode == "streamed" and out["eligible_streamed"]:
        out["route"] = "streamed"
    elif fits_m:
        out["route"] = "materialised"
    elif mode == "auto" and out["eligible_streamed"] and 2 * out["bytes_streamed"] <= free_bytes:
        out["route"] = "streamed"
    else:
        out["route"] = "refused"
    return out


def any_width_route(n_nodes: int, n_edges: int, in_channels: int, out_channels: int, k_hidden: Optional[int], aggr: str, chain: bool,
                    free_bytes: int, mode: Optional[str] = None, dims=None, acts=None) -> dict:
    """Which route a call of a module whose widths are not (64, 64) takes.  Host arithmetic only.

    `materialised`: the reference's order, `nn(pseudo)` as [E, in * out] (E in out 4 bytes; the last Linear costs 2 E K in out
    FLOP).  `reassociated`: the last Linear after the aggregation (E K 4 bytes of hidden activations plus one node block of
    Z' = [in][K + 1 padded to 4] floats per node; 2 E in K + 2 N in K out FLOP).  A route fits when
    twice its bytes are free (the gradient is as large again; the re-associated backward's workspace also holds the permuted last
    Linear and its gradient and the per-edge dx rows, which `bytes_reassociated` does not count - the call shrinks its node block
    to the free memory instead, `_hidden_any_ws_bytes`).  Eligible for re-association: `chain` (a Linear / ReLU chain),
    aggr add / mean, 1 <= k_hidden <= ANY_MAX_HIDDEN.
        off    materialised, or refused when it does not fit           (the behaviour before the re-associated kernels)
        auto   materialised whenever it fits - exactly the calls of `off`; only a call that `off` refuses takes the re-associated
               route, if it is eligible and fits; else refused
        on     every eligible call is re-associated (refused when it does not fit); the others as `off`
        streamed   every eligible call whose chain `dims` the library generates (chain_any_supported; `dims` None: the caller checks its
               chain itself and asks again with mode="off" for one that is not, as NNConv_old does) runs from the edge attributes,
               hidden rows by node block (gpde_nnconv_*_chain_any: neither per-edge tensor is formed; `bytes_streamed` is what the
               route holds besides one block of its budget); the others as `off`
    `acts` (ops.mlp_chain; None or all ReLU: everything above): a chain with another hidden activation (gpde_nnconv_*_chain_act) is
    eligible for the STREAMED route only - `eligible` stays False, `eligible_streamed` says it:
        streamed   streamed, as above
        auto       materialised whenever that fits, as today; a call that today is refused runs streamed (refused when twice
                   `bytes_streamed` is not free either)
        on, off    unchanged: materialised, or refused when it does not fit
    and `bytes_streamed` also counts the pre-activation rows U_l that the backward keeps for GELU, GELU_TANH, SILU and SIN, for a
    block of the preferred budget (they are spent from the block budget: such a chain has fewer edges per block)."""
    mode = ANY_REASSOC if mode is None else mode
    if mode not in ("auto", "on", "off", "streamed"):
        raise ValueError(f"GPDE_ANY_REASSOC must be auto, on or off, got {mode!r}")
    n, e, cin, cout = int(n_nodes), int(n_edges), int(in_channels), int(out_channels)
    k = None if k_hidden is None else int(k_hidden)
    streamable = bool(chain) and aggr in ("add", "mean") and k is not None and 1 <= k <= ANY_MAX_HIDDEN
    eligible = streamable and acts_all_relu(acts)
    if streamable and not eligible:
        return _act_chain_route(n, e, cin, cout, k, free_bytes, mode, dims, acts)
    bytes_m = e * cin * cout * 4
    out = {"eligible": eligible, "bytes_materialised": bytes_m, "bytes_reassociated": None, "node_block": None,
           "flops_materialised": None if k is None else 2 * e * k * cin * cout, "flops_reassociated": None, "bytes_streamed": None}
    fits_m = 2 * bytes_m <= free_bytes
    fits_r = False
    if eligible:
        zrow = cin * ((k + 1 + 3) // 4 * 4) * 4
        block = max(1, min(n, _ANY_PREF_Z_BYTES // zrow))
        out["node_block"] = block
        out["bytes_reassociated"] = e * k * 4 + block * zrow
        out["flops_reassociated"] = 2 * e * cin * k + 2 * n * cin * k * cout
        fits_r = 2 * out["bytes_reassociated"] <= free_bytes
    if eligible and (dims is None or chain_any_supported(dims)):          # (`dims` not given: the caller checks its chain)
        # what the streamed route holds whatever its block budget: the per-edge dx rows, the last Linear permuted and its gradient
        out["bytes_streamed"] = e * cin * 4 + 2 * zrow * ((cout + 3) // 4 * 4)
        if mode == "streamed":
            out["route"] = "streamed"
            return out
    if mode == "on" and eligible:
        out["route"] = "reassociated" if fits_r else "refused"
    elif fits_m:
        out["route"] = "materialised"
    elif mode == "auto" and fits_r:
        out["route"] = "reassociated"
    else:
        out["route"] = "refused"
    return out


# ... on one node set or between two (include/gpde.h gpde_nnconv_*_edgeweights_{any,bip} / gpde_nnconv_*_hidden_{any,bip}).  The library
# runs each pair in ONE body - a call on one node set is the two-set call that hands one table twice - and so does this file: four
# bodies take (x_src, x_dst, csr, ...), x_src [n_src, in_src] gathered by the edges, x_dst [n_dst, in_dst] in the root term, out
# [n_dst, out].  `x_dst` None: no destination features, so no root term.  `x_dst` _ONE_SET: one node set - the `_any` entry point and
# its argument list, x_src also the table of the root term (NOT the same tensor passed twice: the library adds the root term inside
# the ordered sum of grad_x, two partial gradients added by the caller would have other bits).
_ONE_SET = object()


def _dense(t):
    """Operand of the any-width entry points: dense, nothing more (not `_dense16` / `_operand`) - a dense tensor that starts off a
    16-byte boundary reaches the library as it is and takes the dword route there."""
    return t if t is None or t is _ONE_SET else t.detach().contiguous()


def _last_linear_args(w_last, b_last, cin: int, k: int, dev) -> int:
    """The last Linear of a re-associated call checked (w_last [in_src * out, K], b_last [in_src * out] or None); out_channels."""
    if w_last.dtype != torch.float32 or w_last.dim() != 2 or w_last.size(1) != k or w_last.size(0) % cin != 0 or w_last.size(0) == 0 or \
            w_last.device != dev:
        raise ValueError(f"w_last must be float32 [{cin} * out_channels, {k}] on {dev}, got {w_last.dtype} {tuple(w_last.shape)}")
    cout = int(w_last.size(0)) // cin
    if b_last is not None and (b_last.dtype != torch.float32 or tuple(b_last.shape) != (cin * cout,) or b_last.device != dev):
        raise ValueError(f"b_last must be float32 [{cin * cout}] on {dev}, got {b_last.dtype} {tuple(b_last.shape)}")
    return cout


def _any_args(x_src, x_dst, csr: Csr, root, per_edge, last=None, out_channels: Optional[int] = None):
    """The node tables, the per-edge operand - W_e [E, in_src * out], or H [E, K] with `last` = (w_last, b_last) - and root of a call
    checked; (in_src, in_dst, out_channels, K or None).  The messages are those of the entry point that will run: it names its table
    `x` on one node set, `x_src` / `x_dst` between two, and states every fault of the per-edge operand or of root in one message
    on one node set, their column count in a message of its own between two.  `out_channels`: what the caller expects W_e to hold."""
    one = x_dst is _ONE_SET
    n_dst, e, pe_name = csr.n_nodes, csr.n_edges, "edge_weights" if last is None else "hidden"
    n_src = n_dst if one else csr.n_src
    if x_src.dtype != torch.float32 or x_src.dim() != 2 or x_src.size(0) != n_src or x_src.size(1) < 1:
        raise ValueError(f"{'x' if one else 'x_src'} must be float32 [{n_src}, {'in_channels' if one else 'in_src'}], got {x_src.dtype} "
                         f"{tuple(x_src.shape)}")
    dev, cin = x_src.device, int(x_src.size(1))
    if not one and x_dst is not None and (x_dst.dtype != torch.float32 or x_dst.dim() != 2 or x_dst.size(0) != n_dst or x_dst.size(1) < 1 or
                                          x_dst.device != dev):
        raise ValueError(f"x_dst must be float32 [{n_dst}, in_dst] on {dev}, got {x_dst.dtype} {tuple(x_dst.shape)}")
    cind = cin if one or x_dst is None else int(x_dst.size(1))
    bad = per_edge.dtype != torch.float32 or per_edge.dim() != 2 or per_edge.size(0) != e or per_edge.size(1) < 1 or per_edge.device != dev
    ragged = last is None and not bad and per_edge.size(1) % cin != 0
    if bad or (one and ragged):
        cols = "." if not one else f"{cin} * out_channels" if last is None else "k_hidden"
        raise ValueError(f"{pe_name} must be float32 [{e}, {cols}] on {dev}, got {per_edge.dtype} {tuple(per_edge.shape)}")
    if ragged:
        raise ValueError(f"edge_weights must be [{e}, {cin} * out_channels], got {tuple(per_edge.shape)}")
    if last is None:
        cout, k = int(per_edge.size(1)) // cin, None
        if out_channels is not None and int(out_channels) != cout:
            raise ValueError(f"edge_weights has {per_edge.size(1)} columns = {cin} x {cout}, not {cin} x {out_channels}")
    else:
        k = int(per_edge.size(1))
        cout = _last_linear_args(last[0], last[1], cin, k, dev)
    if root is not None and x_dst is None:
        raise ValueError("root without x_dst: the root term is x_dst . root (pass root=None for a call without destination features)")
    if root is not None:
        bad = root.dtype != torch.float32 or root.dim() != 2 or root.size(0) != cind or root.device != dev
        if bad or (one and root.size(1) != cout):
            raise ValueError(f"root must be float32 {f'[{cin},{cout}]' if one else f'[{cind}, out_channels]'} on {dev}, got {root.dtype} "
                             f"{tuple(root.shape)}")
        if root.size(1) != cout:
            raise ValueError(f"root must be [{cind},{cout}], got {tuple(root.shape)}")
    if not (width_supported(cin, cout) and width_supported(cind, cout)):
        raise NotImplementedError(f"{f'in_channels {cin}' if one else f'(in_src {cin}, in_dst {cind})'} -> out_channels {cout}: the native "
                                  f"operator is built for widths 1 .. {ANY_MAX_WIDTH}")
    if k is not None and k > ANY_MAX_HIDDEN:
        raise NotImplementedError(f"last hidden width {k}: the re-associated any-width operator is built for 1 .. {ANY_MAX_HIDDEN}")
    return cin, cind, cout, k


def _any_f32(t, name: str, shape, dev):
    """`t` (bias [out], residual [n_dst, out]; or None) checked and dense."""
    if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != dev):
        raise ValueError(f"{name} must be float32 [{','.join(str(s) for s in shape)}] on {dev}, got {t.dtype} {tuple(t.shape)}")
    return _dense(t)


def _any_grad_out(grad_out, n_dst: int, cout: int):
    grad_out = grad_out.detach().contiguous().float()
    if tuple(grad_out.shape) != (n_dst, cout):
        raise ValueError(f"grad_out must be [{n_dst},{cout}], got {tuple(grad_out.shape)}")
    return grad_out


def _any_native(stem: str, xs, xd, csr: Csr, widths, before, after):
    """One native call: gpde_nnconv_<stem>_any(x, n, *before, in, out, *after, stream) when `xd` is _ONE_SET, else
    gpde_nnconv_<stem>_bip(x_src, n_src, x_dst, n_dst, *before, in_src, in_dst, out, *after, stream)."""
    one, dev = xd is _ONE_SET, xs.device
    name = f"gpde_nnconv_{stem}_{'any' if one else 'bip'}"
    tables = (xs.data_ptr(), csr.n_nodes) if one else (xs.data_ptr(), csr.n_src, _ptr(xd), csr.n_nodes)
    _call(name, dev, *tables, *before, *((widths[0], widths[2]) if one else widths), *after)


def _x_name(x_dst) -> str:
    return "x" if x_dst is _ONE_SET else "x_src"


def _any_fwd_edgeweights(x_src, x_dst, csr: Csr, edge_weights, root, bias, aggr: str, residual, relu: bool, out_channels=None):
    _require_cuda(x_src, _x_name(x_dst))
    if aggr not in _AGGR_WE:
        raise NotImplementedError(f"aggr={aggr!r}")
    xs, xd, we, root_c = _dense(x_src), _dense(x_dst), _dense(edge_weights), _dense(root)
    widths = _any_args(xs, xd, csr, root_c, we, out_channels=out_channels)[:3]
    n_dst, cout, dev = csr.n_nodes, widths[2], xs.device
    bias_c = _any_f32(bias, "bias", (cout,), dev)
    if residual is not None:
        _require_cuda(residual, "residual")
    res = _any_f32(residual, "residual", (n_dst, cout), dev)
    out = torch.empty(n_dst, cout, dtype=torch.float32, device=dev)
    _any_native("fwd_edgeweights", xs, xd, csr, widths,
                (we.data_ptr(), csr.n_edges, csr.rowptr.data_ptr(), csr.src.data_ptr(), _ptr(root_c), _ptr(bias_c), _ptr(res), 1 if relu else 0,
                 _AGGR_WE[aggr]), (out.data_ptr(),))
    return out


def _any_bwd_edgeweights(x_src, x_dst, csr: Csr, edge_weights, root, aggr: str, grad_out, need_x_src, need_x_dst, need_root, need_bias):
    """Returns (grad_x_src, grad_x_dst, grad_edge_weights, grad_root, grad_bias).  One node set: grad_x_dst is None and the entry
    point takes no NULL grad_x - `need_x_src` must be True."""
    lib = _lib.lib()
    for t, nm in ((x_src, _x_name(x_dst)), (edge_weights, "edge_weights"), (grad_out, "grad_out")):
        _require_cuda(t, nm)
    if aggr not in _AGGR:
        raise NotImplementedError(f"aggr={aggr!r}: the gradient of the per-edge weight operator is built for 'add' and 'mean'")
    one = x_dst is _ONE_SET
    xs, xd, we, root_c = _dense(x_src), _dense(x_dst), _dense(edge_weights), _dense(root)
    cin, cind, cout, _ = _any_args(xs, xd, csr, root_c, we)
    n_src, n_dst, e, dev = int(xs.size(0)), csr.n_nodes, csr.n_edges, xs.device
    grad_out = _any_grad_out(grad_out, n_dst, cout)
    new = lambda want, *shape: torch.empty(*shape, dtype=torch.float32, device=dev) if want else None
    gxs, gxd = new(need_x_src, n_src, cin), new(need_x_dst and not one and xd is not None, n_dst, cind)
    gwe = new(True, e, cin * cout)
    groot, gbias = new(need_root and root is not None, cind, cout), new(need_bias, cout)
    if one:
        ws = _alloc_ws(int(lib.gpde_nnconv_bwd_edgeweights_any_workspace_bytes(n_dst, e, cin, cout)), dev)
    else:
        ws = _alloc_ws(int(lib.gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(n_src, n_dst, e, cin, cind, cout)), dev)
    # one node set: grad_x is always written, so the source order is always taken (on a graph without edges too)
    srp, ssl = csr.src_order if (one or (need_x_src and e > 0)) else (None, None)
    _any_native("bwd_edgeweights", xs, xd, csr, (cin, cind, cout),
                (we.data_ptr(), e, csr.rowptr.data_ptr(), csr.src.data_ptr(), _ptr(srp), _ptr(ssl), _ptr(root_c), _AGGR[aggr]),
                (grad_out.data_ptr(), *((gxs.data_ptr(),) if one else (_ptr(gxs), _ptr(gxd))), gwe.data_ptr(), _ptr(groot), _ptr(gbias),
                 ws.data_ptr(), ws.numel()))
    return gxs, gxd, gwe, groot, gbias


def _any_hidden_operands(x_src, x_dst, csr: Csr, hidden, w_last, b_last, root, aggr: str, grad_out=None):
    """What the forward and the backward given H share: device and aggr checks, dense operands, the shape gate."""
    for t, nm in ((x_src, _x_name(x_dst)), (hidden, "hidden"), (w_last, "w_last")) + (() if grad_out is None else ((grad_out, "grad_out"),)):
        _require_cuda(t, nm)
    if aggr not in _AGGR:
        raise NotImplementedError(f"aggr={aggr!r}: the re-associated operator is built for 'add' and 'mean'")
    xs, xd, hid, wl, bl, root_c = (_dense(t) for t in (x_src, x_dst, hidden, w_last, b_last, root))
    return xs, xd, hid, wl, bl, root_c, _any_args(xs, xd, csr, root_c, hid, last=(wl, bl))


def _any_fwd_hidden(x_src, x_dst, csr: Csr, hidden, w_last, b_last, root, bias, aggr: str, ws_bytes):
    lib = _lib.lib()
    xs, xd, hid, wl, bl, root_c, (cin, cind, cout, k) = _any_hidden_operands(x_src, x_dst, csr, hidden, w_last, b_last, root, aggr)
    n_dst, e, dev = csr.n_nodes, csr.n_edges, xs.device
    bias_c = _any_f32(bias, "bias", (cout,), dev)
    query = lib.gpde_nnconv_fwd_hidden_any_workspace_bytes if xd is _ONE_SET else lib.gpde_nnconv_fwd_hidden_bip_workspace_bytes
    ws = _alloc_ws(_hidden_any_ws_bytes(query, n_dst, e, cin, cout, k, dev) if ws_bytes is None else int(ws_bytes), dev)
    out = torch.empty(n_dst, cout, dtype=torch.float32, device=dev)
    _any_native("fwd_hidden", xs, xd, csr, (cin, cind, cout),
                (hid.data_ptr(), e, k, csr.rowptr.data_ptr(), csr.src.data_ptr(), wl.data_ptr(), _ptr(bl), _ptr(root_c), _ptr(bias_c), _AGGR[aggr]),
                (out.data_ptr(), ws.data_ptr(), ws.numel()))
    return out


def _any_bwd_hidden(x_src, x_dst, csr: Csr, hidden, w_last, b_last, root, aggr: str, grad_out, need_x_src, need_x_dst, need_w_last,
                    need_b_last, need_root, need_bias, ws_bytes):
    """Returns (grad_x_src, grad_x_dst, grad_hidden, grad_w_last, grad_b_last, grad_root, grad_bias); grad_x_dst is None on one node set."""
    lib = _lib.lib()
    xs, xd, hid, wl, bl, root_c, (cin, cind, cout, k) = _any_hidden_operands(x_src, x_dst, csr, hidden, w_last, b_last, root, aggr, grad_out)
    one = xd is _ONE_SET
    n_src, n_dst, e, dev = int(xs.size(0)), csr.n_nodes, csr.n_edges, xs.device
    grad_out = _any_grad_out(grad_out, n_dst, cout)
    new = lambda want, *shape: torch.empty(*shape, dtype=torch.float32, device=dev) if want else None
    gxs, gxd, gh = new(need_x_src, n_src, cin), new(need_x_dst and not one and xd is not None, n_dst, cind), new(True, e, k)
    gwl, gbl = new(need_w_last, cin * cout, k), new(need_b_last and b_last is not None, cin * cout)
    groot, gbias = new(need_root and root is not None, cind, cout), new(need_bias, cout)
    if one:
        query = lib.gpde_nnconv_bwd_hidden_any_workspace_bytes
    else:       # (the two-set backward's query takes in_dst as well)
        query = lambda n, ee, ci, co, kk: lib.gpde_nnconv_bwd_hidden_bip_workspace_bytes(n, ee, ci, cind, co, kk)
    ws = _alloc_ws(_hidden_any_ws_bytes(query, n_dst, e, cin, cout, k, dev) if ws_bytes is None else int(ws_bytes), dev)
    srp, ssl = csr.src_order if (need_x_src and e > 0) else (None, None)
    _any_native("bwd_hidden", xs, xd, csr, (cin, cind, cout),
                (hid.data_ptr(), e, k, csr.rowptr.data_ptr(), csr.src.data_ptr(), wl.data_ptr(), _ptr(bl), _ptr(root_c), _AGGR[aggr]),
                (grad_out.data_ptr(), *((_ptr(gxs),) if one else (_ptr(gxs), _ptr(gxd))), gh.data_ptr(), _ptr(gwl), _ptr(gbl), _ptr(groot),
                 _ptr(gbias), _ptr(srp), _ptr(ssl), ws.data_ptr(), ws.numel()))
    return gxs, gxd, gh, gwl, gbl, groot, gbias


# the eight entry points by name (tests and callers spy on, trace and patch these): each a delegation to its body
def nnconv_forward_edgeweights_any_raw(x, csr: Csr, edge_weights, root, bias, aggr: str, residual=None, relu: bool = False,
                                       out_channels: Optional[int] = None) -> torch.Tensor:
    """gpde_nnconv_fwd_edgeweights_any: the operator given the per-edge weights [E, in * out] (CSR slot order) at any width
    1 .. 256 - gather, message, add / mean / max, update() (+ residual [N, out], ReLU) in one launch."""
    return _any_fwd_edgeweights(x, _ONE_SET, csr, edge_weights, root, bias, aggr, residual, relu, out_channels)


def nnconv_backward_edgeweights_any_raw(x: torch.Tensor, csr: Csr, edge_weights: torch.Tensor, root: Optional[torch.Tensor], aggr: str,
                                        grad_out: torch.Tensor, need_root: bool = True, need_bias: bool = True):
    """gpde_nnconv_bwd_edgeweights_any: backward of the any-width operator given the per-edge weights ('add' / 'mean').  Returns
    (grad_x [N, in], grad_edge_weights [E, in * out], grad_root [in, out] or None, grad_bias [out] or None)."""
    gx, _, gwe, groot, gbias = _any_bwd_edgeweights(x, _ONE_SET, csr, edge_weights, root, aggr, grad_out, True, False, need_root, need_bias)
    return gx, gwe, groot, gbias


def nnconv_forward_hidden_any_raw(x, csr: Csr, hidden, w_last, b_last, root, bias, aggr: str, ws_bytes: Optional[int] = None) -> torch.Tensor:
    """gpde_nnconv_fwd_hidden_any: the any-width operator given the last hidden activations [E, K] (CSR slot order) and the last
    Linear (w_last [in * out, K], b_last [in * out] or None) - aggregation, last Linear per node, update().  'add' / 'mean'.
    `ws_bytes`: the workspace to run in (default: the library's preferred size); less gives more node blocks."""
    return _any_fwd_hidden(x, _ONE_SET, csr, hidden, w_last, b_last, root, bias, aggr, ws_bytes)


def nnconv_backward_hidden_any_raw(x, csr: Csr, hidden, w_last, b_last, root, aggr: str, grad_out, need_x: bool = True,
                                   need_w_last: bool = True, need_b_last: bool = True, need_root: bool = True, need_bias: bool = True,
                                   ws_bytes: Optional[int] = None):
    """gpde_nnconv_bwd_hidden_any: backward of the re-associated any-width operator.  Returns (grad_x [N, in], grad_hidden [E, K] -
    dL/d hidden, the caller's ReLU not applied -, grad_w_last [in * out, K], grad_b_last [in * out], grad_root [in, out], grad_bias
    [out]); an output that is not needed (or has no input: b_last / root None) is None."""
    g = _any_bwd_hidden(x, _ONE_SET, csr, hidden, w_last, b_last, root, aggr, grad_out, need_x, False, need_w_last, need_b_last, need_root,
                        need_bias, ws_bytes)
    return (g[0], *g[2:])


def nnconv_forward_edgeweights_bip_raw(x_src, x_dst, csr: Csr, edge_weights, root, bias, aggr: str, residual=None, relu: bool = False) -> torch.Tensor:
    """gpde_nnconv_fwd_edgeweights_bip: the operator between two node sets given the per-edge weights [E, in_src * out] (CSR slot
    order) - gather from x_src, message, add / mean / max over the n_dst destinations, + x_dst . root + bias (+ residual
    [n_dst, out], ReLU) in one launch.  `x_dst` None: no root term (root must be None)."""
    return _any_fwd_edgeweights(x_src, x_dst, csr, edge_weights, root, bias, aggr, residual, relu)


def nnconv_backward_edgeweights_bip_raw(x_src, x_dst, csr: Csr, edge_weights, root, aggr: str, grad_out, need_x_src: bool = True,
                                        need_x_dst: bool = True, need_root: bool = True, need_bias: bool = True):
    """gpde_nnconv_bwd_edgeweights_bip ('add' / 'mean').  Returns (grad_x_src [n_src, in_src], grad_x_dst [n_dst, in_dst],
    grad_edge_weights [E, in_src * out], grad_root [in_dst, out], grad_bias [out]); an output that is not needed or has no input
    (x_dst / root None) is None."""
    return _any_bwd_edgeweights(x_src, x_dst, csr, edge_weights, root, aggr, grad_out, need_x_src, need_x_dst, need_root, need_bias)


def nnconv_forward_hidden_bip_raw(x_src, x_dst, csr: Csr, hidden, w_last, b_last, root, bias, aggr: str, ws_bytes: Optional[int] = None) -> torch.Tensor:
    """gpde_nnconv_fwd_hidden_bip: the re-associated operator between two node sets given the last hidden activations [E, K] (CSR
    slot order) and the last Linear (w_last [in_src * out, K], b_last) - Z' per destination, last Linear per destination,
    + x_dst . root + bias.  'add' / 'mean'."""
    return _any_fwd_hidden(x_src, x_dst, csr, hidden, w_last, b_last, root, bias, aggr, ws_bytes)


def nnconv_backward_hidden_bip_raw(x_src, x_dst, csr: Csr, hidden, w_last, b_last, root, aggr: str, grad_out, need_x_src: bool = True,
                                   need_x_dst: bool = True, need_w_last: bool = True, need_b_last: bool = True, need_root: bool = True,
                                   need_bias: bool = True, ws_bytes: Optional[int] = None):
    """gpde_nnconv_bwd_hidden_bip.  Returns (grad_x_src, grad_x_dst, grad_hidden [E, K], grad_w_last, grad_b_last, grad_root
    [in_dst, out], grad_bias); an output that is not needed or has no input is None."""
    return _any_bwd_hidden(x_src, x_dst, csr, hidden, w_last, b_last, root, aggr, grad_out, need_x_src, need_x_dst, need_w_last, need_b_last,
                           need_root, need_bias, ws_bytes)


def edge_weights_backward_raw(grad_we: torch.Tensor, hidden: torch.Tensor, dims: Sequence[int], w_last: torch.Tensor,
                              need_b: bool = True):
    """gpde_edge_weights_bwd: (grad_hidden [E, K2P] already masked by hidden > 0, grad_w_last, grad_b_last or None) from the
    summed gradient of the per-edge weights."""
    lib = _lib.lib()
    _require_cuda(grad_we, "grad_edge_weights")
    e, dev = int(hidden.size(0)), hidden.device
    nl = len(dims) - 1
    dims_c = _lib.dims_array(dims)
    grad_we = _operand(grad_we.detach(), "grad_edge_weights", (e, WIDTH * WIDTH), dev)
    hidden = _operand(hidden.detach(), "hidden", (e, hidden_width(dims)), dev)
    w_c = _operand(w_last.detach(), "w_last", (WIDTH * WIDTH, dims[-2]), dev)
    gh = torch.empty_like(hidden)
    gw = torch.empty_like(w_c)
    gb = torch.empty(WIDTH * WIDTH, dtype=torch.float32, device=dev) if need_b else None
    ws = _alloc_ws(int(lib.gpde_edge_weights_bwd_workspace_bytes(e, nl, dims_c)), dev)
    _call("gpde_edge_weights_bwd", dev, grad_we.data_ptr(), hidden.data_ptr(), e, nl, dims_c, w_c.data_ptr(), gh.data_ptr(), gw.data_ptr(), _ptr(gb),
          ws.data_ptr(), ws.numel())
    return gh, gw, gb


def nnconv_forward_mixed_raw(x: torch.Tensor, csr: Csr, edge_attr: torch.Tensor, hidden: torch.Tensor,
                             hmax: Optional[torch.Tensor], hidden_nodes: int, pm: PackedMlp,
                             root: Optional[torch.Tensor], bias: Optional[torch.Tensor], aggr: str,
                             precision: Optional[str] = None, z_keep: Optional[torch.Tensor] = None,
                             out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gpde_nnconv_fwd_mixed_keepz: nodes [0, hidden_nodes) aggregate from `hidden` (their in-edges' rows), the
    rest run the fused kernel -- for graphs whose full H does not fit memory.  `z_keep`: as nnconv_forward_raw.
    `edge_attr` may be a NodeAttr (the call's `node_attr`; `hidden` None / hidden_nodes 0: no partial H)."""
    n = csr.n_nodes
    if x.dtype != torch.float32 or x.dim() != 2 or x.size(1) != WIDTH or x.size(0) != n:
        raise ValueError(f"x must be float32 [{n},{WIDTH}]")
    flags = _PRECISION[DEFAULT_PRECISION if precision is None else precision]
    return _forward64("gpde_nnconv_fwd_mixed_keepz", x, csr, pm, root, bias, aggr, flags, attr=edge_attr.detach(), hidden=hidden,
                      hmax=hmax, hidden_nodes=hidden_nodes, z_keep=z_keep, out=out, ws=ws)


def nnconv_backward_hidden_raw(x: torch.Tensor, csr: Csr, hidden: torch.Tensor, dims: Sequence[int],
                               w_last: torch.Tensor, b_last: Optional[torch.Tensor],
                               root: Optional[torch.Tensor], aggr: str, grad_out: torch.Tensor,
                               need_root: bool = True, need_bias: bool = True, z_saved: Optional[torch.Tensor] = None,
                               grad_hidden_acc: Optional[torch.Tensor] = None):
    """gpde_nnconv_bwd in its `hidden` form (the last hidden activations given; `z_saved`: the keep-Z forward's buffer;
    `grad_hidden_acc`: a [E, K2P] tensor dL/dU is ADDED to instead of a fresh one - GPDE_BWD_ACCUMULATE_GRAD_HIDDEN).  Returns (grad_x, grad_hidden [E,K2P], grad_w_last, grad_b_last or None,
    grad_root or None, grad_bias or None)."""
    gx, gh, _, gW, gb, groot, gbias = _backward64("conv", csr, [w_last], [b_last], dims=dims, x=x, hidden=hidden, root=root, aggr=aggr,
                                                  grad_out=grad_out, z_saved=z_saved, grad_hidden_out=grad_hidden_acc,
                                                  need_root=need_root, need_bias=need_bias)
    return gx, gh, gW[-1], gb[-1], groot, gbias


def hidden_backward_raw(csr: Csr, edge_attr: torch.Tensor, dims: Sequence[int],
                        weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]],
                        grad_hidden: torch.Tensor):
    """gpde_hidden_bwd: gradients of the hidden Linear layers from the summed dL/dU of the last hidden
    layer.  `weights` / `biases`: the hidden layers only (all but the last Linear); `dims`: all layer
    widths.  Returns ([grad_W_l], [grad_b_l or None]) for the hidden layers."""
    if len(weights) != len(dims) - 2:
        raise ValueError("hidden_backward_raw takes the hidden layers only")
    _, _, _, gW, gb, _, _ = _backward64("mlp", csr, weights, biases, dims=dims, edge_attr=edge_attr, grad_hidden_in=grad_hidden)
    return gW[:-1], gb[:-1]



# ----------------------------------------------------------------------------------------------
# radius graph
# ----------------------------------------------------------------------------------------------
def radius_graph(pos: torch.Tensor, r: float, reference_ties: bool = False,
                 pos_dst: Optional[torch.Tensor] = None, period=None, origin=None) -> torch.Tensor:
    """edge_index int64 [2,E] of the radius graph of `pos` [n,dim] (dim 1..3), in the reference's
    order (sorted by source, then target; self-loops included) - the GPU replacement of
    `ball_connectivity` (utilities.py:250-255).  One sync (the edge count) per graph.

    `pos_dst`: a second point set - edges (j in pos -> i in pos_dst), the inter-level graphs of
    RandomMultiMeshGenerator (multipole-graph-neural-operator/utilities.py:617-632).
    `reference_ties=True`: scikit-learn's dot-product-expansion arithmetic, so that pairs at exactly distance r
    are kept / dropped exactly as by the reference (gpde_radius_graph2_*, GPDE_RADIUS_REFERENCE_TIES); the default
    tests the exact float64 sum of squares (symmetric graph).
    `period` / `origin`: the graph on a periodic box (see radius_csr_raw), in the same source-major order - the periodic
    CSR stably sorted by source (there is no periodic brute-force kernel)."""
    if period is not None:
        _, src, dst = radius_csr_raw(pos, r, reference_ties, pos_dst, period=period, origin=origin)
        order = torch.sort(src, stable=True).indices          # rows are destination-major: targets stay ascending per source
        return torch.stack([src[order].long(), dst[order].long()])
    lib = _lib.lib()
    _require_cuda(pos, "pos")
    if pos.dim() == 1:
        pos = pos.unsqueeze(1)
    pos = pos.detach().to(torch.float64).contiguous()
    if pos_dst is None:
        pd = pos
    else:
        _require_cuda(pos_dst, "pos_dst")
        pd = (pos_dst.unsqueeze(1) if pos_dst.dim() == 1 else pos_dst).detach().to(torch.float64).contiguous()
        if pd.size(1) != pos.size(1):
            raise ValueError("pos and pos_dst must have the same dimension")
    n, nd, dim = int(pos.size(0)), int(pd.size(0)), int(pos.size(1))
    flags = 1 if reference_ties else 0
    dev = pos.device
    deg = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_graph2_count(pos.data_ptr(), n, pd.data_ptr(), nd, dim, float(r), flags,
                                                deg.data_ptr(), _stream_ptr(dev)), "gpde_radius_graph2_count")
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=offs[1:])
    e = int(offs[-1].item())
    ei = torch.empty(2, e, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_graph2_fill(pos.data_ptr(), n, pd.data_ptr(), nd, dim, float(r), flags,
                                               offs.data_ptr(), ei.data_ptr(), e, _stream_ptr(dev)),
                   "gpde_radius_graph2_fill")
    return ei


def _positions(pos: torch.Tensor, pos_dst: Optional[torch.Tensor]):
    """(pos, pos_dst or pos) as contiguous float64 [n, dim] device tensors of one dimension."""
    _require_cuda(pos, "pos")
    pos = (pos.unsqueeze(1) if pos.dim() == 1 else pos).detach().to(torch.float64).contiguous()
    if pos_dst is None:
        return pos, pos
    _require_cuda(pos_dst, "pos_dst")
    pd = (pos_dst.unsqueeze(1) if pos_dst.dim() == 1 else pos_dst).detach().to(torch.float64).contiguous()
    if pd.size(1) != pos.size(1):
        raise ValueError("pos and pos_dst must have the same dimension")
    return pos, pd


def _host_bounds(pos: torch.Tensor, pd: torch.Tensor):
    """Host arrays lo / hi [dim]: a bounding box of both point sets (one small copy)."""
    dim = int(pos.size(1))
    both = pos if pd is pos else torch.cat([pos, pd])
    lo_t, hi_t = both.min(dim=0).values.cpu(), both.max(dim=0).values.cpu()
    return (ctypes.c_double * dim)(*[float(v) for v in lo_t]), (ctypes.c_double * dim)(*[float(v) for v in hi_t])


def periodic_box(period, origin, dim: int, r: float, reference_ties: bool = False):
    """`period` / `origin` of the radius-graph builders as two lists of `dim` floats (host only; raises ValueError).
    period: a scalar (every axis) or one entry per axis, 0 / None = an open axis; origin: likewise, default 0."""
    def per_axis(v, name):
        if v is None or isinstance(v, (int, float)):
            return [0.0 if v is None else float(v)] * dim
        v = [0.0 if t is None else float(t) for t in (v.tolist() if isinstance(v, torch.Tensor) else v)]
        if len(v) != dim:
            raise ValueError(f"{name} has {len(v)} entries for positions of dimension {dim}")
        return v
    if not 1 <= dim <= 3:
        raise ValueError(f"positions of dimension {dim}: the radius graphs are built in 1..3 dimensions")
    if reference_ties:
        raise ValueError("reference_ties=True has no periodic form: the reference's torus_connectivity / torus1d_connectivity shift an "
                         "ALIAS of the grid (grid1 = grid), so its graphs never wrap and there are no reference ties to reproduce")
    per, org = per_axis(period, "period"), per_axis(origin, "origin")
    if not float(r) > 0.0:
        raise ValueError(f"r = {r} must be positive")
    for k, L in enumerate(per):
        if L < 0.0 or L != L:
            raise ValueError(f"period[{k}] = {L} must be >= 0 (0 = open axis)")
        if L > 0.0 and not 2.0 * float(r) < L:
            raise ValueError(f"2 r = {2.0 * float(r)} >= period[{k}] = {L}: a pair would have more than one image within r")
    return per, org


def _radius_csr_periodic(pos, r, pos_dst, period, origin, reference_ties, fill: bool, geometry: bool):
    """gpde_radius_csr_periodic_count (+ _fill): (deg,) or (rowptr, src, dst, geom | None)."""
    dim_in = 1 if pos.dim() == 1 else int(pos.size(1))
    per, org = periodic_box(period, origin, dim_in, r, reference_ties)          # host checks first: no device is needed to be refused
    lib = _lib.lib()
    pos, pd = _positions(pos, pos_dst)
    n, nd, dim = int(pos.size(0)), int(pd.size(0)), int(pos.size(1))
    dev = pos.device
    if n == 0 or nd == 0:
        if not fill:
            return (torch.zeros(nd, dtype=torch.int32, device=dev),)
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return (torch.zeros(nd + 1, dtype=torch.int32, device=dev), z, z.clone(),
                torch.zeros(0, dim + 1, dtype=torch.float32, device=dev) if geometry else None)
    lo, hi = _host_bounds(pos, pd)
    org_c, per_c = (ctypes.c_double * dim)(*org), (ctypes.c_double * dim)(*per)
    nbytes = int(lib.gpde_radius_csr_periodic_workspace_bytes(n, dim, float(r), lo, hi, org_c, per_c))
    if nbytes == 0:
        _lib.check(-1, "gpde_radius_csr_periodic_workspace_bytes")
    ws = _alloc_ws(nbytes, dev)
    deg = torch.empty(nd, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_csr_periodic_count(pos.data_ptr(), n, pd.data_ptr(), nd, dim, float(r), 0, lo, hi, org_c, per_c,
                                                      deg.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev)),
                   "gpde_radius_csr_periodic_count")
    if not fill:
        return (deg,)
    rowptr64 = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=rowptr64[1:])
    e = int(rowptr64[-1].item())
    if e >= (1 << 31) - 64:
        raise NotImplementedError(f"{e} edges exceed the int32 CSR")
    rowptr = rowptr64.to(torch.int32)
    src = torch.empty(e, dtype=torch.int32, device=dev)
    dst = torch.empty(e, dtype=torch.int32, device=dev)
    geom = torch.empty(e, dim + 1, dtype=torch.float32, device=dev) if geometry else None
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_csr_periodic_fill(pos.data_ptr(), n, pd.data_ptr(), nd, dim, float(r), 0, lo, hi, org_c, per_c,
                                                     rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                                     None if geom is None else geom.data_ptr(), e, ws.data_ptr(), ws.numel(),
                                                     _stream_ptr(dev)), "gpde_radius_csr_periodic_fill")
    return rowptr, src, dst, geom


def radius_csr_raw(pos: torch.Tensor, r: float, reference_ties: bool = False, pos_dst: Optional[torch.Tensor] = None,
                   period=None, origin=None, return_geometry: bool = False):
    """Cell-list radius graph emitted directly as a destination CSR (gpde_radius_csr_count / _fill): returns
    (rowptr int32 [n_dst + 1], src int32 [E], dst int32 [E]) - edge (src[s] in pos -> dst[s] in pos_dst), rows in
    ascending source order.  One sync (the edge count) per graph.

    `period` (a scalar or one entry per axis; 0 / None = open axis) with `origin` (default 0): the graph on a periodic box by
    minimum-image distance (gpde_radius_csr_periodic_*; 2 r < period).  `return_geometry=True` adds a fourth result, `geom`
    float32 [E, dim + 1] by CSR slot: the minimum-image displacement pos[src] - image(pos_dst[dst]) and its norm (on open
    axes, and with period=None, the plain difference)."""
    if period is None and return_geometry and reference_ties:
        raise ValueError("return_geometry=True is built on the exact distance arithmetic: reference_ties must be False")
    if period is not None or return_geometry:
        rowptr, src, dst, geom = _radius_csr_periodic(pos, r, pos_dst, period, origin, reference_ties, True, return_geometry)
        return (rowptr, src, dst, geom) if return_geometry else (rowptr, src, dst)
    lib = _lib.lib()
    _require_cuda(pos, "pos")
    pos = (pos.unsqueeze(1) if pos.dim() == 1 else pos).detach().to(torch.float64).contiguous()
    if pos_dst is None:
        pd = pos
    else:
        _require_cuda(pos_dst, "pos_dst")
        pd = (pos_dst.unsqueeze(1) if pos_dst.dim() == 1 else pos_dst).detach().to(torch.float64).contiguous()
        if pd.size(1) != pos.size(1):
            raise ValueError("pos and pos_dst must have the same dimension")
    n, nd, dim = int(pos.size(0)), int(pd.size(0)), int(pos.size(1))
    dev = pos.device
    if n == 0 or nd == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return torch.zeros(nd + 1, dtype=torch.int32, device=dev), z, z.clone()
    both = pos if pd is pos else torch.cat([pos, pd])
    lo_t, hi_t = both.min(dim=0).values.cpu(), both.max(dim=0).values.cpu()       # host bounds (one small copy)
    lo = (ctypes.c_double * dim)(*[float(v) for v in lo_t])
    hi = (ctypes.c_double * dim)(*[float(v) for v in hi_t])
    flags = 1 if reference_ties else 0
    nbytes = int(lib.gpde_radius_csr_workspace_bytes(n, dim, float(r), lo, hi))
    if nbytes == 0:
        _lib.check(-1, "gpde_radius_csr_workspace_bytes")
    ws = _alloc_ws(nbytes, dev)
    deg = torch.empty(nd, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_csr_count(pos.data_ptr(), n, pd.data_ptr(), nd, dim, float(r), flags, lo, hi, deg.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "gpde_radius_csr_count")
    rowptr64 = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=rowptr64[1:])
    e = int(rowptr64[-1].item())
    if e >= (1 << 31) - 64:
        raise NotImplementedError(f"{e} edges exceed the int32 CSR")
    rowptr = rowptr64.to(torch.int32)
    src = torch.empty(e, dtype=torch.int32, device=dev)
    dst = torch.empty(e, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_csr_fill(pos.data_ptr(), n, pd.data_ptr(), nd, dim, float(r), flags, lo, hi, rowptr.data_ptr(),
                                            src.data_ptr(), dst.data_ptr(), e, ws.data_ptr(), ws.numel(), _stream_ptr(dev)),
                   "gpde_radius_csr_fill")
    return rowptr, src, dst


def radius_in_degrees(pos: torch.Tensor, r: float, reference_ties: bool = False, pos_dst: Optional[torch.Tensor] = None,
                      period=None, origin=None) -> torch.Tensor:
    """int32 [n_dst]: in-degree of every destination of the radius graph - the COUNT pass of the cell-list builder alone
    (gpde_radius_csr_count; no edge is written).  parallel.partition_rows_by_position balances its row blocks on it.
    `period` / `origin`: on a periodic box (see radius_csr_raw)."""
    if period is not None:
        return _radius_csr_periodic(pos, r, pos_dst, period, origin, reference_ties, False, False)[0]
    lib = _lib.lib()
    _require_cuda(pos, "pos")
    pos = (pos.unsqueeze(1) if pos.dim() == 1 else pos).detach().to(torch.float64).contiguous()
    pd = pos if pos_dst is None else (pos_dst.unsqueeze(1) if pos_dst.dim() == 1 else pos_dst).detach().to(torch.float64).contiguous()
    n, nd, dim = int(pos.size(0)), int(pd.size(0)), int(pos.size(1))
    dev = pos.device
    deg = torch.zeros(nd, dtype=torch.int32, device=dev)
    if n == 0 or nd == 0:
        return deg
    both = pos if pd is pos else torch.cat([pos, pd])
    lo_t, hi_t = both.min(dim=0).values.cpu(), both.max(dim=0).values.cpu()
    lo = (ctypes.c_double * dim)(*[float(v) for v in lo_t])
    hi = (ctypes.c_double * dim)(*[float(v) for v in hi_t])
    nbytes = int(lib.gpde_radius_csr_workspace_bytes(n, dim, float(r), lo, hi))
    if nbytes == 0:
        _lib.check(-1, "gpde_radius_csr_workspace_bytes")
    ws = _alloc_ws(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_csr_count(pos.data_ptr(), n, pd.data_ptr(), nd, dim, float(r), 1 if reference_ties else 0, lo, hi,
                                             deg.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "gpde_radius_csr_count")
    return deg


def radius_csr(pos: torch.Tensor, r: float, reference_ties: bool = False, pos_dst: Optional[torch.Tensor] = None,
               period=None, origin=None, return_geometry: bool = False, max_num_neighbors: Optional[int] = None,
               select: str = "nearest", seed: int = 0):
    """The radius graph of one point set as the `Csr` the operator consumes (no edge_index, no sort): rowptr / src / dst
    are what `csr_for(radius_graph(pos, r), n)` builds - bit for bit - and `perm` is the identity: per-edge tensors for
    this graph are laid out by CSR slot (`csr.edge_index` is the edge list in that order), or not needed at all
    (`NodeAttr`).  Replaces ball_connectivity + the per-call index handling of PyG (utilities.py:250-255, nn_conv.py:271).

    `period` / `origin`: the graph on a periodic box (torus; see radius_csr_raw) - what TorusGridSplitter.torus_connectivity and
    torus1d_connectivity (multipole utilities.py:1190-1266, 404-417) are meant to build.  `return_geometry=True` returns
    (Csr, geom): geom float32 [E, dim + 1] = the minimum-image displacement pos[src] - image(pos[dst]) and its norm, already in
    the slot order the operator reads (perm is the identity) - the first columns of the reference's torus edge attributes
    [dx, dy, |d|, a_i, a_j] (utilities.py:1251-1257), which endpoint coordinates (`NodeAttr`) cannot give across the seam.

    `max_num_neighbors=k`: cap the in-degree (PyG's argument of that name; the reference's thinned `gaussian_connectivity`) - a
    destination with more than k sources within r keeps k of them, chosen by `select` (see select_in_edges for the contract):
    "nearest" - the k nearest (exact float64 squared distance, minimum-image on a periodic box; ties by source order), or
    "random" - a uniform k-subset drawn by a hash of (`seed`, destination id, source id): under aggr='mean' the unbiased
    Monte-Carlo estimate of the full-ball mean, which the k nearest are not.  Rows stay in ascending source order, `perm` is the
    identity and `geom` is gathered to the new slots.  The default (None) is the uncapped build, by the same calls as before.
    The cap is defined on the exact arithmetic: with reference_ties=True it raises ValueError.  radius_graph*, radius_csr_raw,
    radius_in_degrees, multilevel_radius_graphs and the rank partitioner (parallel.py) have no capped form."""
    k = _cap_args(max_num_neighbors, select, seed, reference_ties)        # host checks first: no device is needed to be refused
    out = radius_csr_raw(pos, r, reference_ties, pos_dst, period=period, origin=origin, return_geometry=return_geometry)
    rowptr, src, dst = out[:3]
    e = int(src.numel())
    # two point sets: the RECTANGULAR Csr of edges (j in pos -> i in pos_dst) - what csr_for(radius_graph(pos, r, pos_dst=...),
    # n_dst, n_src=n_src) builds, bit for bit; consumed by the module as conv((x_src, x_dst), csr, edge_attr)
    csr = Csr(int(rowptr.numel()) - 1, e, rowptr, src, dst, torch.arange(e, dtype=torch.int32, device=src.device),
              n_src_nodes=None if pos_dst is None else int(pos.size(0)))
    if k is None:
        return (csr, out[3]) if return_geometry else csr
    key = edge_sqdist_keys(csr, pos, pos_dst, period=period, origin=origin) if select == "nearest" else edge_hash_keys(csr.src, csr.dst, seed)
    csr, edge_ids = select_in_edges(csr, k, key)
    return (csr, out[3][edge_ids]) if return_geometry else csr


def multilevel_radius_graphs(pos_levels: Sequence[torch.Tensor], radii_inner: Sequence[float],
                             radii_inter: Sequence[float], reference_ties: Optional[bool] = None, period=None, origin=None):
    """The inner / down / up graphs of RandomMultiMeshGenerator.ball_connectivity
    (multipole-graph-neural-operator/utilities.py:602-640) built on the GPU from the per-level point sets:
    inner[l] = radius graph of level l (local node ids), down[l] = edges (level l -> level l + 1) within
    radii_inter[l], up[l] = down[l] with the rows swapped (utilities.py:631: the SAME edge order).  Returns
    {"inner": [...], "down": [...], "up": [...]} of int64 [2, E] tensors with level-local node ids.
    `reference_ties` defaults to the reference's arithmetic on an open box; with `period` (every level on the same periodic
    box, see radius_csr_raw) it defaults to the exact arithmetic, the only one a periodic graph has."""
    if reference_ties is None:
        reference_ties = period is None
    inner = [radius_graph(p, r, reference_ties=reference_ties, period=period, origin=origin) for p, r in zip(pos_levels, radii_inner)]
    down = [radius_graph(pos_levels[l], radii_inter[l], reference_ties=reference_ties, pos_dst=pos_levels[l + 1], period=period,
                         origin=origin) for l in range(len(pos_levels) - 1)]
    up = [d.flip(0) for d in down]
    return {"inner": inner, "down": down, "up": up}


# ----------------------------------------------------------------------------------------------
# capped in-degree: keep the k nearest or k sampled in-edges of every destination (gpde_select.hip)
# ----------------------------------------------------------------------------------------------
SELECT_MODES = ("nearest", "random")


def _cap_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"max_num_neighbors / k must be an int >= 1 (got {k!r})")
    if k < 1:
        raise ValueError(f"max_num_neighbors / k = {k} must be >= 1")
    return int(k)


def _cap_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, int) or not -(1 << 63) <= seed < (1 << 63):
        raise ValueError(f"seed must be an int in [-2^63, 2^63) (got {seed!r})")
    return int(seed)


def _cap_args(max_num_neighbors, select, seed, reference_ties: bool = False) -> Optional[int]:
    """The host checks of the builders' cap arguments (ValueError): k, or None for the uncapped build."""
    if select not in SELECT_MODES:
        raise ValueError(f"select = {select!r} must be one of {SELECT_MODES}")
    _cap_seed(seed)
    if max_num_neighbors is None:
        return None
    k = _cap_k(max_num_neighbors)
    if reference_ties:
        raise ValueError("max_num_neighbors with reference_ties=True: the cap is defined on the exact distance arithmetic "
                         "(reference_ties must be False)")
    return k


def float_keys_to_int64(key: torch.Tensor) -> torch.Tensor:
    """A floating tensor as int64 keys of the same order (torch ops, any device): a < b gives m(a) < m(b), a == b gives
    m(a) == m(b) (-0.0 and +0.0 are one key) - over negative values, subnormals and +-inf.  The value is widened to float64
    (exact), -0.0 folded into +0.0, and the bits of a negative value are flipped below the sign.  NaN has no place in the order:
    select_in_edges refuses it."""
    if not key.is_floating_point():
        raise ValueError(f"float_keys_to_int64 takes a floating tensor (got {key.dtype})")
    bits = (key.detach().to(torch.float64) + 0.0).contiguous().view(torch.int64)
    return bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFF)


def select_in_edges(csr: Csr, k: int, key: torch.Tensor):
    """Cap the in-degree of a destination `Csr` (gpde_csr_select_k): returns (Csr, edge_ids).
      - a row with at most k in-edges is kept whole; a longer row keeps the k slots with the smallest (key, slot) in
        lexicographic order - slots are distinct, so the choice is unique;
      - kept edges stay in ascending slot order inside their row: ascending source order, and with it the operator's summation
        order, is preserved; no atomics, two identical calls give identical bits;
      - the selection for k is a subset of the selection for any k' > k.
    `key`: int64 [E] in slot order (edge_sqdist_keys, edge_hash_keys, or the caller's), or a floating tensor, mapped to int64
    order-preservingly (float_keys_to_int64); NaN is refused.  One synchronisation: the new edge count (the NaN test rides on it).
    The new Csr has the gathered src / dst, the identity `perm`, `n_src_nodes` and the flow direction of the input and
    max_in_degree = min(old, k).  edge_ids int64 [E'] = csr.perm[kept slots]: the rows of any tensor that addressed the INPUT
    graph's edges - `edge_attr[edge_ids]`, `geom[edge_ids]` are the new graph's per-edge tensors, in its slot order.
    k >= csr.max_in_degree returns the same rows and slots, with edge_ids = perm."""
    k = _cap_k(k)
    if not isinstance(csr, Csr):
        raise ValueError(f"csr must be an ops.Csr (got {type(csr).__name__})")
    if not isinstance(key, torch.Tensor) or key.dim() != 1 or int(key.numel()) != csr.n_edges:
        got = tuple(key.shape) if isinstance(key, torch.Tensor) else type(key).__name__
        raise ValueError(f"key must be a tensor [{csr.n_edges}]: one key per CSR slot (got {got})")
    if key.dtype != torch.int64 and not key.is_floating_point():
        raise ValueError(f"key must be int64 or floating (got {str(key.dtype).replace('torch.', '')})")
    if key.device != csr.rowptr.device:
        raise ValueError(f"key is on {key.device}, the graph on {csr.rowptr.device}")
    _require_cuda(csr.rowptr, "csr")
    lib = _lib.lib()
    dev = csr.rowptr.device
    n, e = csr.n_nodes, csr.n_edges
    nan = torch.isnan(key).any() if key.is_floating_point() else torch.zeros((), dtype=torch.bool, device=dev)
    key = (float_keys_to_int64(key) if key.is_floating_point() else key.detach()).contiguous()
    rp = csr.rowptr.long()
    rowptr64 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum((rp[1:] - rp[:-1]).clamp(max=k), 0, out=rowptr64[1:])
    e_new, has_nan = (int(v) for v in torch.stack([rowptr64[-1], nan.to(torch.int64)]).cpu())
    if has_nan:
        raise ValueError("key holds NaN: a NaN has no place in the order of the keys")
    carry = dict(n_src_nodes=csr.n_src_nodes, _flow_flipped=csr._flow_flipped)
    if e_new == e:                                   # no row is longer than k: the same rows and slots
        out = Csr(n, e, csr.rowptr, csr.src, csr.dst, torch.arange(e, dtype=torch.int32, device=dev), _max_in_degree=csr._max_in_degree, **carry)
        return out, csr.perm.long()
    rowptr = rowptr64.to(torch.int32)
    slots = torch.empty(e_new, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_csr_select_k(csr.rowptr.contiguous().data_ptr(), key.data_ptr(), n, e, k, rowptr.data_ptr(), slots.data_ptr(),
                                         e_new, _stream_ptr(dev)), "gpde_csr_select_k")
    sl = slots.long()
    out = Csr(n, e_new, rowptr, csr.src[sl], csr.dst[sl], torch.arange(e_new, dtype=torch.int32, device=dev), _max_in_degree=k, **carry)
    return out, csr.perm[sl].long()              # (some row was longer than k: the largest in-degree is now k)


def _key_box(period, origin, dim: int):
    """`period` / `origin` of edge_sqdist_keys as two lists of `dim` floats (a scalar: every axis; 0 / None: an open axis)."""
    def per_axis(v, name):
        if v is None or isinstance(v, (int, float)):
            return [0.0 if v is None else float(v)] * dim
        v = [0.0 if t is None else float(t) for t in (v.tolist() if isinstance(v, torch.Tensor) else v)]
        if len(v) != dim:
            raise ValueError(f"{name} has {len(v)} entries for positions of dimension {dim}")
        return v
    per, org = per_axis(period, "period"), per_axis(origin, "origin")
    for a in range(dim):
        if not (0.0 <= per[a] < float("inf")) or not abs(org[a]) < float("inf"):
            raise ValueError(f"period[{a}] = {per[a]} must be >= 0 (0 = open axis) and origin[{a}] = {org[a]} finite")
    return per, org


def edge_sqdist_keys(csr: Csr, pos: torch.Tensor, pos_dst: Optional[torch.Tensor] = None, period=None, origin=None) -> torch.Tensor:
    """int64 [E] by CSR slot: the IEEE-754 bits of the float64 squared distance of every edge (gpde_edge_keys_sqdist) - the
    "nearest" key of select_in_edges (a non-negative double orders as its int64 bits).  `pos` [n_src, dim] are the positions
    `csr.src` indexes, `pos_dst` [n_nodes, dim] those of the destinations (None: one point set).  Open axes: d = pos_dst[i] -
    pos[j], d2 += d * d in axis order, unfused - the builders' exact arithmetic, bit for bit.  `period` / `origin` as in
    radius_csr: on a periodic axis d = pos[j] - pos_dst[i], d -= L rint(d / L) on the raw coordinates - the minimum-image
    difference in the form a float64 host computation follows operation by operation (it does not depend on `origin`)."""
    if not isinstance(csr, Csr):
        raise ValueError(f"csr must be an ops.Csr (got {type(csr).__name__})")
    for t, name, rows in ((pos, "pos", csr.n_src), (pos_dst, "pos_dst", csr.n_nodes)):
        if t is None and name == "pos_dst":
            if csr.n_src_nodes is not None and csr.n_src != csr.n_nodes:
                raise ValueError(f"a rectangular graph ({csr.n_src} sources, {csr.n_nodes} destinations) needs pos_dst")
            continue
        if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or int(t.size(0)) != rows:
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be a tensor [{rows}, dim] (or [{rows}]: one dimension): the points the graph was built on (got {got})")
    dim = 1 if pos.dim() == 1 else int(pos.size(1))
    if not 1 <= dim <= 3:
        raise ValueError(f"positions of dimension {dim}: the radius graphs are built in 1..3 dimensions")
    if pos_dst is not None and (1 if pos_dst.dim() == 1 else int(pos_dst.size(1))) != dim:
        raise ValueError("pos and pos_dst must have the same dimension")
    per, org = _key_box(period, origin, dim)
    lib = _lib.lib()
    pos, pd = _positions(pos, pos_dst)
    dev = pos.device
    if csr.rowptr.device != dev:
        raise ValueError(f"pos is on {dev}, the graph on {csr.rowptr.device}")
    keys = torch.empty(csr.n_edges, dtype=torch.int64, device=dev)
    per_c = (ctypes.c_double * dim)(*per) if any(per) else None
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_edge_keys_sqdist(pos.data_ptr(), pd.data_ptr(), dim, per_c, (ctypes.c_double * dim)(*org), csr.src.contiguous().data_ptr(),
                                             csr.dst.contiguous().data_ptr(), csr.n_edges, keys.data_ptr(), _stream_ptr(dev)),
                   "gpde_edge_keys_sqdist")
    return keys


def edge_hash_keys(src_ids: torch.Tensor, dst_ids: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """int64 [E]: a counter-based hash of (seed, dst id, src id) per edge (gpde_edge_keys_hash; the constants are stated in
    include/gpde.h) - the "random" key of select_in_edges.  It depends on the three numbers only - not on the slot order, the
    builder or k - so the k smallest keys of a row are a uniform k-subset of it, reproducible from the seed: under aggr='mean'
    the unbiased Monte-Carlo estimate of the full-ball mean.  The ids are explicit int32 vectors (`csr.src`, `csr.dst`; a batch
    passes graph-local ids)."""
    seed = _cap_seed(seed)
    for t, name in ((src_ids, "src_ids"), (dst_ids, "dst_ids")):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.int32:
            got = f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be an int32 vector [E] (got {got})")
    if src_ids.numel() != dst_ids.numel() or src_ids.device != dst_ids.device:
        raise ValueError(f"src_ids [{src_ids.numel()}] on {src_ids.device} and dst_ids [{dst_ids.numel()}] on {dst_ids.device} must match")
    _require_cuda(src_ids, "src_ids")
    lib = _lib.lib()
    dev = src_ids.device
    e = int(src_ids.numel())
    keys = torch.empty(e, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_edge_keys_hash(src_ids.contiguous().data_ptr(), dst_ids.contiguous().data_ptr(), e, seed, keys.data_ptr(),
                                           _stream_ptr(dev)), "gpde_edge_keys_hash")
    return keys


# ----------------------------------------------------------------------------------------------
# the radius graphs of a BATCH of point sets in one build (gpde_radius_csr_batched_*)
# ----------------------------------------------------------------------------------------------
def ptr_from_batch(batch: torch.Tensor, n_graphs: Optional[int] = None) -> torch.Tensor:
    """`ptr` int64 [B + 1] of PyG's sorted graph-id vector `batch` [n]: graph b owns the points ptr[b] .. ptr[b + 1].
    B = n_graphs, or batch.max() + 1 (graphs without points are legal anywhere when n_graphs is given).  ValueError for an
    unsorted or negative `batch`, or an id >= n_graphs.  Runs on the device of `batch`; host tensors need no device."""
    if batch.dim() != 1 or batch.is_floating_point() or batch.dtype == torch.bool:
        raise ValueError(f"batch must be a 1-D integer vector of graph ids (got {batch.dtype} {tuple(batch.shape)})")
    batch = batch.detach().to(torch.int64)
    n = int(batch.numel())
    if n > 0:
        if bool((batch[1:] < batch[:-1]).any()):
            raise ValueError("batch is not sorted: the points of a graph must be contiguous (PyG's Batch order)")
        if int(batch[0]) < 0:
            raise ValueError(f"batch holds the negative graph id {int(batch[0])}")
    top = int(batch[-1]) + 1 if n > 0 else 0
    b = top if n_graphs is None else int(n_graphs)
    if b < top:
        raise ValueError(f"batch holds graph id {top - 1}, n_graphs = {b}")
    ptr = torch.zeros(b + 1, dtype=torch.int64, device=batch.device)
    if n > 0:
        torch.cumsum(torch.bincount(batch, minlength=b), 0, out=ptr[1:])
    return ptr


_BATCHED_SINGLE_ONLY = ("period", "origin", "return_geometry")


def _host_ptr(ptr, name: str, n: int) -> torch.Tensor:
    """`ptr` as a host int64 [B + 1] tensor that starts at 0, never decreases and ends at n (ValueError otherwise)."""
    t = ptr.detach() if isinstance(ptr, torch.Tensor) else torch.as_tensor(ptr)
    if t.dim() != 1 or t.numel() < 1 or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"{name} must be a 1-D integer vector [B + 1] (got {t.dtype} {tuple(t.shape)})")
    t = t.to(device="cpu", dtype=torch.int64).contiguous()
    if int(t[0]) != 0:
        raise ValueError(f"{name}[0] = {int(t[0])}: {name} must start at 0")
    if bool((t[1:] < t[:-1]).any()):
        raise ValueError(f"{name} decreases: the points of a graph must be contiguous, graph after graph")
    if int(t[-1]) != n:
        raise ValueError(f"{name} ends at {int(t[-1])}, the position array has {n} points")
    return t


def batched_graph_args(pos, ptr, r, pos_dst=None, ptr_dst=None, unsupported=None):
    """Every argument check of the batched radius-graph builders, on HOST values only (ValueError; no device is needed to be
    refused): returns (dim, ptr host int64 [B + 1], ptr_dst host int64 [B + 1] or None, radii list of B floats)."""
    for k in (unsupported or {}):
        if k in _BATCHED_SINGLE_ONLY:
            raise ValueError(f"{k}= has no batched form: a periodic box, return_geometry, radius_in_degrees and the rank partitioner "
                             "keep their single-graph forms (ops.radius_csr / radius_csr_raw, one call per graph)")
        raise TypeError(f"unexpected keyword argument {k!r}")
    if not isinstance(pos, torch.Tensor) or pos.dim() not in (1, 2):
        raise ValueError("pos must be a tensor [n, dim] (or [n]: one dimension)")
    dim = 1 if pos.dim() == 1 else int(pos.size(1))
    if not 1 <= dim <= 3:
        raise ValueError(f"positions of dimension {dim}: the radius graphs are built in 1..3 dimensions")
    if ptr_dst is not None and pos_dst is None:
        raise ValueError("ptr_dst given without pos_dst: a second ptr needs the second point set it divides")
    if pos_dst is not None:
        if ptr_dst is None:
            raise ValueError("pos_dst given without ptr_dst: the second point set needs its own division into graphs")
        if not isinstance(pos_dst, torch.Tensor) or pos_dst.dim() not in (1, 2):
            raise ValueError("pos_dst must be a tensor [n_dst, dim] (or [n_dst]: one dimension)")
        if (1 if pos_dst.dim() == 1 else int(pos_dst.size(1))) != dim:
            raise ValueError("pos and pos_dst must have the same dimension")
    ptr_h = _host_ptr(ptr, "ptr", int(pos.size(0)))
    n_graphs = int(ptr_h.numel()) - 1
    ptr_dst_h = None
    if pos_dst is not None:
        ptr_dst_h = _host_ptr(ptr_dst, "ptr_dst", int(pos_dst.size(0)))
        if int(ptr_dst_h.numel()) != n_graphs + 1:
            raise ValueError(f"ptr_dst divides pos_dst into {int(ptr_dst_h.numel()) - 1} graphs, ptr divides pos into {n_graphs}")
    if isinstance(r, (int, float)):
        radii = [float(r)] * n_graphs
        if not (float(r) > 0.0 and float(r) != float("inf")):
            raise ValueError(f"r = {r} must be positive and finite")
    else:
        radii = [float(v) for v in (r.detach().reshape(-1).tolist() if isinstance(r, torch.Tensor) else list(r))]
        if len(radii) != n_graphs:
            raise ValueError(f"r has {len(radii)} entries for {n_graphs} graphs (a float, or one radius per graph)")
    for b, v in enumerate(radii):
        if not (v > 0.0 and v != float("inf")):
            raise ValueError(f"r[{b}] = {v} must be positive and finite")
    return dim, ptr_h, ptr_dst_h, radii


def batched_plan(bounds, ptr_src, ptr_dst, radii, dim: int):
    """gpde_radius_csr_batched_plan on host values: (table uint8 [B * GPDE_RADIUS_BATCHED_REC_BYTES] host tensor, n_cells,
    workspace bytes).  bounds: [B, 2, dim] float64 (host); ptr_src / ptr_dst: host int64 [B + 1] (ptr_dst None = ptr_src)."""
    lib = _lib.lib()
    n_graphs = int(ptr_src.numel()) - 1
    bounds = torch.as_tensor(bounds, dtype=torch.float64).reshape(n_graphs, 2, dim).contiguous()
    r_c = (ctypes.c_double * max(n_graphs, 1))(*radii)
    table = torch.zeros(max(n_graphs, 1) * _lib.GPDE_RADIUS_BATCHED_REC_BYTES, dtype=torch.uint8)
    n_cells, nbytes = ctypes.c_int64(0), ctypes.c_size_t(0)
    _lib.check(lib.gpde_radius_csr_batched_plan(bounds.data_ptr(), ptr_src.data_ptr(), None if ptr_dst is None else ptr_dst.data_ptr(),
                                                r_c, n_graphs, dim, table.data_ptr(), ctypes.byref(n_cells), ctypes.byref(nbytes)),
               "gpde_radius_csr_batched_plan")
    return table, int(n_cells.value), int(nbytes.value)


def _graph_ids(ptr_dev: torch.Tensor, n: int) -> torch.Tensor:
    """int64 [n]: the graph of every point of a ptr-divided array (on the device of ptr_dev; no sync)."""
    return torch.searchsorted(ptr_dev[1:].contiguous(), torch.arange(n, dtype=torch.int64, device=ptr_dev.device), right=True)


def radius_csr_batched(pos: torch.Tensor, ptr, r, *, pos_dst: Optional[torch.Tensor] = None, ptr_dst=None,
                       reference_ties: bool = False, max_num_neighbors: Optional[int] = None, select: str = "nearest", seed: int = 0,
                       **single_graph_only):
    """The radius graphs of B independent point sets in ONE build (gpde_radius_csr_batched_*): PyG's
    `radius_graph(pos, r, batch=batch)` as the block-diagonal `Csr` the operator consumes.  Graph b owns the points
    pos[ptr[b]:ptr[b + 1]] (`ptr` int64 [B + 1], see ptr_from_batch; pass it as a host tensor - a device tensor costs one more
    copy) and has radius r[b] (`r`: a float, or a sequence / tensor of B radii).  Returns (Csr, edge_ptr):
      Csr        global node ids, rows in ascending source order, `perm` the identity (edge attributes by CSR slot or NodeAttr) -
                 rowptr / src / dst are the per-graph `radius_csr` results concatenated with their offsets, bit for bit;
      edge_ptr   int64 [B + 1] = rowptr[ptr_dst]: graph b occupies the CSR slots edge_ptr[b] .. edge_ptr[b + 1].
    `pos_dst` with `ptr_dst`: two point sets per graph - edges (j in pos -> i in pos_dst), a rectangular Csr (`n_src_nodes`).
    Two synchronisations per call whatever B is (the per-graph bounds [B, 2, dim] and the edge count), one radix sort, four
    launches - against two synchronisations, a sort and four launches PER GRAPH of a loop over radius_csr.
    A periodic box, return_geometry, radius_in_degrees and the rank partitioner keep their single-graph forms.
    `max_num_neighbors` / `select` / `seed`: the capped in-degree of radius_csr, per graph - "random" hashes GRAPH-LOCAL node ids
    (global id minus the graph's ptr / ptr_dst entry), so for both modes the result is again the per-graph capped `radius_csr`
    results concatenated with their offsets, bit for bit; edge_ptr is taken from the new rowptr.  radius_graph_batched has no
    capped form."""
    k = _cap_args(max_num_neighbors, select, seed, reference_ties)
    dim, ptr_h, ptr_dst_h, radii = batched_graph_args(pos, ptr, r, pos_dst, ptr_dst, single_graph_only)
    lib = _lib.lib()
    pos, pd = _positions(pos, pos_dst)
    n, nd, n_graphs = int(pos.size(0)), int(pd.size(0)), int(ptr_h.numel()) - 1
    dev = pos.device
    ptr_d = ptr_h.to(dev)
    ptr_dst_d = ptr_d if ptr_dst_h is None else ptr_dst_h.to(dev)
    # per-graph bounds of both point sets, reduced on the device: ONE small copy [B, 2, dim] (graphs without points keep +-inf;
    # the plan does not read the bounds of a graph without sources)
    inf = float("inf")
    lo = torch.full((n_graphs, dim), inf, dtype=torch.float64, device=dev)
    hi = torch.full((n_graphs, dim), -inf, dtype=torch.float64, device=dev)
    for p, pt in ((pos, ptr_d),) if pd is pos else ((pos, ptr_d), (pd, ptr_dst_d)):
        if p.size(0) > 0 and n_graphs > 0:
            gid = _graph_ids(pt, int(p.size(0))).unsqueeze(1).expand(-1, dim).contiguous()
            lo.scatter_reduce_(0, gid, p, "amin")
            hi.scatter_reduce_(0, gid, p, "amax")
    bounds = torch.stack([lo, hi], dim=1).cpu()
    table_h, n_cells, nbytes = batched_plan(bounds, ptr_h, ptr_dst_h, radii, dim)
    table = table_h.to(dev)
    ws = _alloc_ws(nbytes, dev)
    flags = 1 if reference_ties else 0
    ptr_dst_c = ptr_h if ptr_dst_h is None else ptr_dst_h
    deg = torch.zeros(nd, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_csr_batched_count(pos.data_ptr(), n, pd.data_ptr(), nd, dim, flags, ptr_h.data_ptr(), ptr_dst_c.data_ptr(),
                                                     n_graphs, table.data_ptr(), n_cells, deg.data_ptr(), ws.data_ptr(), ws.numel(),
                                                     _stream_ptr(dev)), "gpde_radius_csr_batched_count")
    rowptr64 = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=rowptr64[1:])
    edge_ptr = rowptr64[ptr_dst_d]
    e = int(rowptr64[-1].item())
    if e >= (1 << 31) - 64:
        raise NotImplementedError(f"{e} edges exceed the int32 CSR")
    rowptr = rowptr64.to(torch.int32)
    src = torch.empty(e, dtype=torch.int32, device=dev)
    dst = torch.empty(e, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpde_radius_csr_batched_fill(pos.data_ptr(), n, pd.data_ptr(), nd, dim, flags, ptr_h.data_ptr(), ptr_dst_c.data_ptr(),
                                                    n_graphs, table.data_ptr(), n_cells, rowptr.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                                    e, ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "gpde_radius_csr_batched_fill")
    csr = Csr(nd, e, rowptr, src, dst, torch.arange(e, dtype=torch.int32, device=dev), n_src_nodes=None if pos_dst is None else n)
    if k is None:
        return csr, edge_ptr
    if select == "nearest":
        key = edge_sqdist_keys(csr, pos, None if pos_dst is None else pd)        # global ids into the concatenated positions
    else:
        g = _graph_ids(ptr_dst_d, nd)[dst.long()] if e > 0 else torch.zeros(0, dtype=torch.int64, device=dev)   # the graph of every edge
        key = edge_hash_keys((src.long() - ptr_d[g]).to(torch.int32), (dst.long() - ptr_dst_d[g]).to(torch.int32), seed)
    csr, _ = select_in_edges(csr, k, key)
    return csr, csr.rowptr.long()[ptr_dst_d]


def radius_graph_batched(pos: torch.Tensor, ptr, r, *, pos_dst: Optional[torch.Tensor] = None, ptr_dst=None,
                         reference_ties: bool = False, **single_graph_only):
    """(edge_index int64 [2, E], edge_ptr int64 [B + 1]) of the same batch (arguments of radius_csr_batched): every graph in the
    reference's source-major order, graph after graph, global node ids - exactly what collating the per-sample `radius_graph`
    edge lists gives.  It is the batched CSR stably sorted by source (graph b's edges are edge_index[:, edge_ptr[b]:edge_ptr[b + 1]])."""
    csr, edge_ptr = radius_csr_batched(pos, ptr, r, pos_dst=pos_dst, ptr_dst=ptr_dst, reference_ties=reference_ties, **single_graph_only)
    order = torch.sort(csr.src, stable=True).indices            # rows are destination-major: targets stay ascending per source
    return torch.stack([csr.src[order].long(), csr.dst[order].long()]), edge_ptr


# ----------------------------------------------------------------------------------------------
# GCNConv (include/gpde.h gpde_gcn_norm / gpde_gcn_fwd / gpde_gcn_plan; csrc/gpde_gcn.hip)
# ----------------------------------------------------------------------------------------------
GCN_ADD_SELF_LOOPS, GCN_IMPROVED, GCN_NORMALIZE = 1, 2, 4        # gpde_gcn_norm flags (tests/test_gcn_host.py checks them against the header)
GCN_RELU = 1                                                     # gpde_gcn_fwd flag
GCN_ROUTES = ("aggregate_first", "aggregate_mm", "transform_first")


class GcnNorm:
    """The symmetric normalisation of one graph: `coef` [E] by CSR slot and `self_coef` [N] (gpde_gcn_norm) on `csr`, and - built
    on first use, in a backward - the same pair for the REVERSED graph (`reversed`): the backward of the aggregation is the
    aggregation over the transposed matrix, and a graph with an edge j -> i need not hold i -> j."""

    def __init__(self, csr: Csr, coef: torch.Tensor, self_coef: torch.Tensor, flags: int):
        self.csr, self.coef, self.self_coef, self.flags = csr, coef, self_coef, flags
        self._rec = Cached(buffers=(coef, self_coef, csr.rowptr, csr.src, csr.dst, csr.perm))      # stamped by gcn_norm after its kernel
        self._reversed: Optional[Cached] = None     # value: the reversed pair

    def order(self):
        """A hit on this normalisation, from the cache of gcn_norm or from a module that pinned it (GCNConv(cached=True))."""
        self._rec.hit("gcn_norm")

    def records(self) -> list:
        return [self._rec] if self._reversed is None else [self._rec, self._reversed]

    @property
    def reversed(self):
        """(csr_rev, coef_rev): the CSR of the edge list with its rows swapped and each reversed slot's coefficient.  It is built
        from the forward CSR's own slot-order edge list (`Csr.edge_index`, flip=True), so its `perm` maps reversed slots to forward
        slots directly - one gather - and a `Csr` handed in without an edge_index tensor, or a flipped flow, is no special case.
        The diagonal (self_coef) is its own transpose."""
        if self._reversed is None:
            csr = self.csr
            if csr.n_edges == 0:
                self._reversed = Cached((csr, self.coef))        # (the forward arrays: nothing of its own to order)
            else:
                rev = build_csr(csr.edge_index, csr.n_nodes, flip=True)
                coef = gather_rows(self.coef.view(-1, 1), rev.perm).view(-1)
                self._reversed = Cached((rev, coef), (rev.rowptr, rev.src, rev.dst, rev.perm, coef)).stamp(coef.device)
        else:
            self._reversed.hit("gcn_norm")
        return self._reversed.value


# value: the GcnNorm (it orders its own hits); pins: the Csr and the edge_weight storage; nbytes: what the entry keeps alive - the CSR,
# the coefficients and - after a backward - the same again
_gcn_norm_cache = Lru("gcn_norm", max_entries=64, max_bytes=1 << 30)


def gcn_flags(improved: bool = False, add_self_loops: bool = True, normalize: bool = True) -> int:
    return (GCN_IMPROVED if improved else 0) | (GCN_ADD_SELF_LOOPS if add_self_loops else 0) | (GCN_NORMALIZE if normalize else 0)


def gcn_norm(csr: Csr, edge_weight: Optional[torch.Tensor] = None, improved: bool = False, add_self_loops: bool = True,
             normalize: bool = True) -> GcnNorm:
    """gpde_gcn_norm, cached next to the CSR cache: PyG's `gcn_norm` with `add_remaining_self_loops` on the destination CSR.

    coef_e = dinv[src] w_e dinv[dst] per CSR slot, self_coef_i = dinv[i]^2 * (self weight), dinv = deg^-1/2.  The degree is the
    TARGET-side sum - deg[i] = the weights of the in-edges of i plus the self weight - as in PyG 1.6 and later; older PyG summed
    over the source row, which is the same number on the symmetric graphs the reference's scripts use.  Every node gets exactly one
    self loop of weight 1 (`improved`: 2); a node that already has self-loop edges takes the weight of the one with the largest
    original edge id, and every self-loop slot gets coef = 0.  `add_self_loops=False`: no self term, existing self loops stay
    ordinary edges.  `normalize=False`: coef = w, self_coef = 0.  `edge_weight` [E] is in the ORIGINAL edge order.

    Key: the Csr object (csr_for keys it on edge_index identity and version), edge_weight storage / layout / version, the flags -
    the 16 convs of one GCN_Net forward share one normalisation.  Square graphs only."""
    if not isinstance(csr, Csr):
        raise TypeError(f"gcn_norm takes an ops.Csr (ops.csr_for(edge_index, n_nodes)), got {type(csr).__name__}")
    if csr.n_src_nodes is not None:
        raise ValueError(f"GCN is defined on one node set: the CSR joins {csr.n_src_nodes} sources to {csr.n_nodes} destinations")
    flags = gcn_flags(bool(improved), bool(add_self_loops), bool(normalize))
    wkey = None
    if edge_weight is not None:
        if edge_weight.requires_grad:
            raise NotImplementedError("the gradient with respect to edge_weight is not built: pass edge_weight.detach()")
        watch(edge_weight)
        wkey = mem_key(edge_weight)
    key = (id(csr), wkey, flags)
    hit = _gcn_norm_cache.get(key)
    if hit is not None:
        hit.value.order()
        return hit.value
    lib = _lib.lib()
    _require_cuda(csr.rowptr, "csr")
    dev = csr.rowptr.device
    n, e = csr.n_nodes, csr.n_edges
    ew = _operand(edge_weight, "edge_weight", (e,), dev)
    coef = torch.empty(e, dtype=torch.float32, device=dev)
    self_coef = torch.empty(n, dtype=torch.float32, device=dev)
    ws = _alloc_ws(int(lib.gpde_gcn_norm_workspace_bytes(n, e)), dev)
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    _call("gpde_gcn_norm", dev, csr.rowptr.data_ptr(), p(csr.src), p(csr.perm), p(ew), n, e, flags, p(coef), p(self_coef), ws.data_ptr(), ws.numel())
    norm = GcnNorm(csr, coef, self_coef, flags)
    norm._rec.stamp(dev)
    # bytes an entry keeps alive once the CSR cache has let go of the graph: rowptr / src / dst / perm, coef, self_coef, edge_weight -
    # counted twice, for the reversed graph a backward adds (GcnNorm.reversed)
    nbytes = 2 * (16 * e + 8 * n + 4) + (0 if edge_weight is None else 4 * e)
    _gcn_norm_cache.put(key, Cached(norm, (), (csr, None if edge_weight is None else edge_weight.untyped_storage()), nbytes))
    return norm


def gcn_plan(in_channels: int, out_channels: int) -> dict:
    """gpde_gcn_plan: the tiling gpde_gcn_fwd runs at these widths (host arithmetic, no device): destination rows per workgroup,
    LDS row stride, channel passes per lane of the aggregation, 32-column blocks of the product, column blocks per wave, K tail,
    column tail, LDS bytes."""
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().gpde_gcn_plan(int(in_channels), int(out_channels), out), "gpde_gcn_plan")
    return dict(zip(("rows", "kstride", "passes", "col_blocks", "col_blocks_per_wave", "k_tail", "col_tail", "lds_bytes"),
                    (int(v) for v in out)))


def gcn_route(in_channels: int, out_channels: int) -> str:
    """Which of GCN_ROUTES gcn_forward_raw takes by default:
      'aggregate_first'   (A x) W in ONE launch of the fused kernel (aggregation, then the multiply on the LDS tile);
      'aggregate_mm'      the aggregation kernel (W = NULL) at width `in`, then torch.mm;
      'transform_first'   A (x W): torch.mm, then the aggregation kernel at width `out`.
    The rule is what scripts/bench_gcn.py measured on the 421^2 grid (profiles/gcn_bench.txt): the fused kernel
    was slower than 'aggregate_mm' at every width class (0.31 against 0.22 ms at 128 -> 128, 1.13 against 0.51 ms at 256 -> 256),
    so it is never the default - it stays reachable, and tested, through `route=`; of the other two the narrower gather wins
    by about 30 % (in < out: 'aggregate_mm', in > out: 'transform_first'); at in = out they measured within 4 % of each other - a
    tie, which goes to 'transform_first'."""
    return "aggregate_mm" if int(in_channels) < int(out_channels) else "transform_first"


def _gcn_call(x, csr: Csr, coef, self_coef, w, bias, cin: int, cout: int, relu: bool, want_agg: bool):
    n, e, dev = csr.n_nodes, csr.n_edges, x.device
    out = torch.empty(n, cout, dtype=torch.float32, device=dev)
    agg = torch.empty(n, cin, dtype=torch.float32, device=dev) if want_agg else None
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    _call("gpde_gcn_fwd", dev, p(x), n, e, csr.rowptr.data_ptr(), p(csr.src), p(coef), p(self_coef), p(w), p(bias), cin, cout,
          GCN_RELU if relu else 0, p(out), p(agg))
    return out, agg


def gcn_forward_raw(x: torch.Tensor, norm: GcnNorm, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor] = None,
                    relu: bool = False, route: Optional[str] = None, agg_out: bool = False, reverse: bool = False):
    """out = act((A x) W + bias), A = the normalised adjacency of `norm` (`reverse`: its transpose - the backward's operator).
    x [N, in]; weight [in, out] or None (the aggregation alone, out = in); bias [out] or None.  `route`: None = gcn_route(in, out),
    or one of GCN_ROUTES to force it; `agg_out` (the two aggregate routes): also return A x [N, in], the rows before the multiply.
    Returns out, or (out, agg) with `agg_out`."""
    _require_cuda(x, "x")
    if not isinstance(norm, GcnNorm):
        raise TypeError(f"norm must be the result of ops.gcn_norm, got {type(norm).__name__}")
    dev = x.device
    csr, coef = norm.reversed if reverse else (norm.csr, norm.coef)
    n = csr.n_nodes
    x_c = _operand(x, "x", (n, None), dev)
    cin = int(x_c.size(1))
    if weight is not None and weight.dim() != 2:
        raise ValueError(f"weight must be float32 [{cin},*] on {dev}, got {tuple(weight.shape)}")
    cout = cin if weight is None else int(weight.size(1))
    if not (width_supported(cin, cin) and (weight is None or width_supported(cin, cout))):
        raise NotImplementedError(f"in_channels {cin} -> out_channels {cout}: the native GCN operator is built for widths 1 .. {ANY_MAX_WIDTH}")
    w_c = _operand(weight, "weight", (cin, cout), dev)
    b_c = _operand(bias, "bias", (cout,), dev)
    if csr.rowptr.device != dev:
        raise ValueError(f"the graph lives on {csr.rowptr.device}, x on {dev}")
    if route is None:
        route = "aggregate_first" if weight is None else gcn_route(cin, cout)
    if route not in GCN_ROUTES:
        raise ValueError(f"route must be one of {GCN_ROUTES} or None, got {route!r}")
    if route == "transform_first" and weight is not None:
        if agg_out:
            raise ValueError("agg_out is the aggregate routes' by-product: transform_first never forms A x")
        out, _ = _gcn_call(torch.mm(x_c, w_c), csr, coef, norm.self_coef, None, b_c, cout, cout, relu, False)
        return out
    if route == "aggregate_mm" and weight is not None:
        agg, _ = _gcn_call(x_c, csr, coef, norm.self_coef, None, None, cin, cin, False, False)
        out = torch.mm(agg, w_c) if b_c is None else torch.addmm(b_c, agg, w_c)
        if relu:
            out.clamp_min_(0)
        return (out, agg) if agg_out else out
    out, agg = _gcn_call(x_c, csr, coef, norm.self_coef, w_c, b_c, cin, cout, relu, agg_out)
    return (out, agg) if agg_out else out


# ----------------------------------------------------------------------------------------------
# the diagonal-kernel operator (include/gpde.h gpde_diagconv_*; csrc/gpde_diagconv.hip): k [E, w] per edge, message x_j (.) k_e
# ----------------------------------------------------------------------------------------------
_DIAG_PLAN_KEYS = ("V", "LC", "ES", "pass_edges", "chain_edges", "lanes", "per_lane", "consecutive", "active_lanes", "lds_bytes")


def diag_plan(w: int, aligned: bool = True, aggr: str = "add") -> dict:
    """gpde_diagconv_plan: the lane tiling gpde_diagconv.hip runs at width `w` - V (floats per access), LC (column lanes), ES (edge
    slots per wave), the in-edges of a pass (in flight before the first FMA) and of a chain (the first level of the two-level row
    sum), the lanes that hold a slot, channels per column lane, whether a lane's channels are consecutive (w % 4 == 0), the lanes
    that own a channel, LDS bytes.  `aligned`: every buffer of the call is 16-byte aligned (else V = 1 at every width; the tiling
    and the summation order do not change).  Host arithmetic, no device."""
    if aggr not in _AGGR_WE:
        raise NotImplementedError(f"aggr={aggr!r}")
    out = (ctypes.c_int32 * len(_DIAG_PLAN_KEYS))()
    _lib.check(_lib.lib().gpde_diagconv_plan(int(w), 1 if aligned else 0, _AGGR_WE[aggr], out), "gpde_diagconv_plan")
    return dict(zip(_DIAG_PLAN_KEYS, (int(v) for v in out)))


def _diag_args(x_src, x_dst, csr: Csr, edge_kernel, root):
    """The node tables, k [E, w] and root of a diagonal call checked; (w, in_dst).  `x_dst`: _ONE_SET, a tensor or None, as
    `_any_args` takes it."""
    one = x_dst is _ONE_SET
    n_dst, e = csr.n_nodes, csr.n_edges
    n_src = n_dst if one else csr.n_src
    if one and csr.n_src != n_dst:
        raise ValueError(f"a call on one node set needs a square graph, got {csr.n_src} sources and {n_dst} destinations")
    if x_src.dtype != torch.float32 or x_src.dim() != 2 or x_src.size(0) != n_src or x_src.size(1) < 1:
        raise ValueError(f"{_x_name(x_dst)} must be float32 [{n_src}, width], got {x_src.dtype} {tuple(x_src.shape)}")
    dev, w = x_src.device, int(x_src.size(1))
    if not one and x_dst is not None and (x_dst.dtype != torch.float32 or x_dst.dim() != 2 or x_dst.size(0) != n_dst or x_dst.size(1) < 1 or
                                          x_dst.device != dev):
        raise ValueError(f"x_dst must be float32 [{n_dst}, in_dst] on {dev}, got {x_dst.dtype} {tuple(x_dst.shape)}")
    cind = w if one or x_dst is None else int(x_dst.size(1))
    if edge_kernel.dtype != torch.float32 or tuple(edge_kernel.shape) != (e, w) or edge_kernel.device != dev:
        raise ValueError(f"edge_kernel must be float32 [{e},{w}] (one value per edge and channel of {_x_name(x_dst)}) on {dev}, got "
                         f"{edge_kernel.dtype} {tuple(edge_kernel.shape)}")
    if root is not None and x_dst is None:
        raise ValueError("root without x_dst: the root term is x_dst . root (pass root=None for a call without destination features)")
    if root is not None and (root.dtype != torch.float32 or tuple(root.shape) != (cind, w) or root.device != dev):
        raise ValueError(f"root must be float32 [{cind},{w}] on {dev}, got {root.dtype} {tuple(root.shape)}")
    if csr.rowptr.device != dev:
        raise ValueError(f"the graph lives on {csr.rowptr.device}, {_x_name(x_dst)} on {dev}")
    if not (width_supported(w, w) and width_supported(cind, w)):
        raise NotImplementedError(f"width {w} (in_dst {cind}): the native diagonal operator is built for widths 1 .. {ANY_MAX_WIDTH}")
    return w, cind


def _diag_tables(xs, xd, csr: Csr):
    """(x_src ptr, n_src, x_dst ptr, n_dst) of a native call: one node set hands one table twice."""
    if xd is _ONE_SET:
        return xs.data_ptr(), csr.n_nodes, xs.data_ptr(), csr.n_nodes
    return xs.data_ptr(), csr.n_src, _ptr(xd), csr.n_nodes


def diagconv_forward_raw(x_src, x_dst, csr: Csr, edge_kernel, root, bias, aggr: str, residual=None, relu: bool = False):
    """gpde_diagconv_fwd: out_i = aggr_{e: j -> i} x_src[j] * edge_kernel[e] + x_dst[i] . root + bias (+ residual, ReLU) in one
    launch.  x_src [n_src, w]; `x_dst` ops._ONE_SET (one node set: x_src is the table of the root term too), a tensor [n_dst, in_dst]
    or None (no root term: root must be None); edge_kernel [E, w] in CSR slot order; root [in_dst, w], bias [w], residual
    [n_dst, w] or None; aggr add / mean / max.  Operands are made dense, nothing more: one that starts off a 16-byte boundary takes
    the dword route (the same bits).  The result is a fresh tensor: this wrapper takes no caller-given output (DESIGN.md "Operand
    layouts" holds every public `out=` to 16-byte alignment, and this kernel's dword route exists for buffers that are not)."""
    return _diagconv_forward(x_src, x_dst, csr, edge_kernel, root, bias, aggr, residual, relu, None)


def _diagconv_forward(x_src, x_dst, csr: Csr, edge_kernel, root, bias, aggr: str, residual, relu: bool, out):
    """The body of diagconv_forward_raw.  `out`: None, or the float32 [n_dst, w] tensor to write - dense, any 4-byte alignment (off a
    16-byte boundary the kernel takes its dword route), not x_src's or residual's memory; validated here (the tests reach the dword
    stores through it)."""
    _require_cuda(x_src, _x_name(x_dst))
    if aggr not in _AGGR_WE:
        raise NotImplementedError(f"aggr={aggr!r}")
    xs, xd, k, root_c = _dense(x_src), _dense(x_dst), _dense(edge_kernel), _dense(root)
    w, cind = _diag_args(xs, xd, csr, k, root_c)
    n_dst, dev = csr.n_nodes, xs.device
    bias_c = _any_f32(bias, "bias", (w,), dev)
    res = _any_f32(residual, "residual", (n_dst, w), dev)
    if out is None:
        out = torch.empty(n_dst, w, dtype=torch.float32, device=dev)
    else:
        if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (n_dst, w) or out.device != dev:
            raise ValueError(f"out must be float32 [{n_dst},{w}] on {dev}, got "
                             f"{(out.dtype, tuple(out.shape), out.device) if torch.is_tensor(out) else type(out).__name__}")
        if not out.is_contiguous():
            raise ValueError(f"out is written by the kernel in place: it must be contiguous, got strides {tuple(out.stride())} (views are "
                             "not copied)")
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * 4
        for t, nm in ((xs, _x_name(x_dst)), (res, "residual")):
            if t is not None and t.numel() and lo < t.data_ptr() + t.numel() * 4 and t.data_ptr() < hi:
                raise ValueError(f"out shares memory with {nm}: other waves still read those rows")
    _call("gpde_diagconv_fwd", dev, *_diag_tables(xs, xd, csr), k.data_ptr(), csr.n_edges, csr.rowptr.data_ptr(), csr.src.data_ptr(),
          _ptr(root_c), _ptr(bias_c), _ptr(res), 1 if relu else 0, _AGGR_WE[aggr], w, cind, out.data_ptr())
    return out


def diagconv_backward_raw(x_src, x_dst, csr: Csr, edge_kernel, root, aggr: str, grad_out, need_x_src: bool = True, need_x_dst: bool = True,
                          need_root: bool = True, need_bias: bool = True):
    """gpde_diagconv_bwd ('add' / 'mean').  Returns (grad_x_src [n_src, w], grad_x_dst [n_dst, in_dst], grad_edge_kernel [E, w],
    grad_root [in_dst, w], grad_bias [w]); an output that is not needed or has no input (x_dst / root None) is None.  One node set
    (`x_dst` ops._ONE_SET): grad_x_dst is None and grad_x_src holds both terms, the source sum and g . root^T.  grad_x_src is summed
    by one owner per source in ascending slot order (csr.src_order), never by atomics."""
    lib = _lib.lib()
    for t, nm in ((x_src, _x_name(x_dst)), (edge_kernel, "edge_kernel"), (grad_out, "grad_out")):
        _require_cuda(t, nm)
    if aggr not in _AGGR:
        raise NotImplementedError(f"aggr={aggr!r}: the gradient of the diagonal operator is built for 'add' and 'mean'")
    one = x_dst is _ONE_SET
    xs, xd, k, root_c = _dense(x_src), _dense(x_dst), _dense(edge_kernel), _dense(root)
    w, cind = _diag_args(xs, xd, csr, k, root_c)
    n_src, n_dst, e, dev = int(xs.size(0)), csr.n_nodes, csr.n_edges, xs.device
    grad_out = _any_grad_out(grad_out, n_dst, w)
    new = lambda want, *shape: torch.empty(*shape, dtype=torch.float32, device=dev) if want else None
    # (two node sets given the SAME memory twice: the library reads "one table twice and no grad_x_dst" as one node set and would
    # add g . root^T to grad_x_src - such a call always takes its grad_x_dst, needed or not)
    same_table = not one and xd is not None and xd.data_ptr() == xs.data_ptr() and n_src == n_dst and cind == w
    gxs, gxd = new(need_x_src, n_src, w), new((need_x_dst or same_table) and not one and xd is not None, n_dst, cind)
    gk = new(True, e, w)
    groot, gbias = new(need_root and root is not None, cind, w), new(need_bias, w)
    ws = _alloc_ws(int(lib.gpde_diagconv_bwd_workspace_bytes(n_dst, w, cind)), dev)
    if need_x_src and e > 0:
        if DX_MODE == "atomic":
            raise NotImplementedError("GPDE_BWD_DX=atomic: the diagonal operator sums grad_x per source in slot order only")
        srp, ssl = csr.src_order
    else:
        srp, ssl = None, None
    _call("gpde_diagconv_bwd", dev, *_diag_tables(xs, xd, csr), k.data_ptr(), e, csr.rowptr.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(),
          _ptr(srp), _ptr(ssl), _ptr(root_c), _AGGR[aggr], w, cind, grad_out.data_ptr(), _ptr(gxs), _ptr(gxd), gk.data_ptr(), _ptr(groot),
          _ptr(gbias), ws.data_ptr(), ws.numel())
    return gxs, (gxd if need_x_dst else None), gk, groot, gbias


# ... streamed (include/gpde.h gpde_nnconv_*_chain_any; csrc/gpde_chain_any.hip): the route's block tables and its two wrappers live in
# chain_any.py and are reached through this module like every other entry point (imported last: chain_any.py uses the helpers above)
from .chain_any import (ChainBlocks, chain_any_blocks, chain_any_table, nnconv_backward_chain_any_raw,      # noqa: E402,F401
                        nnconv_forward_chain_any_raw)
