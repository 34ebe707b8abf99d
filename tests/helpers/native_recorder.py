"""What the 64-wide wrappers of ops.py hand to libgpde.so, recorded on the CPU: the library is replaced by a stub that notes every
call, the wrappers run on CPU tensors, and each argument is written down by what it IS - a scalar's value, the name of the
caller's tensor a pointer belongs to, `ret[i]` for a tensor the wrapper returned, "new" for anything the wrapper allocated,
None for NULL.  tests/golden/native_calls_w64.json is this record of the table of forms below
(tests/golden/make_native_calls.py); tests/test_native_calls_host.py holds the wrappers to it.  No GPU, no library."""
import contextlib
import ctypes
import zlib
from unittest import mock

import torch

from graph_pde_amd import _lib, ops

N, E, K0, K2 = 6, 9, 3, 32                  # the fixture graph of tests/test_layouts_host.py
DIMS = (K0, 16, K2, 4096)
K2P = 128
W = 64


def is_query(name: str) -> bool:
    return "workspace_bytes" in name


def query_bytes(name: str) -> int:
    """What the stub answers a `*workspace_bytes*` query: a multiple of 256, fixed per query name."""
    return 256 * (zlib.crc32(name.encode()) % 4093 + 1)


class RecordingLibrary:
    """Stands in for the ctypes library: every attribute is a function that notes (name, args) and returns 0 - a workspace
    query its fixed size, an entry point with scripted return codes the next of them."""

    def __init__(self, script=None):
        self.calls = []
        self.script = {k: list(v) for k, v in (script or {}).items()}

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if is_query(name):
                return query_bytes(name)
            if name == "gpde_last_error":
                return b"scripted"
            codes = self.script.get(name)
            return codes.pop(0) if codes else 0
        return fn


@contextlib.contextmanager
def recording(script=None):
    """The stub in place of the library, CPU tensors accepted, and the module's environment switches at their defaults."""
    stub = RecordingLibrary(script)
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(_lib, "lib", lambda: stub))
        st.enter_context(mock.patch.object(ops, "_require_cuda", lambda t, name: None))
        st.enter_context(mock.patch.object(ops, "_stream_ptr", lambda dev: 0))
        st.enter_context(mock.patch.object(torch.cuda, "device", lambda dev: contextlib.nullcontext()))
        st.enter_context(mock.patch.object(ops, "DEFAULT_PRECISION", "f16split"))
        st.enter_context(mock.patch.object(ops, "DX_MODE", "ordered"))
        st.enter_context(mock.patch.object(ops, "BWD_WS_FRACTION", 0.0))
        st.enter_context(mock.patch.object(ops, "ATTR_SLOT_ORDER", True))
        yield stub


def graph(max_in_degree=2):
    rowptr = torch.tensor([0, 2, 4, 5, 7, 9, 9], dtype=torch.int32)
    src = torch.arange(E, dtype=torch.int32) % N
    dst = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), (rowptr[1:] - rowptr[:-1]).long())
    csr = ops.Csr(N, E, rowptr, src, dst, torch.arange(E, dtype=torch.int32), _max_in_degree=max_in_degree)
    csr._src_order = (torch.zeros(N + 1, dtype=torch.int32), torch.zeros(E, dtype=torch.int32))
    csr._rowptr_host = rowptr.clone()        # (on the CPU `rowptr.cpu()` is rowptr itself: two names would share one pointer)
    return csr


def named_args():
    """The caller's side of every form: fresh tensors under the names the record uses."""
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(
        x=r(N, W), csr=graph(), ea=r(E, K0), pm=ops.PackedMlp(DIMS, torch.zeros(4), _lib.dims_array(DIMS)),
        root=r(W, W), bias=r(W), hidden=r(E, K2P), hmax=torch.ones(1), g=r(N, W), residual=r(N, W),
        na=ops.NodeAttr(r(N, K0), [(0, 0), (1, 1), (0, 2)]),
        w=[r(16, K0), r(K2, 16), r(W * W, K2)], b=[r(16), r(K2), r(W * W)],
        out=torch.zeros(N, W), ws=torch.zeros(4096, dtype=torch.uint8), z=torch.zeros(N, W * K2P),
        gh=r(E, K2P), acc=torch.zeros(E, K2P), x1=r(N, W), x2=r(N, W), g1=r(N, W), g2=r(N, W),
        ea_sorted=r(E, K0), identity=torch.arange(E, dtype=torch.int32),
        we=r(E, W * W), we2=r(E, W * W), csr2=graph(), gwe=r(E, W * W),
        acc_we=[torch.zeros(E, W * W), torch.zeros(W, W), torch.zeros(W)])


def _names(a):
    """data_ptr -> name over everything in `a` that owns device memory a pointer argument can equal."""
    out = {}

    def put(t, name):
        if isinstance(t, torch.Tensor) and t.numel() > 0:
            out.setdefault(t.data_ptr(), name)
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            put(v, k)
        elif isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                put(t, f"{k}[{i}]")
        elif isinstance(v, ops.NodeAttr):
            put(v.table, f"{k}.table")
        elif isinstance(v, ops.PackedMlp):
            put(v.packed, f"{k}.packed")
        elif isinstance(v, ops.Csr):
            for f in ("rowptr", "src", "dst", "perm", "_rowptr_host"):
                put(getattr(v, f), f"{k}.{f.lstrip('_')}")
            if v._src_order is not None:
                put(v._src_order[0], f"{k}.src_rowptr")
                put(v._src_order[1], f"{k}.src_slots")
    return out


def _returned(ret, path="ret", out=None):
    out = {} if out is None else out
    if isinstance(ret, torch.Tensor):
        if ret.numel() > 0:
            out.setdefault(ret.data_ptr(), path)
    elif isinstance(ret, (list, tuple)):
        for i, r in enumerate(ret):
            _returned(r, f"{path}[{i}]", out)
    return out


def _describe(ret):
    if isinstance(ret, torch.Tensor):
        return [str(ret.dtype).replace("torch.", ""), list(ret.shape)]
    if isinstance(ret, (list, tuple)):
        return [_describe(r) for r in ret]
    return ret


def _normalise(name, args, ptr_name):
    """One call's arguments by position (`_lib.SIGNATURES[name]` says which are pointers)."""
    argtypes = _lib.SIGNATURES[name][1]
    assert len(argtypes) == len(args), (name, len(argtypes), len(args))
    ptr = lambda p: None if not p else ptr_name.get(int(p), "new")        # (NULL comes as None or as 0)
    out = []
    for ct, a in zip(argtypes, args):
        if ct is not ctypes.c_void_p:
            out.append(int(a) if not isinstance(a, float) else a)
        elif a is None:
            out.append(None)
        elif isinstance(a, ctypes.Array) and issubclass(a._type_, ctypes.Structure):
            assert a._type_ is _lib.GpdeWeConvDesc, a._type_
            out.append([{f: ptr(getattr(d, f)) if ct is ctypes.c_void_p else int(getattr(d, f)) for f, ct in d._fields_} for d in a])
        elif isinstance(a, ctypes.Array):
            out.append([ptr(v) for v in a] if a._type_ is ctypes.c_void_p else [int(v) for v in a])
        elif hasattr(a, "_obj"):                      # ctypes.byref(...)
            o = a._obj
            assert isinstance(o, _lib.GpdeNodeAttr), type(o)
            out.append({"table": ptr(o.table), "stride": int(o.stride), "n_slots": int(o.n_slots), "sel": [int(s) for s in o.sel]})
        else:
            out.append(ptr(a))
    return out


def record(form):
    """{"wrapper", "calls": [[entry point, [arguments]]...], "returns" | "raises"} of one form: `form` = (id, wrapper name,
    callable taking the dict of named_args(), scripted return codes or None)."""
    _, wrapper, call, script = form
    a = named_args()
    rec = {"wrapper": wrapper}
    with recording(script) as stub:
        try:
            ret = call(a)
        except Exception as exc:                       # noqa: BLE001  (the refusal IS the record)
            ret = None
            rec["raises"] = [type(exc).__name__, str(exc)]
        else:
            rec["returns"] = _describe(ret)
    ptr_name = _returned(ret)
    ptr_name.update(_names(a))                          # (a returned tensor that the caller gave keeps the caller's name)
    rec["calls"] = [[name, _normalise(name, args, ptr_name)] for name, args in stub.calls]
    return rec


def operator_calls(rec):
    """The record without its workspace queries (their number may change; what reaches an entry point may not)."""
    return dict(rec, calls=[c for c in rec["calls"] if not is_query(c[0])])


# ---------------------------------------------------------------------------------------------------------------------------
# the table of forms
# ---------------------------------------------------------------------------------------------------------------------------
def _with(a, **over):
    a.update(over)
    return a


def _slot_order_patched(a, call):
    with mock.patch.object(ops, "attr_in_slot_order", lambda csr, ea: (a["ea_sorted"], a["identity"])):
        return call()


def _atomic(call):
    with mock.patch.object(ops, "DX_MODE", "atomic"):
        return call()


def forms():
    F = []

    def add(fid, wrapper, call, script=None):
        F.append((fid, wrapper, call, script))

    fr, fn, fh, fm = ops.nnconv_forward_raw, ops.nnconv_forward_nodeattr_raw, ops.nnconv_forward_hidden_raw, ops.nnconv_forward_mixed_raw
    hf, br, bl = ops.hidden_forward_raw, ops.nnconv_backward_raw, ops.nnconv_backward_light_raw
    bd, bh, hb = ops.nnconv_backward_deferred_raw, ops.nnconv_backward_hidden_raw, ops.hidden_backward_raw
    ew, fg, fe = ops.edge_weights_raw, ops.nnconv_forward_edgeweights_group, ops.nnconv_forward_edgeweights_raw
    be, eb = ops.nnconv_backward_edgeweights_raw, ops.edge_weights_backward_raw
    big = lambda: graph(max_in_degree=ops.EDGE_PATH_MAX_IN_DEGREE + 1)
    e3 = lambda a: int(a["csr"].rowptr[3])

    # ---- nnconv_forward_raw
    w = "nnconv_forward_raw"
    add("fwd.plain", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean"))
    add("fwd.add", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "add"))
    add("fwd.f32", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", precision="f32"))
    add("fwd.f16split", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", precision="f16split"))
    add("fwd.high_in_degree", w, lambda a: fr(a["x"], _with(a, csr=big())["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean"))
    add("fwd.high_in_degree_named", w, lambda a: fr(a["x"], _with(a, csr=big())["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean",
                                                   precision="f16split"))
    add("fwd.residual", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", residual=a["residual"]))
    add("fwd.relu", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", relu=True))
    add("fwd.residual_relu", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", residual=a["residual"],
                                            relu=True))
    add("fwd.z_keep", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", z_keep=a["z"]))
    add("fwd.nodeattr", w, lambda a: fr(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], "mean"))
    add("fwd.nodeattr_z_keep", w, lambda a: fr(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], "mean", z_keep=a["z"],
                                              precision="f32"))
    add("fwd.no_root", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], None, a["bias"], "mean"))
    add("fwd.no_bias", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], None, "mean"))
    add("fwd.out_ws", w, lambda a: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", out=a["out"], ws=a["ws"]))
    add("fwd.slot_order", w, lambda a: _slot_order_patched(a, lambda: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean")))

    # ---- nnconv_forward_nodeattr_raw
    w = "nnconv_forward_nodeattr_raw"
    add("fwd_na.plain", w, lambda a: fn(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], "mean"))
    add("fwd_na.bench", w, lambda a: fn(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], "mean", out=a["out"], ws=a["ws"],
                                       precision="f16split"))
    add("fwd_na.no_root_bias", w, lambda a: fn(a["x"], a["csr"], a["na"], a["pm"], None, None, "add", precision="f32"))

    # ---- nnconv_forward_hidden_raw
    w = "nnconv_forward_hidden_raw"
    add("fwd_h.plain", w, lambda a: fh(a["x"], a["csr"], a["hidden"], a["pm"], a["root"], a["bias"], "mean"))
    add("fwd_h.hmax", w, lambda a: fh(a["x"], a["csr"], a["hidden"], a["pm"], a["root"], a["bias"], "mean", hmax=a["hmax"]))
    add("fwd_h.residual_relu", w, lambda a: fh(a["x"], a["csr"], a["hidden"], a["pm"], a["root"], a["bias"], "mean",
                                              residual=a["residual"], relu=True))
    add("fwd_h.z_keep_hmax", w, lambda a: fh(a["x"], a["csr"], a["hidden"], a["pm"], a["root"], a["bias"], "mean", hmax=a["hmax"],
                                            z_keep=a["z"]))
    add("fwd_h.out_ws", w, lambda a: fh(a["x"], a["csr"], a["hidden"], a["pm"], None, None, "add", out=a["out"], ws=a["ws"]))

    # ---- nnconv_forward_mixed_raw
    w = "nnconv_forward_mixed_raw"
    add("fwd_m.tensor", w, lambda a: fm(a["x"], a["csr"], a["ea"], None, None, 0, a["pm"], a["root"], a["bias"], "mean"))
    add("fwd_m.partial", w, lambda a: fm(a["x"], a["csr"], a["ea"], _with(a, part=a["hidden"][:e3(a)].clone())["part"], a["hmax"], 3,
                                        a["pm"], a["root"], a["bias"], "mean"))
    add("fwd_m.hidden_given_nodes_0", w, lambda a: fm(a["x"], a["csr"], a["ea"], a["hidden"], a["hmax"], 0, a["pm"], a["root"], a["bias"],
                                                     "mean", precision="f32"))
    add("fwd_m.nodeattr_partial", w, lambda a: fm(a["x"], a["csr"], a["na"], _with(a, part=a["hidden"][:e3(a)].clone())["part"], None, 3,
                                                 a["pm"], a["root"], a["bias"], "mean"))
    add("fwd_m.z_keep", w, lambda a: fm(a["x"], a["csr"], a["ea"], None, None, 0, a["pm"], a["root"], a["bias"], "mean", z_keep=a["z"]))
    add("fwd_m.out_ws", w, lambda a: fm(a["x"], a["csr"], a["ea"], None, None, 0, a["pm"], None, None, "add", out=a["out"], ws=a["ws"]))
    add("fwd_m.slot_order", w, lambda a: _slot_order_patched(a, lambda: fm(a["x"], a["csr"], a["ea"], None, None, 0, a["pm"], a["root"],
                                                                          a["bias"], "mean")))

    # ---- hidden_forward_raw
    w = "hidden_forward_raw"
    add("hid.tensor", w, lambda a: hf(a["csr"], a["ea"], a["pm"], a["w"], a["b"]))
    add("hid.nodeattr", w, lambda a: hf(a["csr"], a["na"], a["pm"], a["w"], a["b"]))
    add("hid.tensor_limit", w, lambda a: hf(a["csr"], a["ea"], a["pm"], a["w"], a["b"], n_nodes_limit=3))
    add("hid.nodeattr_limit", w, lambda a: hf(a["csr"], a["na"], a["pm"], a["w"], a["b"], n_nodes_limit=3))
    add("hid.f32", w, lambda a: hf(a["csr"], a["ea"], a["pm"], a["w"], a["b"], precision="f32"))
    add("hid.last_entries_none", w, lambda a: hf(a["csr"], a["ea"], a["pm"], a["w"][:-1] + [None], a["b"][:-1] + [None], "f32"))
    add("hid.retry", w, lambda a: hf(a["csr"], a["ea"], a["pm"], a["w"], a["b"]), {"gpde_hidden_fwd": [-3, 0]})
    add("hid.retry_unsupported", w, lambda a: hf(a["csr"], a["ea"], a["pm"], a["w"], a["b"]), {"gpde_hidden_fwd": [-1, 0]})

    # ---- nnconv_backward_raw
    w = "nnconv_backward_raw"
    add("bwd.tensor", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"]))
    add("bwd.nodeattr", w, lambda a: br(a["x"], a["csr"], a["na"], a["w"], a["b"], a["root"], "mean", a["g"]))
    add("bwd.need_attr", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"], need_attr=True))
    add("bwd.z_saved", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"], z_saved=a["z"]))
    add("bwd.hidden_saved", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"], hidden_saved=a["hidden"]))
    add("bwd.no_need_root", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"], need_root=False))
    add("bwd.no_need_bias", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"], need_bias=False))
    add("bwd.root_none", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], None, "add", a["g"]))
    add("bwd.bias_entry_none", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], [a["b"][0], None, a["b"][2]], a["root"], "mean", a["g"]))
    add("bwd.ws", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"], ws=a["ws"]))
    add("bwd.atomic", w, lambda a: _atomic(lambda: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"])))
    add("bwd.slot_order", w, lambda a: _slot_order_patched(a, lambda: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"])))
    add("bwd.need_attr_slot_order", w, lambda a: _slot_order_patched(a, lambda: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean",
                                                                                  a["g"], need_attr=True)))

    def no_nodes(a):
        z32 = torch.zeros(0, dtype=torch.int32)
        csr = ops.Csr(0, 0, torch.zeros(1, dtype=torch.int32), z32, z32.clone(), z32.clone(), _max_in_degree=0)
        return br(torch.zeros(0, W), csr, torch.zeros(0, K0), a["w"], a["b"], a["root"], "mean", torch.zeros(0, W))
    add("bwd.no_nodes", w, no_nodes)

    # ---- nnconv_backward_light_raw
    w = "nnconv_backward_light_raw"
    add("light.tensor", w, lambda a: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"]))
    add("light.nodeattr", w, lambda a: bl(a["x"], a["csr"], a["na"], a["w"], a["b"], a["root"], "mean", a["g"]))
    add("light.z_saved", w, lambda a: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"], z_saved=a["z"]))
    add("light.hidden_part", w, lambda a: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"],
                                            hidden_part=_with(a, part=a["hidden"][:e3(a)].clone())["part"], hidden_nodes=3))
    add("light.hidden_part_nodes_0", w, lambda a: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"],
                                                    hidden_part=a["hidden"], hidden_nodes=0))
    add("light.no_root_no_bias", w, lambda a: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"][:-1] + [None], None, "add", a["g"],
                                                need_root=False, need_bias=False))
    add("light.atomic", w, lambda a: _atomic(lambda: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"])))

    # ---- nnconv_backward_deferred_raw
    w = "nnconv_backward_deferred_raw"
    add("defer.L1", w, lambda a: bd([a["x"]], [a["g"]], a["csr"], a["ea"], a["w"], a["b"], "mean"))
    add("defer.L3", w, lambda a: bd([a["x"], a["x1"], a["x2"]], [a["g"], a["g1"], a["g2"]], a["csr"], a["ea"], a["w"], a["b"], "mean"))
    add("defer.L5", w, lambda a: bd([a["x"], a["x1"], a["x2"], a["x"], a["x1"]], [a["g"], a["g1"], a["g2"], a["g"], a["g1"]], a["csr"], a["ea"],
                                   a["w"], a["b"], "add"))
    add("defer.nodeattr", w, lambda a: bd([a["x"], a["x1"]], [a["g"], a["g1"]], a["csr"], a["na"], a["w"], a["b"], "mean"))
    add("defer.hidden_part", w, lambda a: bd([a["x"], a["x1"]], [a["g"], a["g1"]], a["csr"], a["ea"], a["w"], a["b"], "mean",
                                            hidden_part=_with(a, part=a["hidden"][:e3(a)].clone())["part"], hidden_nodes=3))
    add("defer.bias_entry_none", w, lambda a: bd([a["x"]], [a["g"]], a["csr"], a["ea"], a["w"], [None, a["b"][1], a["b"][2]], "mean"))

    # ---- nnconv_backward_hidden_raw
    w = "nnconv_backward_hidden_raw"
    add("bwd_h.plain", w, lambda a: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], a["b"][2], a["root"], "mean", a["g"]))
    add("bwd_h.accumulate", w, lambda a: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], a["b"][2], a["root"], "mean", a["g"],
                                           grad_hidden_acc=a["acc"]))
    add("bwd_h.b_last_none", w, lambda a: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], None, a["root"], "mean", a["g"]))
    add("bwd_h.z_saved", w, lambda a: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], a["b"][2], a["root"], "mean", a["g"], z_saved=a["z"]))
    add("bwd_h.no_root_no_bias", w, lambda a: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], a["b"][2], None, "add", a["g"],
                                                need_bias=False))
    add("bwd_h.atomic", w, lambda a: _atomic(lambda: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], a["b"][2], a["root"], "mean", a["g"])))

    # ---- hidden_backward_raw
    w = "hidden_backward_raw"
    add("hid_b.tensor", w, lambda a: hb(a["csr"], a["ea"], DIMS, a["w"][:-1], a["b"][:-1], a["gh"]))
    add("hid_b.nodeattr", w, lambda a: hb(a["csr"], a["na"], DIMS, a["w"][:-1], a["b"][:-1], a["gh"]))
    add("hid_b.bias_entry_none", w, lambda a: hb(a["csr"], a["ea"], DIMS, a["w"][:-1], [a["b"][0], None], a["gh"]))
    add("hid_b.slot_order", w, lambda a: _slot_order_patched(a, lambda: hb(a["csr"], a["ea"], DIMS, a["w"][:-1], a["b"][:-1], a["gh"])))

    # ---- edge_weights_raw
    w = "edge_weights_raw"
    add("we.plain", w, lambda a: ew(a["hidden"], a["pm"], a["w"][2], a["b"][2]))
    add("we.b_last_none", w, lambda a: ew(a["hidden"], a["pm"], a["w"][2], None))

    # ---- nnconv_forward_edgeweights_group / nnconv_forward_edgeweights_raw
    w = "nnconv_forward_edgeweights_group"
    add("we_group.two_calls", w, lambda a: fg([
        dict(x=a["x"], csr=a["csr"], edge_weights=a["we"], root=a["root"], bias=a["bias"], aggr="mean", residual=a["residual"], relu=True),
        dict(x=a["x1"], csr=a["csr2"], edge_weights=a["we2"], root=None, bias=None, aggr="max", out=a["out"])]))
    w = "nnconv_forward_edgeweights_raw"
    add("we_fwd.plain", w, lambda a: fe(a["x"], a["csr"], a["we"], a["root"], a["bias"], "mean"))
    add("we_fwd.glue_out", w, lambda a: fe(a["x"], a["csr"], a["we"], None, a["bias"], "add", residual=a["residual"], relu=True, out=a["out"]))

    # ---- nnconv_backward_edgeweights_raw
    w = "nnconv_backward_edgeweights_raw"
    add("we_bwd.plain", w, lambda a: be(a["x"], a["csr"], a["we"], a["root"], "mean", a["g"]))
    add("we_bwd.acc", w, lambda a: be(a["x"], a["csr"], a["we"], a["root"], "mean", a["g"], acc=tuple(a["acc_we"])))
    add("we_bwd.root_none", w, lambda a: be(a["x"], a["csr"], a["we"], None, "add", a["g"]))
    add("we_bwd.no_need_bias", w, lambda a: be(a["x"], a["csr"], a["we"], a["root"], "mean", a["g"], need_bias=False))

    # ---- edge_weights_backward_raw
    w = "edge_weights_backward_raw"
    add("we_b.plain", w, lambda a: eb(a["gwe"], a["hidden"], DIMS, a["w"][2]))
    add("we_b.no_need_b", w, lambda a: eb(a["gwe"], a["hidden"], DIMS, a["w"][2], need_b=False))

    # ---- single-fault refusals
    fwd_calls = {
        "nnconv_forward_raw": lambda a, **k: fr(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], k.pop("aggr", "mean"), **k),
        "nnconv_forward_nodeattr_raw": lambda a, **k: fn(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], k.pop("aggr", "mean"), **k),
        "nnconv_forward_hidden_raw": lambda a, **k: fh(a["x"], a["csr"], a["hidden"], a["pm"], a["root"], a["bias"], k.pop("aggr", "mean"), **k),
        "nnconv_forward_mixed_raw": lambda a, **k: fm(a["x"], a["csr"], a["ea"], None, None, 0, a["pm"], a["root"], a["bias"],
                                                      k.pop("aggr", "mean"), **k),
    }
    for w, call in fwd_calls.items():
        add(f"refuse.{w}.x_float64", w, lambda a, call=call: call(_with(a, x=a["x"].double())))
        add(f"refuse.{w}.x_63_columns", w, lambda a, call=call: call(_with(a, x=torch.zeros(N, W - 1))))
        add(f"refuse.{w}.x_rows", w, lambda a, call=call: call(_with(a, x=torch.zeros(N + 1, W))))
        add(f"refuse.{w}.aggr_max", w, lambda a, call=call: call(a, aggr="max"))
        if w != "nnconv_forward_hidden_raw":
            add(f"refuse.{w}.precision", w, lambda a, call=call: call(a, precision="f8"))
    w, c_fr, c_fn, c_fh = "nnconv_forward_raw", fwd_calls["nnconv_forward_raw"], fwd_calls["nnconv_forward_nodeattr_raw"], \
        fwd_calls["nnconv_forward_hidden_raw"]
    add("refuse.fwd.edge_attr_columns", w, lambda a: c_fr(_with(a, ea=torch.zeros(E, K0 + 1))))
    add("refuse.fwd.edge_attr_float64", w, lambda a: c_fr(_with(a, ea=a["ea"].double())))
    add("refuse.fwd.z_keep_relu", w, lambda a: c_fr(a, z_keep=a["z"], relu=True))
    add("refuse.fwd.z_keep_residual", w, lambda a: c_fr(a, z_keep=a["z"], residual=a["residual"]))
    add("refuse.fwd.nodeattr_residual", w, lambda a: fr(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], "mean", residual=a["residual"]))
    add("refuse.fwd.nodeattr_relu", w, lambda a: fr(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], "mean", relu=True))
    add("refuse.fwd.residual_shape", w, lambda a: c_fr(a, residual=torch.zeros(N + 1, W)))
    add("refuse.fwd.z_keep_shape", w, lambda a: c_fr(a, z_keep=torch.zeros(N, W * K2P + 1)))
    w = "nnconv_forward_hidden_raw"
    add("refuse.fwd_h.z_keep_relu", w, lambda a: c_fh(a, z_keep=a["z"], relu=True))
    add("refuse.fwd_h.hidden_shape", w, lambda a: c_fh(_with(a, hidden=torch.zeros(E + 1, K2P))))
    bad_table = lambda a: _with(a, na=ops.NodeAttr(torch.zeros(N + 1, K0), [(0, 0), (1, 1), (0, 2)]))
    bad_slots = lambda a: _with(a, na=ops.NodeAttr(torch.zeros(N, K0), [(0, 0), (1, 1)]))
    w = "nnconv_forward_nodeattr_raw"
    add("refuse.fwd_na.table_rows", w, lambda a: c_fn(bad_table(a)))
    add("refuse.fwd_na.table_slots", w, lambda a: c_fn(bad_slots(a)))
    w = "nnconv_forward_mixed_raw"
    add("refuse.fwd_m.table_rows", w, lambda a: fm(a["x"], a["csr"], bad_table(a)["na"], None, None, 0, a["pm"], a["root"], a["bias"], "mean"))
    add("refuse.fwd_m.hidden_shape", w, lambda a: fm(a["x"], a["csr"], a["ea"], a["hidden"], a["hmax"], 3, a["pm"], a["root"], a["bias"], "mean"))
    add("refuse.fwd.table_rows", "nnconv_forward_raw",
        lambda a: fr(a["x"], a["csr"], bad_table(a)["na"], a["pm"], a["root"], a["bias"], "mean"))
    w = "hidden_forward_raw"
    add("refuse.hid.precision", w, lambda a: hf(a["csr"], a["ea"], a["pm"], a["w"], a["b"], precision="f8"))
    add("refuse.hid.edge_attr_columns", w, lambda a: hf(a["csr"], torch.zeros(E, K0 + 1), a["pm"], a["w"], a["b"]))
    w = "nnconv_backward_raw"
    add("refuse.bwd.aggr_max", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "max", a["g"]))
    add("refuse.bwd.hidden_saved_shape", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"],
                                                        hidden_saved=torch.zeros(E + 1, K2P)))
    add("refuse.bwd.hidden_saved_need_attr", w, lambda a: br(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"],
                                                            hidden_saved=a["hidden"], need_attr=True))
    add("refuse.bwd.need_attr_nodeattr", w, lambda a: br(a["x"], a["csr"], a["na"], a["w"], a["b"], a["root"], "mean", a["g"], need_attr=True))
    add("refuse.bwd.x_rows", w, lambda a: br(torch.zeros(N + 1, W), a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"]))
    add("refuse.bwd.weight_shape", w, lambda a: br(a["x"], a["csr"], a["ea"], [a["w"][0], torch.zeros(K2, 17), a["w"][2]], a["b"], a["root"],
                                                  "mean", a["g"]))
    w = "nnconv_backward_light_raw"
    add("refuse.light.aggr_max", w, lambda a: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "max", a["g"]))
    add("refuse.light.z_saved_shape", w, lambda a: bl(a["x"], a["csr"], a["ea"], a["w"], a["b"], a["root"], "mean", a["g"],
                                                     z_saved=torch.zeros(N, W)))
    w = "nnconv_backward_deferred_raw"
    add("refuse.defer.pairs", w, lambda a: bd([a["x"], a["x1"]], [a["g"]], a["csr"], a["ea"], a["w"], a["b"], "mean"))
    add("refuse.defer.no_pairs", w, lambda a: bd([], [], a["csr"], a["ea"], a["w"], a["b"], "mean"))
    add("refuse.defer.aggr_max", w, lambda a: bd([a["x"]], [a["g"]], a["csr"], a["ea"], a["w"], a["b"], "max"))
    add("refuse.defer.gs_shape", w, lambda a: bd([a["x"]], [torch.zeros(N, W + 1)], a["csr"], a["ea"], a["w"], a["b"], "mean"))
    w = "nnconv_backward_hidden_raw"
    add("refuse.bwd_h.aggr_max", w, lambda a: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], a["b"][2], a["root"], "max", a["g"]))
    add("refuse.bwd_h.acc_shape", w, lambda a: bh(a["x"], a["csr"], a["hidden"], DIMS, a["w"][2], a["b"][2], a["root"], "mean", a["g"],
                                                 grad_hidden_acc=torch.zeros(E, K2P + 1)))
    w = "hidden_backward_raw"
    add("refuse.hid_b.weight_count", w, lambda a: hb(a["csr"], a["ea"], DIMS, a["w"], a["b"], a["gh"]))
    add("refuse.hid_b.grad_hidden_shape", w, lambda a: hb(a["csr"], a["ea"], DIMS, a["w"][:-1], a["b"][:-1], torch.zeros(E, K2P + 1)))
    add("refuse.we.w_last_shape", "edge_weights_raw", lambda a: ew(a["hidden"], a["pm"], torch.zeros(W * W, K2 + 1), a["b"][2]))
    add("refuse.we_group.devices", "nnconv_forward_edgeweights_group", lambda a: fg([
        dict(x=a["x"], csr=a["csr"], edge_weights=a["we"], root=a["root"], bias=a["bias"]),
        dict(x=a["x1"].to("meta"), csr=a["csr2"], edge_weights=a["we2"], root=None, bias=None)]))
    add("refuse.we_fwd.aggr", "nnconv_forward_edgeweights_raw", lambda a: fe(a["x"], a["csr"], a["we"], a["root"], a["bias"], "min"))
    add("refuse.we_bwd.aggr_max", "nnconv_backward_edgeweights_raw", lambda a: be(a["x"], a["csr"], a["we"], a["root"], "max", a["g"]))
    add("refuse.we_b.grad_shape", "edge_weights_backward_raw", lambda a: eb(torch.zeros(E + 1, W * W), a["hidden"], DIMS, a["w"][2]))
    assert len({f[0] for f in F}) == len(F), "form ids are unique"
    return F


def record_all():
    return {f[0]: record(f) for f in forms()}


# every (wrapper, entry point) pair the table must reach (tests/test_native_calls_host.py asserts the set)
PAIRS = {
    ("nnconv_forward_raw", "gpde_nnconv_fwd"), ("nnconv_forward_raw", "gpde_nnconv_fwd_act"), ("nnconv_forward_raw", "gpde_nnconv_fwd_keepz"),
    ("nnconv_forward_raw", "gpde_nnconv_fwd_mixed_keepz"),
    ("nnconv_forward_nodeattr_raw", "gpde_nnconv_fwd_mixed_keepz"),
    ("nnconv_forward_hidden_raw", "gpde_nnconv_fwd_hidden_act"), ("nnconv_forward_hidden_raw", "gpde_nnconv_fwd_keepz"),
    ("nnconv_forward_mixed_raw", "gpde_nnconv_fwd_mixed_keepz"),
    ("hidden_forward_raw", "gpde_hidden_fwd"),
    ("nnconv_backward_raw", "gpde_nnconv_bwd"), ("nnconv_backward_light_raw", "gpde_nnconv_bwd_light"),
    ("nnconv_backward_deferred_raw", "gpde_nnconv_bwd_deferred"), ("nnconv_backward_hidden_raw", "gpde_nnconv_bwd"),
    ("hidden_backward_raw", "gpde_hidden_bwd"),
    ("edge_weights_raw", "gpde_edge_weights_fwd"), ("nnconv_forward_edgeweights_group", "gpde_nnconv_fwd_edgeweights_group"),
    ("nnconv_forward_edgeweights_raw", "gpde_nnconv_fwd_edgeweights_group"),
    ("nnconv_backward_edgeweights_raw", "gpde_nnconv_bwd_edgeweights_acc"), ("edge_weights_backward_raw", "gpde_edge_weights_bwd"),
}
