"""Host tier of the operand-layout contract (DESIGN.md "Operand layouts"): ops._operand on CPU tensors, and a table over every
wrapper of ops.py that takes a caller-written tensor (`out`, `z_keep`, `acc`): an awkward one is refused BEFORE any call into
libgpde.so - the library is replaced by an object whose every attribute raises.  No GPU."""
import contextlib
import inspect

import pytest
import torch

from graph_pde_amd import _lib, ops
from tests.helpers import layouts
from tests.helpers.layouts import AWKWARD, KINDS, all_sentinel, as_layout, guards_intact

CPU = torch.device("cpu")


def _value(kind, shape):
    g = torch.Generator().manual_seed(len(kind) + sum(shape))
    if kind == "expanded":
        return torch.full(shape, 0.375)
    return torch.randn(*shape, generator=g)


def _kinds_for(shape):
    return [k for k in KINDS if not (k == "transposed_storage" and len(shape) != 2)]


@pytest.mark.parametrize("shape", [(7, 64), (5, 3), (64,), (1, 1)])
def test_read_only_operand_comes_back_dense_aligned_and_equal(shape):
    for kind in _kinds_for(shape):
        t = _value(kind, shape)
        view, backing = as_layout(t, kind)
        got = ops._operand(view, "x", shape, CPU)
        assert got.is_contiguous() and got.data_ptr() % 16 == 0, kind
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(shape), kind
        assert torch.equal(got.view(torch.int32), t.contiguous().view(torch.int32)), kind
        guards_intact(backing)
        if kind == "dense":
            assert got is view                                  # no copy, no new object: the caches key on data_ptr
        elif view.is_contiguous() and view.data_ptr() % 16 == 0:
            assert got is view, kind                            # (a [1, 1] view of any stride is dense)
        else:
            assert got.data_ptr() != view.data_ptr(), kind


def test_layout_kinds_are_what_they_say():
    t = torch.randn(6, 8)
    v, _ = as_layout(t, "row_strided")
    assert v.stride() == (11, 1) and not v.is_contiguous()
    v, _ = as_layout(t, "row_skipping")
    assert v.stride() == (16, 1) and not v.is_contiguous()
    v, _ = as_layout(t, "transposed_storage")
    assert v.stride() == (1, 6)
    for kind, rem in (("offset4", 4), ("offset8", 8)):
        v, b = as_layout(t, kind)
        assert v.is_contiguous() and v.data_ptr() % 16 == rem
        assert all_sentinel(b.buf[~b.mask]) and int((~b.mask).sum()) >= 16
    v, _ = as_layout(torch.full((6, 8), 2.0), "expanded")
    assert v.stride() == (0, 0)
    v, b = as_layout(t, "row_strided")
    b.buf[0, 8] = 0.0                                           # a stray 0.0 in a guard column is seen
    with pytest.raises(AssertionError, match="guard"):
        guards_intact(b)


def test_none_passes_and_dense_requires_grad_keeps_identity():
    assert ops._operand(None, "root", (64, 64), CPU) is None
    p = torch.nn.Parameter(torch.randn(64, 64))
    assert ops._operand(p, "root", (64, 64), CPU) is p
    v, _ = as_layout(p.detach(), "offset4")
    v.requires_grad_(True)
    got = ops._operand(v, "root", (64, 64), CPU)
    assert not got.requires_grad and torch.equal(got, p.detach())


def test_node_table_that_wants_a_gradient_stays_in_the_graph():
    """ops.NodeAttr makes its table dense and aligned; a table that requires grad (a column slice of a learned parameter, a
    parameter re-pointed into a flat buffer) is copied DIFFERENTIABLY: the module materialises the gather from `.table`."""
    sel = [(0, 0), (1, 1)]
    p = torch.nn.Parameter(torch.randn(6, 5))
    assert ops.NodeAttr(p, sel).table is p                      # dense and aligned: the tensor itself
    for view in (p[:, :3], p[::2], p.t()[:5, :4]):
        assert view.requires_grad and not view.is_contiguous()
        na = ops.NodeAttr(view, sel)
        assert na.table.requires_grad and na.table.is_contiguous() and na.table.data_ptr() % 16 == 0
        na.materialize(torch.tensor([[0, 1, 2], [2, 1, 0]])).sum().backward()
        assert p.grad is not None and float(p.grad.abs().sum()) > 0
        p.grad = None
    off, _ = as_layout(torch.randn(6, 3), "offset4")
    off.requires_grad_(True)
    na = ops.NodeAttr(off, sel)
    assert na.table.requires_grad and na.table.data_ptr() % 16 == 0
    na.materialize(torch.tensor([[0, 1], [1, 0]])).sum().backward()
    assert off.grad is not None and float(off.grad.abs().sum()) > 0
    with torch.no_grad():                                       # no graph is being built: a plain dense copy
        assert not ops.NodeAttr(p[:, :3], sel).table.requires_grad
    v, b = as_layout(torch.randn(6, 3), "row_strided")
    assert not ops.NodeAttr(v, sel).table.requires_grad
    guards_intact(b)


@pytest.mark.parametrize("writable", [False, True])
def test_wrong_dtype_shape_device_raise_naming_the_operand(writable):
    good = torch.zeros(5, 64)
    for bad_dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
        with pytest.raises(ValueError, match="residual") as err:
            ops._operand(good.to(bad_dtype), "residual", (5, 64), CPU, writable=writable)
        assert str(bad_dtype).replace("torch.", "") in str(err.value)
    for bad_shape in ((4, 64), (5, 63), (5,), (5, 64, 1), (64, 5)):
        with pytest.raises(ValueError, match="residual"):
            ops._operand(torch.zeros(*bad_shape), "residual", (5, 64), CPU, writable=writable)
    with pytest.raises(ValueError, match="residual"):           # a tensor on another device than the call's
        ops._operand(good, "residual", (5, 64), torch.device("cuda", 0), writable=writable)
    with pytest.raises(ValueError, match="residual"):
        ops._operand(good, "residual", (5, 64), torch.device("meta"), writable=writable)
    with pytest.raises(NotImplementedError, match="x"):         # a wrapper keeps its own exception type
        ops._operand(good.double(), "x", (5, 64), CPU, exc=NotImplementedError)
    assert ops._operand(good, "ws", (None, 64), CPU, writable=writable) is good      # None: any extent
    with pytest.raises(ValueError, match="ws"):
        ops._operand(torch.zeros(8, dtype=torch.float32), "ws", (None,), CPU, dtype=torch.uint8, writable=writable)


@pytest.mark.parametrize("shape", [(7, 64), (64,)])
def test_written_operand_is_never_copied(shape):
    for kind in _kinds_for(shape):
        t = _value(kind, shape)
        view, backing = as_layout(t, kind)
        if kind == "dense":
            assert ops._operand(view, "out", shape, CPU, writable=True) is view
            continue
        with pytest.raises(ValueError, match="z_keep"):
            ops._operand(view, "z_keep", shape, CPU, writable=True)
        guards_intact(backing)
    out, backing = layouts.carve_out(shape, CPU)                # dense and aligned inside a larger buffer: accepted as it is
    assert ops._operand(out, "out", shape, CPU, writable=True) is out


# ---------------------------------------------------------------------------------------------------------------------------
# every wrapper that takes a caller-written tensor refuses an awkward one before the library is reached
# ---------------------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"reached the library ({name})")


N, E, K0, K2 = 6, 9, 3, 32
DIMS = (K0, 16, K2, 4096)
K2P = 128


def _graph():
    rowptr = torch.tensor([0, 2, 4, 5, 7, 9, 9], dtype=torch.int32)
    src = torch.arange(E, dtype=torch.int32) % N
    dst = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), (rowptr[1:] - rowptr[:-1]).long())
    return ops.Csr(N, E, rowptr, src, dst, torch.arange(E, dtype=torch.int32), _max_in_degree=2)


def _args():
    pm = ops.PackedMlp(DIMS, torch.zeros(4), _lib.dims_array(DIMS))
    return dict(x=torch.randn(N, 64), csr=_graph(), ea=torch.randn(E, K0), pm=pm, root=torch.randn(64, 64), bias=torch.randn(64),
                hidden=torch.randn(E, K2P), we=torch.randn(E, 4096), g=torch.randn(N, 64),
                na=ops.NodeAttr(torch.randn(N, K0), [(0, 0), (1, 1), (0, 2)]))


# wrapper -> {written parameter -> (its shape, the call with that parameter given)}
def _table():
    a = _args()
    z_shape = (N, 64 * K2P)
    return {
        "nnconv_forward_raw": {
            "out": ((N, 64), lambda t: ops.nnconv_forward_raw(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", out=t)),
            "z_keep": (z_shape, lambda t: ops.nnconv_forward_raw(a["x"], a["csr"], a["ea"], a["pm"], a["root"], a["bias"], "mean", z_keep=t)),
        },
        "nnconv_forward_nodeattr_raw": {
            "out": ((N, 64), lambda t: ops.nnconv_forward_nodeattr_raw(a["x"], a["csr"], a["na"], a["pm"], a["root"], a["bias"], "mean", out=t)),
        },
        "nnconv_forward_hidden_raw": {
            "out": ((N, 64), lambda t: ops.nnconv_forward_hidden_raw(a["x"], a["csr"], a["hidden"], a["pm"], a["root"], a["bias"], "mean", out=t)),
            "z_keep": (z_shape, lambda t: ops.nnconv_forward_hidden_raw(a["x"], a["csr"], a["hidden"], a["pm"], a["root"], a["bias"], "mean",
                                                                          z_keep=t)),
        },
        "nnconv_forward_mixed_raw": {
            "out": ((N, 64), lambda t: ops.nnconv_forward_mixed_raw(a["x"], a["csr"], a["ea"], None, None, 0, a["pm"], a["root"], a["bias"],
                                                                     "mean", out=t)),
            "z_keep": (z_shape, lambda t: ops.nnconv_forward_mixed_raw(a["x"], a["csr"], a["ea"], None, None, 0, a["pm"], a["root"], a["bias"],
                                                                        "mean", z_keep=t)),
        },
        "nnconv_forward_edgeweights_raw": {
            "out": ((N, 64), lambda t: ops.nnconv_forward_edgeweights_raw(a["x"], a["csr"], a["we"], a["root"], a["bias"], "mean", out=t)),
        },
        "nnconv_forward_edgeweights_group": {       # (takes `calls`: each descriptor's "out")
            "out": ((N, 64), lambda t: ops.nnconv_forward_edgeweights_group([
                dict(x=a["x"], csr=a["csr"], edge_weights=a["we"], root=a["root"], bias=a["bias"], aggr="add"),
                dict(x=a["x"], csr=a["csr"], edge_weights=a["we"], root=a["root"], bias=a["bias"], aggr="max", out=t)])),
        },
        "nnconv_backward_edgeweights_raw": {
            "acc[0]": ((E, 4096), lambda t: ops.nnconv_backward_edgeweights_raw(a["x"], a["csr"], a["we"], a["root"], "mean", a["g"],
                                                                                 acc=(t, torch.zeros(64, 64), torch.zeros(64)))),
            "acc[1]": ((64, 64), lambda t: ops.nnconv_backward_edgeweights_raw(a["x"], a["csr"], a["we"], a["root"], "mean", a["g"],
                                                                                acc=(torch.zeros(E, 4096), t, torch.zeros(64)))),
            "acc[2]": ((64,), lambda t: ops.nnconv_backward_edgeweights_raw(a["x"], a["csr"], a["we"], a["root"], "mean", a["g"],
                                                                             acc=(torch.zeros(E, 4096), torch.zeros(64, 64), t))),
        },
    }


WRITTEN = ("out", "z_keep", "acc")


def test_table_covers_every_wrapper_with_a_written_operand():
    """The table below is complete: every function of ops.py with a parameter named out / z_keep / acc has a row per such
    parameter (the group entry point takes them inside `calls` and has its own row)."""
    table = _table()
    for name, fn in inspect.getmembers(ops, inspect.isfunction):
        if fn.__module__ != ops.__name__ or name.startswith("_"):      # (public wrappers; `_out_ws` is the check itself)
            continue
        written = [p for p in inspect.signature(fn).parameters if p in WRITTEN]
        if written:
            assert name in table, f"ops.{name} takes {written}: add it to the table"
            have = {k.split("[")[0] for k in table[name]}
            assert have == set(written), (name, have, written)
    assert "nnconv_forward_edgeweights_group" in table


@pytest.mark.parametrize("wrapper", sorted(_table()))
def test_awkward_written_operand_is_refused_before_the_library(wrapper, monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    monkeypatch.setattr(ops, "_require_cuda", lambda t, name: None)       # CPU tensors stand in: the layout checks are host code
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    for param, (shape, call) in _table()[wrapper].items():
        for kind in ("row_strided", "row_skipping", "offset4", "offset8") + (("transposed_storage",) if len(shape) == 2 else ()):
            view, backing = as_layout(torch.zeros(shape), kind)
            with pytest.raises(ValueError, match=param.split("[")[0]) as err:
                call(view)
            assert "reached the library" not in str(err.value)
            guards_intact(backing)
        for bad in (torch.zeros(shape, dtype=torch.float64), torch.zeros((shape[0] + 1,) + tuple(shape[1:])),
                    torch.zeros(shape, device="meta")):
            with pytest.raises(ValueError, match=param.split("[")[0]):
                call(bad)
        # the control: a dense aligned tensor passes the host checks - the next thing the wrapper does is call the library
        with pytest.raises(AssertionError, match="reached the library"):
            call(torch.zeros(shape))


@pytest.mark.parametrize("operand", ["x", "root", "bias", "residual", "out"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16])
def test_wrong_dtype_never_reaches_the_library(operand, dtype, monkeypatch):
    """float64 / float16 / bfloat16 x, root, bias, residual, out on the forward wrappers: refused on the host (x with the
    exception type the wrapper has always used for it)."""
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    monkeypatch.setattr(ops, "_require_cuda", lambda t, name: None)
    a = _args()
    calls0 = _lib.n_native_calls

    def kw(**over):
        d = dict(x=a["x"], root=a["root"], bias=a["bias"], residual=torch.randn(N, 64), out=torch.zeros(N, 64))
        d.update(over)
        return d
    k = kw(**{operand: kw()[operand].to(dtype)})
    with pytest.raises(NotImplementedError if operand == "x" else ValueError, match="float32" if operand == "x" else operand):
        ops.nnconv_forward_raw(k["x"], a["csr"], a["ea"], a["pm"], k["root"], k["bias"], "mean", out=k["out"], residual=k["residual"])
    with pytest.raises(ValueError, match=operand):
        ops.nnconv_forward_hidden_raw(k["x"], a["csr"], a["hidden"], a["pm"], k["root"], k["bias"], "mean", out=k["out"],
                                      residual=k["residual"])
    with pytest.raises(ValueError, match=operand):
        ops.nnconv_forward_edgeweights_raw(k["x"], a["csr"], a["we"], k["root"], k["bias"], "mean", residual=k["residual"], out=k["out"])
    if operand != "residual":
        with pytest.raises(ValueError, match=operand):
            ops.nnconv_forward_mixed_raw(k["x"], a["csr"], a["ea"], None, None, 0, a["pm"], k["root"], k["bias"], "mean", out=k["out"])
        with pytest.raises(ValueError, match=operand):
            ops.nnconv_forward_nodeattr_raw(k["x"], a["csr"], a["na"], a["pm"], k["root"], k["bias"], "mean", out=k["out"])
    if operand in ("x", "root"):
        with pytest.raises(ValueError, match=operand):
            ops.nnconv_backward_edgeweights_raw(k["x"], a["csr"], a["we"], k["root"], "mean", a["g"])
    assert _lib.n_native_calls == calls0
