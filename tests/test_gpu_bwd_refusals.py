"""GPU tier: the refusals of the native backward's own orchestration (bwd_impl: BwdCall::setup, next_chunk and the per-edge
kernel choice, csrc/gpde_bwd.hip) on graphs of 8 nodes and 16 edges.  Each is a host-side error return - the return code and the
gpde_last_error() text are asserted, and the device is synchronised afterwards: what the call launched before it refused ran
to its end.  ops.py refuses a k0 > 8 attribute gradient itself, so that case calls the entry point the way tests/test_abi.py
does."""
import pytest
import torch

from graph_pde_amd import _lib, ops
from tests.helpers.bwd_walk import ws_for

pytestmark = pytest.mark.gpu
N, E = 8, 16
EUNSUPPORTED, EWORKSPACE = -2, -3
DEPTH_FORM = ("kernel MLP outside the depth-deferred form (3 Linear layers of widths that are multiples of 128, k0 <= 7): "
              "use gpde_nnconv_bwd")


def _case(dims, n=N, dst=None, seed=0):
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    if dst is None:
        dst = torch.randint(0, n, (E,), generator=g)
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    csr = ops.build_csr(torch.stack([src, dst]).to(d), n)
    W = [(torch.empty(dims[i + 1], dims[i]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5).to(d) for i in range(len(dims) - 1)]
    B = [(torch.empty(dims[i + 1]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5).to(d) for i in range(len(dims) - 1)]
    x, gout = torch.randn(n, 64, generator=g).to(d), torch.randn(n, 64, generator=g).to(d)
    return d, csr, W, B, x, gout, torch.randn(dst.numel(), dims[0], generator=g).to(d)


def _refused(code, text, call):
    """`call` fails with the library's `code` (_lib.check: NotImplementedError for GPDE_EUNSUPPORTED, else GpdeError naming the
    code) and `text` is what gpde_last_error() holds."""
    with pytest.raises(NotImplementedError if code == EUNSUPPORTED else _lib.GpdeError) as ei:
        call()
    torch.cuda.synchronize()
    last = _lib.lib().gpde_last_error().decode()
    assert text in last, last
    assert last in str(ei.value), (last, str(ei.value))
    if code != EUNSUPPORTED:
        assert f"(code {code})" in str(ei.value), str(ei.value)


def test_light_and_deferred_refuse_a_kernel_mlp_outside_the_depth_deferred_form():
    # deferred: k2 = 64 pads to 128, below the split-f16 backward GEMMs; light: two Linear layers have no fused store kernel
    d, csr, W, B, x, gout, ea = _case([3, 64, 64, 4096])
    _refused(EUNSUPPORTED, "gpde_nnconv_bwd_deferred: " + DEPTH_FORM,
             lambda: ops.nnconv_backward_deferred_raw([x, x], [gout, gout], csr, ea, W, B, "add"))
    d, csr, W, B, x, gout, ea = _case([3, 64, 4096])
    _refused(EUNSUPPORTED, "gpde_nnconv_bwd_light: " + DEPTH_FORM,
             lambda: ops.nnconv_backward_light_raw(x, csr, ea, W, B, None, "mean", gout))


def test_node_table_attributes_refuse_a_kernel_mlp_that_is_not_3_linear():
    d, csr, W, B, x, gout, _ = _case([3, 64, 4096])
    table = torch.randn(N, 2, device=d)
    na = ops.NodeAttr(table, [(0, 0), (1, 0), (0, 1)])
    _refused(EUNSUPPORTED, "gpde_nnconv_bwd: node-table attributes need the 3-Linear split-f16 form (and src / dst)",
             lambda: ops.nnconv_backward_raw(x, csr, na, W, B, None, "add", gout))


def test_grad_edge_attr_refuses_more_than_8_slots():
    dims = [9, 64, 64, 4096]
    d, csr, W, B, x, gout, ea = _case(dims)
    lib = _lib.lib()
    _, dims_c, ws_, bs_ = ops._mlp_operands(W, B, d)
    gx, ga = torch.empty(N, 64, device=d), torch.zeros(E, dims[0], device=d)
    gW, gb = [torch.empty_like(w) for w in ws_], [torch.empty_like(b) for b in bs_]
    ws = torch.empty(int(lib.gpde_nnconv_bwd_workspace_bytes(N, E, 3, dims_c)), dtype=torch.uint8, device=d)
    srp, ssl = csr.src_order

    def call():       # the attribute rows in the caller's order with the CSR's own perm, as ops.nnconv_backward_raw(need_attr=True)
        rc = lib.gpde_nnconv_bwd(x.data_ptr(), N, ea.data_ptr(), None, None, E, csr.rowptr.data_ptr(), csr.src.data_ptr(),
                                 csr.dst.data_ptr(), csr.perm.data_ptr(), csr.rowptr_host.data_ptr(), ops._ptr(srp), ops._ptr(ssl), 3,
                                 dims_c, ops._ptr_array(ws_), ops._ptr_array(bs_), None, 0, gout.data_ptr(), None, gx.data_ptr(), None,
                                 ga.data_ptr(), ops._ptr_array(gW), ops._ptr_array(gb), None, None, 0, ws.data_ptr(), ws.numel(),
                                 ops._stream_ptr(d))
        assert rc == EUNSUPPORTED, rc
        _lib.check(rc, "gpde_nnconv_bwd")
    _refused(EUNSUPPORTED, "gpde_nnconv_bwd: the edge-attribute gradient is built for the full backward on an attribute tensor of <= 8 slots",
             call)


def test_a_node_with_more_in_edges_than_a_chunk_holds_is_named():
    dims = [6, 256, 256, 4096]
    heavy, deg = 3, 600
    dst = torch.cat([torch.arange(N).repeat(2), torch.full((deg,), heavy)])          # 2 in-edges per node, 600 more into node 3
    d, csr, W, B, x, gout, ea = _case(dims, dst=dst)
    e = dst.numel()
    ws_bytes = ws_for(N, e, dims, 200)
    ec = ops.bwd_plan(N, e, dims, ws_bytes)["edges_per_chunk"]
    assert 200 <= ec < deg, ec
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d)
    _refused(EWORKSPACE, f"gpde_nnconv_bwd: node {heavy} has in-degree {deg + 2} > {ec} edges per chunk; give more workspace",
             lambda: ops.nnconv_backward_raw(x, csr, ea, W, B, None, "mean", gout, ws=ws))


def test_accumulating_grad_hidden_refuses_the_forced_fp32_staged_kernel(monkeypatch):
    dims = [3, 64, 64, 4096]
    d, csr, W, B, x, gout, _ = _case(dims)
    H = torch.rand(E, ops.hidden_width(dims), device=d)
    monkeypatch.setenv("GPDE_EDGE_BWD", "2")
    _refused(EUNSUPPORTED, "gpde_nnconv_bwd: GPDE_BWD_ACCUMULATE_GRAD_HIDDEN is built into the split-f16 per-edge kernel only "
             "(GPDE_EDGE_BWD=2 forces the other one)",
             lambda: ops.nnconv_backward_hidden_raw(x, csr, H, dims, W[-1], B[-1], None, "add", gout, grad_hidden_acc=torch.zeros_like(H)))
