"""Host tier: where the forward's workspace and plan make room for the attribute operand image of
gpde_fused_f16v6_kernel (csrc/gpde_api.hip make_plan; no device work)."""
import ctypes
import os
import re
import types

from graph_pde_amd import _lib, ops

HEADLINE = (58081, 95539625, [6, 1024, 1024, 4096])


def _al(v):
    return (v + 255) // 256 * 256


def _image_bytes(e):
    return 256 + 2 * _al(16 * e) + _al(4 * e)           # constant record, hi plane, lo plane, isc


def _queue_bytes(e):
    """Block bounds of the kernel's work queue (3-Linear MLPs): the other part of the workspace that grows with the edges."""
    return _al((e // 4096 + e // 8 // 512 + 10 + 2 + 64) * 4)


def _ws(dims, n, e):
    return int(_lib.lib().gpde_nnconv_fwd_workspace_bytes(n, e, len(dims) - 1, _lib.dims_array(dims)))


def _pm(dims):
    return types.SimpleNamespace(dims=list(dims), dims_c=_lib.dims_array(dims))


def test_workspace_grows_by_the_image_exactly_where_the_forward_chooses_the_kernel():
    n, small = 1000, 32767
    for dims in ([6, 256, 256, 4096], [6, 1024, 1024, 4096], [7, 1152, 256, 4096], [1, 384, 128, 4096]):
        for e in (32768, 40000, 1 << 20):
            grown = _ws(dims, n, e) - _ws(dims, n, small)
            assert grown == _queue_bytes(e) - _queue_bytes(small) + _image_bytes(e), (dims, e, grown)
    # 3-Linear MLPs the kernel does not take: fewer than eight k1 chunks; k1 beyond the image variant's LDS (the fp32 kernel
    # and the kernel's per-tile prologue respectively)
    for dims in ([6, 160, 128, 4096], [6, 224, 256, 4096], [6, 1216, 256, 4096]):
        for e in (40000, 1 << 20):
            assert _ws(dims, n, e) - _ws(dims, n, small) == _queue_bytes(e) - _queue_bytes(small), (dims, e)
    # below 32,768 edges nothing is set aside
    for dims in ([6, 256, 256, 4096], [6, 1024, 1024, 4096]):
        assert _ws(dims, n, 30000) - _ws(dims, n, 20000) == _queue_bytes(30000) - _queue_bytes(20000)
    # two-Linear MLPs: no part of the workspace depends on the edges
    assert _ws([6, 256, 4096], n, 40000) == _ws([6, 256, 4096], n, small)
    # k0 = 8 (front layers run as dense layers): only the two activation buffers grow
    e1, e2 = 40000, 20000
    assert _ws([8, 256, 256, 4096], n, e1) - _ws([8, 256, 256, 4096], n, e2) == 2 * (e1 - e2) * 256 * 4


def test_headline_plan_keeps_four_chunks_with_the_image():
    n, e, dims = HEADLINE
    pm = _pm(dims)
    full = ops.workspace_bytes(n, e, pm)
    plan = ops.launch_plan(n, e, pm, full)
    assert (plan["n_chunks"], plan["nodes_per_chunk"], plan["attr_image"]) == (4, 16384, True), plan
    # one byte less: no room for the image beside the recommended node chunks - the plan of a workspace without it
    less = ops.launch_plan(n, e, pm, full - 1)
    assert less["attr_image"] is False, less
    zrow, prow = 64 * 1024 * 4, 64 * 64 * 4
    fixed = _al(n * 64 * 4) + 256 + _queue_bytes(e)
    npc = (full - 1 - fixed - 512) // (zrow + prow) // 64 * 64
    assert less["nodes_per_chunk"] == npc and less["n_chunks"] == -(-n // npc), (less, npc)
    # the flag turns it off at any size
    lib = _lib.lib()
    nch = ctypes.c_int32()
    flags = ops._PRECISION["f16split_noimage"]
    assert lib.gpde_nnconv_fwd_attr_image(n, e, 3, pm.dims_c, flags, full, ctypes.byref(nch)) == 0
    assert lib.gpde_nnconv_fwd_attr_image(n, e, 3, pm.dims_c, ops._PRECISION["f16split"], full, ctypes.byref(nch)) == 1
    assert nch.value == 4
    # the kernel's name does not depend on it
    assert ops.fused_kernel_name(n, e, pm, "f16split_noimage") == ops.fused_kernel_name(n, e, pm, "f16split") == "gpde_fused_f16v6_kernel"
    wide = _pm([6, 1216, 1024, 4096])
    assert ops.fused_kernel_name(n, e, wide, "f16split") == "gpde_fused_f16v6_kernel"
    assert ops.launch_plan(n, e, wide, ops.workspace_bytes(n, e, wide))["attr_image"] is False


def test_flag_value_matches_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpde.h")).read()
    m = re.search(r"GPDE_FWD_NO_ATTR_IMAGE\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.GPDE_FWD_NO_ATTR_IMAGE == 128
    assert ops._PRECISION["f16split_noimage"] == _lib.GPDE_FWD_F16SPLIT | _lib.GPDE_FWD_NO_ATTR_IMAGE
