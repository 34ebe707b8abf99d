"""CPU tier: the host side of the STREAMED any-width route (csrc/gpde_chain_any.hip: gpde_nnconv_chain_any_plan /
gpde_nnconv_chain_any_workspace_bytes / gpde_nnconv_fwd_chain_any / gpde_nnconv_bwd_chain_any) - the ABI, the plan's arithmetic
on hand-made rowptrs, every refusal the two entry points make before any device work (with null device pointers), and the routing
rule of ops.any_width_route(mode="streamed").  No GPU."""
import ctypes
import re
import subprocess

import pytest
import torch

import graph_pde_amd  # noqa: F401
from graph_pde_amd import _lib, ops

NEW = ("gpde_nnconv_chain_any_plan", "gpde_nnconv_chain_any_workspace_bytes", "gpde_nnconv_fwd_chain_any", "gpde_nnconv_bwd_chain_any")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
DIMS = [6, 12, 33, 24 * 40]
WIDTHS = (24, 24, 40)


def test_header_binding_and_library_have_the_entry_points():
    protos = _lib.header_prototypes()
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES, name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gpde_")}
    assert set(NEW) <= exported and exported == set(protos), sorted(exported ^ set(protos))
    assert protos["gpde_nnconv_fwd_chain_any"][1][-1] == "void*" and protos["gpde_nnconv_bwd_chain_any"][1][-1] == "void*"   # the stream
    assert "int32_t*" in protos["gpde_nnconv_fwd_chain_any"][1]                                      # n_bad
    assert len(protos["gpde_nnconv_bwd_chain_any"][1]) == len(protos["gpde_nnconv_fwd_chain_any"][1]) + 8


def test_version_is_still_101():
    assert int(re.search(r"#define\s+GPDE_VERSION\s+(\d+)", open(_lib.HEADER_PATH).read()).group(1)) == 101
    assert _lib.GPDE_VERSION == 101 and (_lib.lib().gpde_version() & 0xffff) == 101


def _plan(degrees, budget, dims=DIMS, widths=WIDTHS, want_table=True):
    rp = torch.zeros(len(degrees) + 1, dtype=torch.int32)
    rp[1:] = torch.tensor(degrees, dtype=torch.int64).cumsum(0).to(torch.int32) if degrees else rp[1:]
    n, e = len(degrees), int(rp[-1])
    table = torch.full((n + 1, 2), -7, dtype=torch.int32)
    nb, wf, wb = ctypes.c_int64(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = _lib.lib().gpde_nnconv_chain_any_plan(rp.data_ptr(), n, e, len(dims) - 1, _lib.dims_array(dims), *widths, budget,
                                               table.data_ptr() if want_table else None, ctypes.byref(nb), ctypes.byref(wf), ctypes.byref(wb))
    return rc, table[:max(nb.value, 0) + 1].tolist(), nb.value, wf.value, wb.value, rp


def _per_edge(dims):
    """Bytes per hidden row of a backward block: every hidden width padded to 4 floats, kept once; dH; two dU buffers of the widest."""
    kp = [(k + 3) // 4 * 4 for k in dims[1:-1]]
    return (sum(kp) + kp[-1] + 2 * max(kp)) * 4


def test_plan_all_zero_degrees_is_one_block_without_rows():
    rc, table, nb, wf, wb, _ = _plan([0] * 9, 1 << 20)
    assert rc == 0 and nb == 1 and table == [[0, 0], [9, 0]] and wb >= wf > 0


def test_plan_hub_above_the_budget_is_a_block_of_its_own_and_the_sizes_cover_it():
    pe = _per_edge(DIMS)
    degrees = [2, 3, 500, 1, 0, 4]
    rc, table, nb, wf, wb, rp = _plan(degrees, 10 * pe)                    # ten rows per block; the hub has 500
    assert rc == 0 and table == [[0, 0], [2, 5], [3, 505], [6, 510]] and nb == 3
    rc, _, _, wf_small, wb_small, _ = _plan([2, 3, 5, 1, 0, 4], 10 * pe)
    assert rc == 0 and wb - wb_small >= (500 - 10) * pe and wf > wf_small           # the hub's rows are in both workspaces
    # the size query for this very table names the plan's sizes
    t = torch.tensor(table, dtype=torch.int32)
    f, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert _lib.lib().gpde_nnconv_chain_any_workspace_bytes(t.data_ptr(), nb, 6, 510, 3, _lib.dims_array(DIMS), *WIDTHS, ctypes.byref(f),
                                                            ctypes.byref(b)) == 0
    assert (f.value, b.value) == (wf, wb)


def test_plan_budget_of_one_edge_makes_every_non_empty_node_a_block():
    degrees = [0, 3, 0, 0, 2, 1, 0, 7, 0]
    rc, table, nb, _, _, rp = _plan(degrees, 1)
    assert rc == 0 and nb == sum(d > 0 for d in degrees) == 4
    assert table == [[0, 0], [4, 3], [5, 5], [7, 6], [9, 13]]               # nodes without in-edges join the block before them
    for (a, e0), (b, e1) in zip(table[:-1], table[1:]):
        assert sum(d > 0 for d in degrees[a:b]) == 1 and e0 == int(rp[a]) and e1 == int(rp[b])


def test_plan_budget_above_all_edges_is_one_block_and_edge_sums_equal_e():
    degrees = [5, 0, 17, 33, 1, 64]
    rc, table, nb, wf, wb, _ = _plan(degrees, 1 << 30)
    assert rc == 0 and nb == 1 and table == [[0, 0], [6, 120]]
    for budget in (1, 7 * _per_edge(DIMS), 40 * _per_edge(DIMS), 1 << 30):
        rc, table, nb, wf, wb, rp = _plan(degrees, budget)
        assert rc == 0 and wb >= wf
        assert sum(t1[1] - t0[1] for t0, t1 in zip(table[:-1], table[1:])) == 120 == int(rp[-1])
        assert all(t1[0] >= t0[0] and t1[1] >= t0[1] for t0, t1 in zip(table[:-1], table[1:])) and table[-1] == [6, 120]
        cap = max(1, budget // _per_edge(DIMS))
        assert all(t1[1] - t0[1] <= max(cap, max(degrees[t0[0]:t1[0]])) for t0, t1 in zip(table[:-1], table[1:]))
    assert _plan(degrees, 1 << 30, want_table=False)[2] == 1                # NULL table: count and sizes only


def test_plan_refuses_a_block_of_two_to_the_31_elements():
    dims = [6, 4096, 8 * 8]
    rc, *_ = _plan([3, 1 << 19, 2], 1 << 20, dims=dims, widths=(8, 8, 8))     # 2^19 rows x 4096 floats = 2^31
    assert rc == EUNSUPPORTED and "2^31" in _lib.lib().gpde_last_error().decode()
    rc, *_ = _plan([3, (1 << 19) - 1, 2], 1 << 20, dims=dims, widths=(8, 8, 8))
    assert rc == 0


def test_plan_refuses_bad_arguments():
    lib = _lib.lib()
    nb = ctypes.c_int64()
    rp = torch.tensor([0, 2, 1, 4], dtype=torch.int32)
    args = lambda rowptr, n, e, dims, widths: (rowptr, n, e, len(dims) - 1, _lib.dims_array(dims), *widths, 1 << 20, None, ctypes.byref(nb), None, None)
    assert lib.gpde_nnconv_chain_any_plan(*args(rp.data_ptr(), 3, 4, DIMS, WIDTHS)) == EINVAL            # rowptr decreases
    assert lib.gpde_nnconv_chain_any_plan(*args(rp.data_ptr(), 3, 5, DIMS, WIDTHS)) == EINVAL            # does not end at n_edges
    assert lib.gpde_nnconv_chain_any_plan(*args(None, 3, 4, DIMS, WIDTHS)) == EINVAL
    ok = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
    assert lib.gpde_nnconv_chain_any_plan(*args(ok.data_ptr(), 3, 4, DIMS, WIDTHS)) == 0
    for dims, widths in (([6, 960], WIDTHS), ([6, 8, 8, 8, 8, 8, 960], WIDTHS), ([65, 12, 960], WIDTHS), ([0, 12, 960], WIDTHS),
                         ([6, 4097, 960], WIDTHS), ([6, 0, 960], WIDTHS), ([6, 12, 257 * 40], (257, 257, 40)), ([6, 12, 960], (24, 0, 40))):
        assert lib.gpde_nnconv_chain_any_plan(*args(ok.data_ptr(), 3, 4, dims, widths)) == EUNSUPPORTED, (dims, widths)
    assert lib.gpde_nnconv_chain_any_plan(*args(ok.data_ptr(), 3, 4, [6, 12, 961], WIDTHS)) == EINVAL     # last Linear != in * out


# ---- the two entry points: every refusal comes before any device work, so null device pointers reach all of them ---------------------------
def _fwd(table, n_blocks, *, n_dst=3, n_edges=4, dims=DIMS, widths=WIDTHS, aggr=_lib.GPDE_AGGR_MEAN, ws_bytes=0, weights="null", square=1,
         n_src=3):
    w = None if weights is None else (ctypes.c_void_p * (len(dims) - 1))()
    t = None if table is None else torch.tensor(table, dtype=torch.int32)
    return _lib.lib().gpde_nnconv_fwd_chain_any(None, n_src, None, n_dst, square, None, n_edges, None, None, len(dims) - 1, _lib.dims_array(dims), w, None,
                                                None, None, aggr, *widths, None if t is None else t.data_ptr(), n_blocks, None, None, None, ws_bytes,
                                                None)


def _bwd(table, n_blocks, *, n_dst=3, n_edges=4, dims=DIMS, widths=WIDTHS, aggr=_lib.GPDE_AGGR_MEAN, ws_bytes=0, weights="null", square=1,
         n_src=3):
    w = None if weights is None else (ctypes.c_void_p * (len(dims) - 1))()
    t = None if table is None else torch.tensor(table, dtype=torch.int32)
    return _lib.lib().gpde_nnconv_bwd_chain_any(None, n_src, None, n_dst, square, None, n_edges, None, None, len(dims) - 1, _lib.dims_array(dims), w, None,
                                                None, aggr, *widths, None, None, None, None, None, None, None, None, None, None,
                                                None if t is None else t.data_ptr(), n_blocks, None, None, ws_bytes, None)


GOOD = [[0, 0], [2, 3], [3, 4]]


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_entry_point_refusals_with_null_device_pointers(call):
    err = lambda: _lib.lib().gpde_last_error().decode()
    # host arguments
    assert call(None, 2) == EINVAL and call(GOOD, 2, weights=None) == EINVAL and call(GOOD, 2, n_edges=-1) == EINVAL
    assert call(GOOD, 2, square=0, n_src=0) == EINVAL                                   # edges without sources
    # the chain and the widths
    for dims in ([6, 960], [6, 8, 8, 8, 8, 8, 960], [65, 12, 960], [6, 4097, 960]):
        assert call(GOOD, 2, dims=dims) == EUNSUPPORTED, dims
    assert call(GOOD, 2, widths=(257, 257, 40), dims=[6, 12, 257 * 40]) == EUNSUPPORTED
    assert call(GOOD, 2, aggr=_lib.GPDE_AGGR_MAX) == EUNSUPPORTED and call(GOOD, 2, aggr=9) == EINVAL
    assert call(GOOD, 2, dims=[6, 12, 961]) == EINVAL
    # the block table: not monotone, not ending at (n_dst, n_edges), not starting at (0, 0), slots in a block without nodes
    for table, nb in (([[0, 0], [2, 3], [1, 3], [3, 4]], 3), ([[0, 0], [2, 3], [3, 2], [3, 4]], 3), ([[0, 0], [2, 3]], 1), ([[0, 0], [2, 3], [3, 5]], 2),
                      ([[1, 0], [2, 3], [3, 4]], 2), ([[0, 0], [0, 3], [3, 4]], 2)):
        assert call(table, nb) == EINVAL, table
        assert "table" in err()
    # 2^31 elements in one block
    assert call([[0, 0], [1, 1 << 19]], 1, n_dst=1, n_edges=1 << 19, dims=[6, 4096, 64], widths=(8, 8, 8)) == EUNSUPPORTED and "2^31" in err()
    # the workspace: too small is GPDE_EWORKSPACE and the message names the plan's size
    f, b = ctypes.c_size_t(), ctypes.c_size_t()
    t = torch.tensor(GOOD, dtype=torch.int32)
    assert _lib.lib().gpde_nnconv_chain_any_workspace_bytes(t.data_ptr(), 2, 3, 4, 3, _lib.dims_array(DIMS), *WIDTHS, ctypes.byref(f), ctypes.byref(b)) == 0
    need = f.value if call is _fwd else b.value
    assert call(GOOD, 2, ws_bytes=need - 1) == EWORKSPACE and str(need) in err()
    # ... and with room for it, the null device pointers are what is left to refuse
    assert call(GOOD, 2, ws_bytes=need) == EINVAL and "null device argument" in err()
    # an empty block in the table is valid (the refusal is again the null pointers)
    assert call([[0, 0], [2, 3], [2, 3], [3, 4]], 3, ws_bytes=need) == EINVAL and "null device argument" in err()


def test_zero_destinations_need_nothing():
    assert _fwd([[0, 0]], 0, n_dst=0, n_edges=0, n_src=0) == 0
    assert _bwd([[0, 0]], 0, n_dst=0, n_edges=0, n_src=0) == 0


# ---- the routing rule ------------------------------------------------------------------------------------------------------------------------
def test_streamed_mode_takes_every_eligible_call():
    r = ops.any_width_route(100, 1000, 24, 40, 33, "mean", True, 1, mode="streamed", dims=[6, 12, 33, 960])       # (nothing free: no refusal)
    assert r["route"] == "streamed" and r["eligible"]
    assert r["bytes_streamed"] == 1000 * 24 * 4 + 2 * 24 * 36 * 40 * 4       # the per-edge dx rows, P and dP: KP = 36, out padded to 40
    assert ops.any_width_route(100, 1000, 24, 40, 33, "add", True, 1 << 40, mode="streamed")["route"] == "streamed"     # dims left to the caller
    assert ops.chain_any_supported([6, 12, 33, 960]) and ops.chain_any_supported([64, 4096, 4])
    for dims in ([6, 960], [65, 12, 960], [6, 4097, 960], [6, 1, 2, 3, 4, 5, 960], None):
        assert not ops.chain_any_supported(dims), dims


@pytest.mark.parametrize("kw", [dict(aggr="max"), dict(chain=False, k_hidden=None), dict(k_hidden=4097), dict(dims=[65, 33, 960]), dict(dims=[6, 960])])
@pytest.mark.parametrize("free", [1 << 40, 1000])
def test_streamed_mode_sends_ineligible_calls_where_off_sends_them(kw, free):
    a = dict(n_nodes=100, n_edges=1000, in_channels=24, out_channels=40, k_hidden=33, aggr="mean", chain=True, free_bytes=free)
    a.update(kw)
    s = ops.any_width_route(mode="streamed", **a)
    off = ops.any_width_route(mode="off", **a)
    assert s["route"] == off["route"] in ("materialised", "refused") and s == off


def _old_rule(n, e, cin, cout, k, aggr, chain, free, mode):
    """ops.any_width_route as it was before the streamed mode (tests/test_reassoc_host.py states the same rule in words)."""
    eligible = bool(chain) and aggr in ("add", "mean") and k is not None and 1 <= k <= 4096
    bytes_m = e * cin * cout * 4
    out = {"eligible": eligible, "bytes_materialised": bytes_m, "bytes_reassociated": None, "node_block": None,
           "flops_materialised": None if k is None else 2 * e * k * cin * cout, "flops_reassociated": None}
    fits_r = False
    if eligible:
        zrow = cin * ((k + 4) // 4 * 4) * 4
        out["node_block"] = max(1, min(n, (512 << 20) // zrow))
        out["bytes_reassociated"] = e * k * 4 + out["node_block"] * zrow
        out["flops_reassociated"] = 2 * e * cin * k + 2 * n * cin * k * cout
        fits_r = 2 * out["bytes_reassociated"] <= free
    if mode == "on" and eligible:
        out["route"] = "reassociated" if fits_r else "refused"
    elif 2 * bytes_m <= free:
        out["route"] = "materialised"
    elif mode == "auto" and fits_r:
        out["route"] = "reassociated"
    else:
        out["route"] = "refused"
    return out


@pytest.mark.parametrize("mode", ["auto", "on", "off"])
def test_auto_on_off_results_are_unchanged(mode):
    """The argument sets of tests/test_reassoc_host.py: every key the result had keeps its value; `bytes_streamed` is the one new key."""
    sets = [(100, 1000, 24, 40, 33, "mean", True), (5000, 10, 256, 256, 1023, "add", True), (0, 0, 8, 8, 3, "add", True),
            (100, 1000, 24, 40, 33, "add", True), (1, 1, 1, 1, 1, "add", True), (100, 1000, 24, 40, 33, "max", True),
            (100, 1000, 24, 40, None, "mean", False), (100, 1000, 24, 40, 4097, "mean", True)]
    for args in sets:
        for free in (1 << 40, 1 << 50, 7_680_000, 7_679_999, 955_200, 955_199, 1000, 1):
            r = ops.any_width_route(*args, free, mode=mode)
            want = _old_rule(*args, free, mode)
            assert {k: r[k] for k in want} == want and set(r) - set(want) == {"bytes_streamed"}, (args, free, r)
    with pytest.raises(ValueError, match="must be auto, on or off"):
        ops.any_width_route(1, 1, 1, 1, 1, "add", True, 1, mode="maybe")
