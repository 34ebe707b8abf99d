"""CPU tier: the host side of the re-associated any-width route - ops.any_width_route's byte / FLOP arithmetic and routing rule,
and the four entry points of include/gpde.h (csrc/gpde_reassoc_any.hip) in the header, the binding and the library."""
import os
import re
import subprocess

import pytest

from graph_pde_amd import _lib, ops

MIB = 1 << 20


def test_bytes_and_flops_by_hand():
    # 100 nodes, 1000 edges, 24 -> 40, K = 33: per-edge weights 1000 * 24 * 40 * 4; H 1000 * 33 * 4; Z' row 24 * 36 floats (33 + 1 -> 36)
    r = ops.any_width_route(100, 1000, 24, 40, 33, "mean", True, 1 << 40, mode="auto")
    assert r["bytes_materialised"] == 3_840_000
    assert r["node_block"] == 100 and r["bytes_reassociated"] == 132_000 + 100 * 24 * 36 * 4 == 477_600
    assert r["flops_materialised"] == 2 * 1000 * 33 * 24 * 40 == 63_360_000
    assert r["flops_reassociated"] == 2 * 1000 * 24 * 33 + 2 * 100 * 24 * 33 * 40 == 7_920_000
    # 256 -> 256, K = 1023: a Z' row is 256 * 1024 * 4 = 1 MiB, the node block is capped at 512 of the 5000 nodes
    r = ops.any_width_route(5000, 10, 256, 256, 1023, "add", True, 1 << 40, mode="on")
    assert r["node_block"] == 512 and r["bytes_reassociated"] == 10 * 1023 * 4 + 512 * MIB
    assert r["bytes_materialised"] == 10 * 256 * 256 * 4
    # no node: a block is never smaller than one node
    assert ops.any_width_route(0, 0, 8, 8, 3, "add", True, 1 << 30)["node_block"] == 1


@pytest.mark.parametrize("free,expect", [(7_680_000, "materialised"), (7_679_999, "reassociated"), (955_200, "reassociated"), (955_199, "refused")])
def test_auto_reroutes_only_what_was_refused(free, expect):
    r = ops.any_width_route(100, 1000, 24, 40, 33, "mean", True, free, mode="auto")
    assert r["route"] == expect, r
    off = ops.any_width_route(100, 1000, 24, 40, 33, "mean", True, free, mode="off")["route"]
    assert off == ("materialised" if expect == "materialised" else "refused")
    if off == "materialised":
        assert r["route"] == "materialised"                     # a call that runs today runs as today


def test_on_and_off():
    big = 1 << 40
    assert ops.any_width_route(100, 1000, 24, 40, 33, "add", True, big, mode="on")["route"] == "reassociated"
    assert ops.any_width_route(100, 1000, 24, 40, 33, "add", True, 955_199, mode="on")["route"] == "refused"
    assert ops.any_width_route(100, 1000, 24, 40, 33, "add", True, big, mode="off")["route"] == "materialised"
    assert ops.any_width_route(100, 1000, 24, 40, 33, "add", True, 1000, mode="off")["route"] == "refused"
    with pytest.raises(ValueError):
        ops.any_width_route(1, 1, 1, 1, 1, "add", True, 1, mode="maybe")
    assert ops.ANY_REASSOC == os.environ.get("GPDE_ANY_REASSOC", "auto")


@pytest.mark.parametrize("kw", [dict(aggr="max"), dict(chain=False), dict(k_hidden=4097), dict(k_hidden=None, chain=False), dict(k_hidden=0)])
@pytest.mark.parametrize("mode", ["auto", "on", "off"])
def test_never_reassociated(kw, mode):
    a = dict(n_nodes=100, n_edges=1000, in_channels=24, out_channels=40, k_hidden=33, aggr="mean", chain=True)
    a.update(kw)
    for free in (1 << 40, 955_200, 10):
        r = ops.any_width_route(free_bytes=free, mode=mode, **a)
        assert not r["eligible"] and r["route"] == ("materialised" if free >= 7_680_000 else "refused"), r


NEW = ("gpde_nnconv_fwd_hidden_any_workspace_bytes", "gpde_nnconv_fwd_hidden_any", "gpde_nnconv_bwd_hidden_any_workspace_bytes",
       "gpde_nnconv_bwd_hidden_any")


def test_header_declares_and_the_binding_binds_the_new_entry_points():
    protos = _lib.header_prototypes()
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES, name
    assert protos[NEW[0]] == ("size_t", ["int64_t", "int64_t", "int", "int", "int"]) == protos[NEW[2]]
    assert protos[NEW[1]][0] == "int" and len(protos[NEW[1]][1]) == 18 and protos[NEW[1]][1][-3:] == ["void*", "size_t", "void*"]
    assert protos[NEW[3]][0] == "int" and len(protos[NEW[3]][1]) == 25 and protos[NEW[3]][1][-5:] == ["const int32_t*"] * 2 + ["void*", "size_t", "void*"]
    hdr = open(_lib.HEADER_PATH).read()
    assert re.search(r"#define\s+GPDE_REASSOC_ANY_MAX_HIDDEN\s+4096\b", hdr) and _lib.GPDE_REASSOC_ANY_MAX_HIDDEN == 4096 == ops.ANY_MAX_HIDDEN
    assert re.search(r"#define\s+GPDE_VERSION\s+101\b", hdr)    # additions only
    lib = _lib.lib()                                            # resolves every declared symbol
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", syms, flags=re.M), name
    # workspace queries are host arithmetic: preferred size grows with the node block up to its cap, 0 outside the built range
    w1, w2, w3 = (int(lib.gpde_nnconv_fwd_hidden_any_workspace_bytes(n, 1000, 24, 40, 33)) for n in (1, 2, 3))
    assert w2 - w1 == w3 - w2 == (24 * 36 + 40) * 4
    b1, b2 = (int(lib.gpde_nnconv_bwd_hidden_any_workspace_bytes(n, 1000, 24, 40, 33)) for n in (1, 2))
    assert b2 - b1 == (2 * 24 * 36 + 40) * 4
    assert int(lib.gpde_nnconv_fwd_hidden_any_workspace_bytes(10**9, 10, 256, 256, 1023)) < 600 * MIB + 256 * 1024 * 256 * 4 + 512 * 32 * 256 * 4
    # the node block any_width_route reports is the library's own preferred block (RA_PREF_Z_BYTES of gpde_reassoc_any.hip and
    # ops._ANY_PREF_Z_BYTES are one number): nodes of the preferred workspace = (w(N) - w(1)) / (w(2) - w(1)) + 1
    for n, e, cin, cout, k in ((100, 1000, 24, 40, 33), (5000, 10, 256, 256, 1023), (10**6, 10, 128, 96, 100), (3, 10, 1, 1, 1), (10**6, 10, 256, 1, 4096)):
        wn, v1, v2 = (int(lib.gpde_nnconv_fwd_hidden_any_workspace_bytes(m, e, cin, cout, k)) for m in (n, 1, 2))
        bn, c1, c2 = (int(lib.gpde_nnconv_bwd_hidden_any_workspace_bytes(m, e, cin, cout, k)) for m in (n, 1, 2))
        block = ops.any_width_route(n, e, cin, cout, k, "add", True, 1 << 50)["node_block"]
        assert (wn - v1) // (v2 - v1) + 1 == block == (bn - c1) // (c2 - c1) + 1, (n, e, cin, cout, k)
    for bad in ((1, 1, 0, 40, 33), (1, 1, 24, 257, 33), (1, 1, 24, 40, 0), (1, 1, 24, 40, 4097), (-1, 1, 24, 40, 33)):
        assert int(lib.gpde_nnconv_fwd_hidden_any_workspace_bytes(*bad)) == 0 == int(lib.gpde_nnconv_bwd_hidden_any_workspace_bytes(*bad))
