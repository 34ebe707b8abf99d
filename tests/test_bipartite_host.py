"""CPU tier: the host side of NNConv between two node sets (no device): constructor, validation, refusals, `ops.Csr` with a
source count, the CSR cache key, the node count the route is asked with, and the C ABI additions in the header / binding."""
import re

import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops

NEW_SYMBOLS = ("gpde_csr_from_coo2", "gpde_nnconv_fwd_edgeweights_bip", "gpde_nnconv_bwd_edgeweights_bip",
               "gpde_nnconv_bwd_edgeweights_bip_workspace_bytes", "gpde_nnconv_fwd_hidden_bip", "gpde_nnconv_bwd_hidden_bip",
               "gpde_nnconv_fwd_hidden_bip_workspace_bytes", "gpde_nnconv_bwd_hidden_bip_workspace_bytes")


def net(cin, cout, k0=3):
    return torch.nn.Sequential(torch.nn.Linear(k0, 8), torch.nn.ReLU(), torch.nn.Linear(8, cin * cout))


def graph(n_src=5, n_dst=7, e=11):
    g = torch.Generator().manual_seed(0)
    return torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst, (e,), generator=g)]), torch.rand(e, 3, generator=g)


# ---- constructor -------------------------------------------------------------------------------------------------------------
def test_constructor_takes_a_channel_pair():
    conv = gp.NNConv((24, 7), 40, net(24, 40))
    assert conv.in_channels == (24, 7) and conv.out_channels == 40
    assert tuple(conv.root.shape) == (7, 40) and tuple(conv.bias.shape) == (40,)
    bound = 1.0 / 24 ** 0.5                                   # reset_parameters keeps size = in_src
    assert float(conv.root.detach().abs().max()) <= bound and float(conv.bias.detach().abs().max()) <= bound
    assert repr(conv) == "NNConv((24, 7), 40)" and repr(gp.NNConv_old(3, 5, net(3, 5))) == "NNConv_old(3, 5)"
    other = gp.NNConv((24, 7), 40, net(24, 40))
    other.load_state_dict(conv.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(conv.state_dict().values(), other.state_dict().values()))
    assert gp.NNConv([24, 7], 40, net(24, 40), root_weight=False).root is None
    with pytest.raises(ValueError, match="pair"):
        gp.NNConv((1, 2, 3), 4, net(1, 4))


def test_constructor_takes_target_to_source():
    conv = gp.NNConv(3, 5, net(3, 5), flow="target_to_source")
    assert conv.flow == "target_to_source" and gp.NNConv(3, 5, net(3, 5)).flow == "source_to_target"
    with pytest.raises(ValueError, match="flow"):
        gp.NNConv(3, 5, net(3, 5), flow="sideways")


# ---- validation before any device is needed ----------------------------------------------------------------------------------
def test_shape_and_size_validation_needs_no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("validation must not reach the device")
    for name in ("staging_device", "csr_for", "device_free_bytes"):
        monkeypatch.setattr(ops, name, boom)
    ei, ea = graph()
    conv = gp.NNConv((4, 2), 3, net(4, 3))
    xs, xd = torch.randn(5, 4), torch.randn(7, 2)
    cases = [
        (((xs, xd, xd), ei, ea), {}, "pair"),                                             # arity
        (((xs[:, :3], xd), ei, ea), {}, "x_src must be"),                                 # width of x_src against in_src
        (((xs, torch.randn(7, 4)), ei, ea), {}, "x_dst must be"),                         # width of x_dst against in_dst
        (((xs, xd), ei, ea), {"size": (6, 7)}, r"size\[0\]"),                             # size against the tensors
        (((xs, xd), ei, ea), {"size": (5, 8)}, r"size\[1\]"),
        (((xs, xd), ei, ea), {"size": (5, 7, 1)}, "size must be"),
        (((xs, None), ei, ea), {}, "number of destination nodes is unknown"),             # neither size nor x_dst
        (((xs, None), ei, ea), {"size": (5, None)}, "number of destination nodes is unknown"),
        (((xs, xd), ei, ea), {"residual": torch.randn(5, 3)}, "residual must be"),
        ((xs, ei, ea), {"size": (5, 7)}, r"size\[1\]"),                                   # one tensor cannot serve two node counts
    ]
    for args, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            conv(*args, **kw)
    with pytest.raises(ValueError, match=r"size\[1\]"):
        conv.propagate(ei, size=(5, 8), x=(xs, xd), pseudo=ea)
    with pytest.raises(ValueError, match="x_dst must be"):
        gp.NNConv(4, 3, net(4, 3))((xs, xd), ei, ea)                                      # one width: x_dst must have it too


def test_refusals_name_the_limit(monkeypatch):
    monkeypatch.setattr(ops, "staging_device", lambda: (_ for _ in ()).throw(AssertionError("refusals come before the device")))
    ei, ea = graph()
    xs, xd = torch.randn(5, 4), torch.randn(7, 2)
    conv = gp.NNConv((4, 2), 3, net(4, 3), aggr="max")
    with pytest.raises(NotImplementedError, match="aggr='max' with a gradient on a call between two node sets"):
        conv((xs, xd), ei, ea)
    na = ops.NodeAttr(torch.randn(7, 3), [(0, 0), (1, 1), (0, 2)])
    with pytest.raises(NotImplementedError, match="NodeAttr attributes on a call between two node sets"):
        gp.NNConv((4, 2), 3, net(4, 3))((xs, xd), ei, na)
    with pytest.raises(NotImplementedError, match="NodeAttr attributes with flow='target_to_source'"):
        gp.NNConv(4, 3, net(4, 3), flow="target_to_source")(xs, ei, na)
    csr = ops.Csr(7, 0, torch.zeros(8, dtype=torch.int32), *(torch.zeros(0, dtype=torch.int32) for _ in range(3)), n_src_nodes=5)
    with pytest.raises(NotImplementedError, match="a CSR has its direction built in"):
        gp.NNConv(4, 3, net(4, 3), flow="target_to_source")(torch.randn(7, 4), ops.Csr(7, 0, csr.rowptr, csr.src, csr.dst, csr.perm), ea[:0])
    pair = gp.NNConv((4, 2), 3, net(4, 3))
    with pytest.raises(NotImplementedError):                  # message() / update() keep their square meaning
        pair.message(xs, ea[:5])


def test_a_rectangular_call_in_a_group_runs_on_its_own(monkeypatch):
    ei, ea = graph()
    xs, xd = torch.randn(5, 4), torch.randn(7, 2)
    conv = gp.NNConv((4, 2), 3, net(4, 3))
    seen = []
    monkeypatch.setattr(gp.NNConv, "forward", lambda self, x, ei_, ea_, **kw: seen.append((x, kw)) or "ran alone")
    monkeypatch.setattr(ops, "nnconv_forward_edgeweights_group", lambda calls: [] if not calls else pytest.fail("shared launch"))
    from graph_pde_amd.nn_conv import nnconv_group
    assert nnconv_group([(conv, (xs, xd), ei, ea, None, "relu")]) == ["ran alone"]
    assert seen[0][0][0] is xs and seen[0][1] == {"residual": None, "activation": "relu"}


def test_the_same_tensor_twice_is_the_square_call(monkeypatch):
    """A pair whose two tensors are the same object (size square or None) takes the square path: propagate is reached with x."""
    ei, ea = graph(5, 5)
    x = torch.randn(5, 4)
    conv = gp.NNConv_old(4, 3, net(4, 3))
    got = []
    monkeypatch.setattr(conv, "_propagate_any_width", lambda x_, ei_, ps, **k: got.append(x_) or "square")
    monkeypatch.setattr(conv, "_propagate_rect", lambda *a, **k: "rect")
    assert conv((x, x), ei, ea) == "square" and conv((x, x), ei, ea, size=(5, 5)) == "square" and conv(x, ei, ea, size=5) == "square"
    assert all(t is x for t in got)
    assert conv((x, x.clone()), ei, ea) == "rect" and conv((x, None), ei, ea, size=(5, 9)) == "rect"


# ---- ops.Csr, the cache key, the route ---------------------------------------------------------------------------------------
def test_csr_with_and_without_a_source_count():
    z = torch.zeros(0, dtype=torch.int32)
    sq = ops.Csr(7, 0, torch.zeros(8, dtype=torch.int32), z, z, z)
    assert sq.n_src_nodes is None and sq.n_src == 7 and sq.n_nodes == 7
    rect = ops.Csr(7, 0, torch.zeros(8, dtype=torch.int32), z, z, z, n_src_nodes=5)
    assert rect.n_src == 5 and rect.n_nodes == 7
    assert ops.csr_for(sq, 7) is sq and ops.csr_for(rect, 7, n_src=5) is rect
    with pytest.raises(ValueError, match="source nodes"):
        ops.csr_for(rect, 7)                                  # a rectangular CSR in a square call
    with pytest.raises(ValueError, match="source nodes"):
        ops.csr_for(sq, 7, n_src=5)
    with pytest.raises(ValueError, match="7 nodes"):
        ops.csr_for(rect, 8, n_src=5)


def test_the_csr_cache_key_includes_the_source_count_and_the_flip(monkeypatch):
    built = []
    monkeypatch.setattr(ops, "build_csr", lambda ei, n, n_src=None, flip=False: built.append((n, n_src, flip)) or object())
    monkeypatch.setattr(ops, "_csr_cache", ops.Lru("csr", max_entries=64, max_bytes=8 << 30))
    ei, _ = graph(5, 5)
    a, b, c, d = ops.csr_for(ei, 5), ops.csr_for(ei, 5, n_src=5), ops.csr_for(ei, 5, n_src=9), ops.csr_for(ei, 5, flip=True)
    assert len({id(t) for t in (a, b, c, d)}) == 4 and built == [(5, None, False), (5, 5, False), (5, 9, False), (5, None, True)]
    assert ops.csr_for(ei, 5) is a and ops.csr_for(ei, 5, n_src=9) is c and ops.csr_for(ei, 5, flip=True) is d and len(built) == 4
    square_keys = [k for k in ops._csr_cache if len(k) == 7]
    assert len(square_keys) == 1                               # the square key is what it always was


def test_the_route_is_asked_with_n_dst(monkeypatch):
    ei, ea = graph(5, 7)
    z = torch.zeros(0, dtype=torch.int32)
    monkeypatch.setattr(ops, "staging_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "csr_for", lambda e, n, n_src=None, flip=False: ops.Csr(n, 11, torch.zeros(n + 1, dtype=torch.int32), z, z, z,
                                                                                       n_src_nodes=n_src))
    monkeypatch.setattr(ops, "device_free_bytes", lambda dev: (1 << 40, 1 << 40))
    asked = []

    class Stop(Exception):
        pass

    def route(n_nodes, n_edges, cin, cout, k, aggr, chain, free, mode=None):
        asked.append((n_nodes, n_edges, cin, cout, k, aggr, chain))
        raise Stop
    monkeypatch.setattr(ops, "any_width_route", route)
    with pytest.raises(Stop), torch.no_grad():
        gp.NNConv((4, 2), 3, net(4, 3), aggr="mean")((torch.randn(5, 4), torch.randn(7, 2)), ei, ea)
    assert asked == [(7, 11, 4, 3, 8, "mean", True)]


# ---- the C ABI additions -----------------------------------------------------------------------------------------------------
def test_header_declares_every_new_symbol_and_the_binding_has_it():
    protos = _lib.header_prototypes()
    for name in NEW_SYMBOLS:
        assert name in protos and name in _lib.SIGNATURES, name
    assert protos["gpde_csr_from_coo2"][1][3:6] == ["int64_t", "int64_t", "int64_t"]          # n_edges, n_src, n_dst
    assert len(protos["gpde_nnconv_fwd_edgeweights_bip"][1]) == len(protos["gpde_nnconv_fwd_edgeweights_any"][1]) + 3
    assert len(protos["gpde_nnconv_bwd_edgeweights_bip"][1]) == len(protos["gpde_nnconv_bwd_edgeweights_any"][1]) + 4
    assert len(protos["gpde_nnconv_fwd_hidden_bip"][1]) == len(protos["gpde_nnconv_fwd_hidden_any"][1]) + 3
    assert len(protos["gpde_nnconv_bwd_hidden_bip"][1]) == len(protos["gpde_nnconv_bwd_hidden_any"][1]) + 4
    assert re.search(r"#define\s+GPDE_VERSION\s+101\b", open(_lib.HEADER_PATH).read())


def test_workspace_queries_are_host_arithmetic():
    lib = _lib.lib()
    assert lib.gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(5, 5, 9, 24, 24, 40) == lib.gpde_nnconv_bwd_edgeweights_any_workspace_bytes(5, 9, 24, 40)
    assert lib.gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(5, 7, 9, 24, 100, 40) > lib.gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(5, 7, 9, 24, 7, 40)
    assert lib.gpde_nnconv_bwd_edgeweights_bip_workspace_bytes(5, 7, 9, 24, 257, 40) == 0
    assert lib.gpde_nnconv_fwd_hidden_bip_workspace_bytes(7, 9, 24, 40, 33) == lib.gpde_nnconv_fwd_hidden_any_workspace_bytes(7, 9, 24, 40, 33)
    assert lib.gpde_nnconv_bwd_hidden_bip_workspace_bytes(7, 9, 24, 24, 40, 33) == lib.gpde_nnconv_bwd_hidden_any_workspace_bytes(7, 9, 24, 40, 33)
    assert lib.gpde_nnconv_bwd_hidden_bip_workspace_bytes(7, 9, 24, 0, 40, 33) == 0
