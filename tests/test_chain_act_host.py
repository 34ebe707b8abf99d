"""CPU tier: the host side of the streamed any-width route for kernel networks with OTHER ACTIVATIONS than the ReLU
(csrc/gpde_chain_any.hip: gpde_nnconv_chain_act_plan / gpde_nnconv_chain_act_workspace_bytes / gpde_nnconv_fwd_chain_act /
gpde_nnconv_bwd_chain_act) - what ops.mlp_chain recognises, the routing rule of ops.any_width_route(acts=...), the plan's and the
size query's arithmetic for each kind and the refusals of a kind or a parameter the library does not take.  No GPU."""
import ctypes
import subprocess

import pytest
import torch
from torch import nn

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops

NEW = ("gpde_nnconv_chain_act_plan", "gpde_nnconv_chain_act_workspace_bytes", "gpde_nnconv_fwd_chain_act", "gpde_nnconv_bwd_chain_act")
EINVAL, EUNSUPPORTED = -1, -2
DIMS = [6, 33, 65, 24 * 40]
WIDTHS = (24, 24, 40)
KINDS = {"relu": ops.ACT_RELU, "leaky_relu": ops.ACT_LEAKY_RELU, "elu": ops.ACT_ELU, "tanh": ops.ACT_TANH, "sigmoid": ops.ACT_SIGMOID,
         "gelu": ops.ACT_GELU, "gelu_tanh": ops.ACT_GELU_TANH, "silu": ops.ACT_SILU, "sin": ops.ACT_SIN}
FROM_U = ("gelu", "gelu_tanh", "silu", "sin")


class DenseNet(nn.Module):
    """The reference's DenseNet(layers, nonlinearity) as far as the parser sees it: Linears and activation modules in `.layers`."""

    def __init__(self, layers, nonlinearity, out_nonlinearity=None, normalize=False):
        super().__init__()
        self.layers = nn.ModuleList()
        for j in range(len(layers) - 1):
            self.layers.append(nn.Linear(layers[j], layers[j + 1]))
            if j != len(layers) - 2:
                if normalize:
                    self.layers.append(nn.BatchNorm1d(layers[j + 1]))
                self.layers.append(nonlinearity())
        if out_nonlinearity is not None:
            self.layers.append(out_nonlinearity())

    def forward(self, x):
        for l in self.layers:
            x = l(x)
        return x


# ---- ops.mlp_chain ---------------------------------------------------------------------------------------------------------------------------
def test_mlp_chain_recognises_each_module_with_its_parameters():
    seq = nn.Sequential(nn.Linear(6, 8), nn.LeakyReLU(0.2), nn.Linear(8, 9), nn.ELU(1.5), nn.Linear(9, 10), nn.GELU(), nn.Linear(10, 11),
                        nn.GELU(approximate="tanh"), nn.Linear(11, 12))
    lin, acts = ops.mlp_chain(seq)
    assert [l.out_features for l in lin] == [8, 9, 10, 11, 12]
    assert acts == [(ops.ACT_LEAKY_RELU, pytest.approx(0.2), 0.0), (ops.ACT_ELU, 1.5, 0.0), (ops.ACT_GELU, 0.0, 0.0), (ops.ACT_GELU_TANH, 0.0, 0.0)]
    for mod, kind in ((nn.ReLU, "relu"), (nn.Tanh, "tanh"), (nn.Sigmoid, "sigmoid"), (nn.SiLU, "silu"), (gp.Sin, "sin"), (nn.GELU, "gelu"),
                      (nn.LeakyReLU, "leaky_relu"), (nn.ELU, "elu")):
        lin, acts = ops.mlp_chain(DenseNet([6, 16, 32, 960], mod))
        assert len(lin) == 3 and [a[0] for a in acts] == [KINDS[kind]] * 2, kind
    assert ops.mlp_chain(DenseNet([6, 16, 960], nn.LeakyReLU))[1][0][1] == pytest.approx(0.01)          # torch's default slope
    assert ops.mlp_chain(nn.Sequential(nn.Linear(6, 16), nn.ReLU(inplace=True), nn.Linear(16, 960)))[1] == [(ops.ACT_RELU, 0.0, 0.0)]
    assert gp.Sin()(torch.tensor([0.5])).item() == pytest.approx(torch.sin(torch.tensor(0.5)).item()) and "Sin" in gp.__all__
    assert ops.acts_all_relu(None) and ops.acts_all_relu([(0, 0.0, 0.0)]) and not ops.acts_all_relu([(0, 0.0, 0.0), (3, 0.0, 0.0)])
    assert ops.acts_key([(0, 0.0, 0.0)]) is None and ops.acts_key([(1, 0.2, 0.0)]) == ((1, 0.2, 0.0),)


def test_mlp_chain_returns_none_for_everything_else():
    class MyTanh(nn.Tanh):
        def forward(self, x):
            return 2 * super().forward(x)

    class MyLinear(nn.Linear):
        def forward(self, x):
            return super().forward(x) + 1

    class SinInside(nn.Module):                # the reference's DenseNet_sin: torch.sin inside forward, only Linears in `.layers`
        def __init__(self):
            super().__init__()
            self.layers = nn.ModuleList([nn.Linear(6, 16), nn.Linear(16, 960)])

        def forward(self, x):
            return self.layers[1](torch.sin(self.layers[0](x)))

    for net in (DenseNet([6, 16, 960], nn.GELU, normalize=True),                       # BatchNorm
                DenseNet([6, 16, 960], nn.GELU, out_nonlinearity=nn.GELU),             # an output activation
                DenseNet([6, 16, 960], lambda: nn.LeakyReLU(-0.1)),
                DenseNet([6, 16, 960], nn.Softplus),
                DenseNet([6, 16, 960], lambda: nn.ELU(0.0)),
                DenseNet([6, 16, 960], MyTanh),
                nn.Sequential(MyLinear(6, 16), nn.Tanh(), nn.Linear(16, 960)),
                nn.Sequential(nn.Linear(6, 16), nn.Linear(16, 960)), nn.Sequential(nn.Linear(6, 16), nn.Tanh()), nn.Linear(6, 960),
                nn.Sequential(nn.Tanh(), nn.Linear(6, 960), nn.Tanh()), nn.Sequential(nn.Linear(6, 16), nn.Tanh(), nn.Linear(17, 960)),
                SinInside(), nn.Tanh()):
        assert ops.mlp_chain(net) is None, net


def test_mlp_linears_still_raises_its_old_messages():
    with pytest.raises(NotImplementedError, match=r"kernel network layer Tanh is not supported \(Linear/ReLU chains only\)"):
        ops.mlp_linears(DenseNet([6, 16, 960], nn.Tanh))
    with pytest.raises(NotImplementedError, match="kernel network layer GELU is not supported"):
        ops.mlp_linears(nn.Sequential(nn.Linear(6, 16), nn.GELU(), nn.Linear(16, 960)))
    with pytest.raises(NotImplementedError, match="two Linear layers without ReLU between them"):
        ops.mlp_linears(nn.Sequential(nn.Linear(6, 16), nn.Linear(16, 960)))
    with pytest.raises(NotImplementedError, match="is not a Linear/ReLU chain"):
        ops.mlp_linears(gp.Sin())
    assert len(ops.mlp_linears(DenseNet([6, 16, 960], nn.ReLU))) == 2


# ---- the routing rule ------------------------------------------------------------------------------------------------------------------------
TANH, GELU = [(ops.ACT_TANH, 0.0, 0.0)] * 2, [(ops.ACT_GELU, 0.0, 0.0)] * 2
ROUTE_ARGS = (100, 1000, 24, 40, 65, "mean", True)
BYTES_M = 1000 * 24 * 40 * 4


@pytest.mark.parametrize("acts", [TANH, GELU], ids=["tanh", "gelu"])
def test_route_of_a_chain_with_another_activation(acts):
    fixed = 1000 * 24 * 4 + 2 * 24 * 68 * 40 * 4                    # the per-edge dx rows, P and dP (KP = 68)
    route = lambda free, mode: ops.any_width_route(*ROUTE_ARGS, free, mode=mode, dims=DIMS, acts=acts)
    for free in (1 << 40, 2 * BYTES_M):                              # the per-edge weights fit
        assert route(free, "streamed")["route"] == "streamed"
        for mode in ("auto", "on", "off"):
            assert route(free, mode)["route"] == "materialised", (free, mode)
    r = route(2 * BYTES_M - 1, "auto")                               # they do not: auto streams what it refused before
    assert r["route"] == "streamed" and not r["eligible"] and r["eligible_streamed"] and r["bytes_reassociated"] is None
    assert route(2 * BYTES_M - 1, "streamed")["route"] == "streamed"
    assert route(2 * BYTES_M - 1, "on")["route"] == "refused" and route(2 * BYTES_M - 1, "off")["route"] == "refused"
    # bytes_streamed: what the ReLU chain's route holds, plus the U_l rows of a block (only for a kind that keeps them)
    extra = 1000 * (36 + 68) * 4 if acts is GELU else 0
    assert r["bytes_streamed"] == fixed + extra
    assert route(2 * r["bytes_streamed"], "auto")["route"] == "streamed" and route(2 * r["bytes_streamed"] - 1, "auto")["route"] == "refused"
    # not streamable: aggr='max', a chain the library does not generate
    for kw in (dict(aggr="max"), dict(dims=[65, 33, 65, 960])):
        a = dict(n_nodes=100, n_edges=1000, in_channels=24, out_channels=40, k_hidden=65, aggr="mean", chain=True, free_bytes=1000, dims=DIMS, acts=acts)
        a.update(kw)
        for mode in ("streamed", "auto", "on", "off"):
            assert ops.any_width_route(mode=mode, **a)["route"] == "refused", (kw, mode)
        a["free_bytes"] = 1 << 40
        assert ops.any_width_route(mode="streamed", **a)["route"] == "materialised", kw


def test_route_of_a_relu_chain_does_not_depend_on_acts():
    relu = [(ops.ACT_RELU, 0.0, 0.0)] * 2
    for mode in ("streamed", "auto", "on", "off"):
        for free in (1 << 40, 955_200, 1000):
            assert ops.any_width_route(*ROUTE_ARGS, free, mode=mode, dims=DIMS, acts=relu) == ops.any_width_route(*ROUTE_ARGS, free, mode=mode, dims=DIMS)


# ---- the plan and the size query -----------------------------------------------------------------------------------------------------------
DEGREES = [5, 0, 17, 33, 1, 64, 0, 9, 130, 2]


def _arrays(kinds, params=None):
    n = len(kinds)
    params = [0.0] * (2 * n) if params is None else params
    return (ctypes.c_int32 * n)(*kinds), (ctypes.c_float * (2 * n))(*params)


def _plan_act(kinds, budget, params=None, dims=DIMS, degrees=DEGREES, widths=WIDTHS):
    rp = torch.zeros(len(degrees) + 1, dtype=torch.int32)
    rp[1:] = torch.tensor(degrees, dtype=torch.int64).cumsum(0).to(torch.int32)
    n, e = len(degrees), int(rp[-1])
    table = torch.full((n + 1, 2), -7, dtype=torch.int32)
    nb, wf, wb = ctypes.c_int64(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
    k, p = _arrays(kinds, params)
    rc = _lib.lib().gpde_nnconv_chain_act_plan(rp.data_ptr(), n, e, len(dims) - 1, _lib.dims_array(dims), k, p, *widths, budget, table.data_ptr(),
                                               ctypes.byref(nb), ctypes.byref(wf), ctypes.byref(wb))
    return rc, table[:max(nb.value, 0) + 1].tolist(), nb.value, wf.value, wb.value, rp


def _plan_any(budget, dims=DIMS, degrees=DEGREES, widths=WIDTHS):
    rp = torch.zeros(len(degrees) + 1, dtype=torch.int32)
    rp[1:] = torch.tensor(degrees, dtype=torch.int64).cumsum(0).to(torch.int32)
    n, e = len(degrees), int(rp[-1])
    table = torch.full((n + 1, 2), -7, dtype=torch.int32)
    nb, wf, wb = ctypes.c_int64(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = _lib.lib().gpde_nnconv_chain_any_plan(rp.data_ptr(), n, e, len(dims) - 1, _lib.dims_array(dims), *widths, budget, table.data_ptr(),
                                               ctypes.byref(nb), ctypes.byref(wf), ctypes.byref(wb))
    return rc, table[:max(nb.value, 0) + 1].tolist(), nb.value, wf.value, wb.value, rp


def test_header_binding_and_library_have_the_entry_points():
    protos = _lib.header_prototypes()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("gpde_")}
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES and name in exported, name
        old = protos[name.replace("_act", "_any")][1]
        dims_at = next(i for i in range(1, len(old)) if old[i] == "const int32_t*" and old[i - 1] == "int")      # `dims` follows `int n_linear`
        # argument for argument the `_chain_any` prototype, the two host arrays right after `dims`
        assert protos[name][1] == old[:dims_at + 1] + ["const int32_t*", "const float*"] + old[dims_at + 1:], name
    assert all(f"#define GPDE_ACT_{k.upper()} {v}" in open(_lib.HEADER_PATH).read() for k, v in KINDS.items())
    assert ops.ACT_NAMES == tuple(KINDS) and ops.ACT_FROM_U == {KINDS[k] for k in FROM_U}


@pytest.mark.parametrize("budget", [1, 40 * 1000, 1 << 30])
def test_all_relu_acts_give_the_numbers_of_the_chain_any_plan(budget):
    want = _plan_any(budget)
    got = _plan_act([ops.ACT_RELU] * 2, budget)
    assert want[0] == got[0] == 0 and want[1:5] == got[1:5]
    lib = _lib.lib()
    nb, wf, wb = ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_size_t()      # NULL arrays: all RELU too
    assert lib.gpde_nnconv_chain_act_plan(want[5].data_ptr(), len(DEGREES), sum(DEGREES), 3, _lib.dims_array(DIMS), None, None, *WIDTHS, budget,
                                          None, ctypes.byref(nb), ctypes.byref(wf), ctypes.byref(wb)) == 0
    assert (nb.value, wf.value, wb.value) == want[2:5]


def test_workspaces_by_kind():
    """One block (a budget above everything): ws_fwd does not depend on the kinds; ws_bwd of a kind whose derivative comes from h is
    the ReLU chain's; of one that needs u it grows by at least max_block_edges * sum KP_l * 4."""
    _, table, nb, wf0, wb0, _ = _plan_any(1 << 30)
    assert nb == 1
    e, sum_kp = sum(DEGREES), 36 + 68
    for name, kind in KINDS.items():
        p = [0.1, 0.0] * 2 if name == "leaky_relu" else [1.0, 0.0] * 2 if name == "elu" else None
        rc, t, nb, wf, wb, _ = _plan_act([kind] * 2, 1 << 30, p)
        assert rc == 0 and t == table and wf == wf0, name
        if name in FROM_U:
            assert wb >= wb0 + e * sum_kp * 4, (name, wb, wb0)
        else:
            assert wb == wb0, (name, wb, wb0)
        f, b = ctypes.c_size_t(), ctypes.c_size_t()
        k, pp = _arrays([kind] * 2, p)
        tt = torch.tensor(t, dtype=torch.int32)
        assert _lib.lib().gpde_nnconv_chain_act_workspace_bytes(tt.data_ptr(), nb, len(DEGREES), e, 3, _lib.dims_array(DIMS), k, pp, *WIDTHS,
                                                                ctypes.byref(f), ctypes.byref(b)) == 0
        assert (f.value, b.value) == (wf, wb), name
    # a mixed chain keeps U only where it is needed
    rc, _, _, wf, wb, _ = _plan_act([ops.ACT_TANH, ops.ACT_SILU], 1 << 30)
    assert rc == 0 and wf == wf0 and wb0 + e * 68 * 4 <= wb < wb0 + e * sum_kp * 4


def test_forward_workspace_where_the_node_sub_block_is_cut_by_the_row_bytes():
    """N = 1000, E = 25,000, 128 -> 128, [6, 32, 64, 16384] in one block: Z' of all nodes (1000 x 128 x 68 x 4 B) is larger than the
    block's hidden rows, so the node sub-block is sized by the per-edge bytes - by those of the ReLU chain for every kind: ws_fwd is
    one number, ws_bwd of a from-h kind is the ReLU chain's, of a from-u kind larger by exactly its U_l rows (256-byte aligned)."""
    dims, widths, degrees = [6, 32, 64, 128 * 128], (128, 128, 128), [25] * 1000
    e = sum(degrees)
    assert e * ops.chain_edge_bytes(dims) < 1000 * 128 * 68 * 4                    # the sub-block is not all nodes
    rc, table, nb, wf0, wb0, _ = _plan_any(1 << 40, dims=dims, degrees=degrees, widths=widths)
    assert rc == 0 and nb == 1
    for name, kind in KINDS.items():
        p = [0.1, 0.0] * 2 if name == "leaky_relu" else [1.0, 0.0] * 2 if name == "elu" else None
        rc, t, nb, wf, wb, _ = _plan_act([kind] * 2, 1 << 40, p, dims=dims, degrees=degrees, widths=widths)
        assert rc == 0 and t == table and wf == wf0, (name, wf, wf0)
        assert wb == (wb0 + e * (32 + 64) * 4 if name in FROM_U else wb0), (name, wb, wb0)
    # ... and so does a smaller sub-block of a budget-cut table: every kind under ITS OWN plan
    for name in ("tanh", "gelu"):
        rc, t, nb, wf, wb, _ = _plan_act([KINDS[name]] * 2, 1 << 20, dims=dims, degrees=degrees, widths=widths)
        tt, f, b = torch.tensor(t, dtype=torch.int32), ctypes.c_size_t(), ctypes.c_size_t()
        assert _lib.lib().gpde_nnconv_chain_any_workspace_bytes(tt.data_ptr(), nb, 1000, e, 3, _lib.dims_array(dims), *widths, ctypes.byref(f),
                                                                ctypes.byref(b)) == 0
        assert rc == 0 and f.value == wf, (name, wf, f.value)                        # the ReLU chain's forward size for the same table


def test_the_budget_is_spent_on_the_pre_activations_too():
    """Under one budget a GELU chain has fewer edges per block than the ReLU chain: its rows are (sum KP) * 4 bytes larger."""
    per_relu = ops.chain_edge_bytes(DIMS)
    per_gelu = ops.chain_edge_bytes(DIMS, [(ops.ACT_GELU, 0.0, 0.0)] * 2)
    assert per_relu == (36 + 68 + 68 + 2 * 68) * 4 and per_gelu == per_relu + (36 + 68) * 4
    assert ops.chain_edge_bytes(DIMS, [(ops.ACT_TANH, 0.0, 0.0)] * 2) == per_relu
    degrees = [10] * 12
    budget = 30 * per_relu                                            # 3 nodes of the ReLU chain per block, 2 of the GELU chain
    assert _plan_any(budget, degrees=degrees)[2] == 4
    assert _plan_act([ops.ACT_TANH] * 2, budget, degrees=degrees)[2] == 4
    rc, table, nb, _, _, _ = _plan_act([ops.ACT_GELU] * 2, budget, degrees=degrees)
    assert rc == 0 and nb == 6 and all(b[1] - a[1] == 20 for a, b in zip(table[:-1], table[1:]))


def test_unknown_kinds_and_bad_parameters_are_refused():
    err = lambda: _lib.lib().gpde_last_error().decode()
    assert _plan_act([9, 0], 1 << 20)[0] == EUNSUPPORTED and "activation kind 9" in err()
    assert _plan_act([0, -1], 1 << 20)[0] == EUNSUPPORTED
    assert _plan_act([ops.ACT_LEAKY_RELU, 0], 1 << 20, [-0.1, 0, 0, 0])[0] == EINVAL and "slope" in err()
    assert _plan_act([ops.ACT_LEAKY_RELU, 0], 1 << 20, [0.0, 0, 0, 0])[0] == 0
    assert _plan_act([0, ops.ACT_ELU], 1 << 20, [0, 0, 0.0, 0])[0] == EINVAL and "alpha" in err()
    assert _plan_act([0, ops.ACT_ELU], 1 << 20, [0, 0, -1.0, 0])[0] == EINVAL
    for bad in (float("nan"), float("inf")):
        assert _plan_act([ops.ACT_LEAKY_RELU, 0], 1 << 20, [bad, 0, 0, 0])[0] == EINVAL
        assert _plan_act([ops.ACT_ELU, 0], 1 << 20, [bad, 0, 0, 0])[0] == EINVAL
        assert _plan_act([ops.ACT_TANH, 0], 1 << 20, [0, bad, 0, 0])[0] == EINVAL and "non-finite" in err()
    # the two entry points refuse the same before any device work (null device pointers)
    lib, t, w = _lib.lib(), torch.tensor([[0, 0], [2, 3], [3, 4]], dtype=torch.int32), (ctypes.c_void_p * 3)()
    for kinds, params, want in (([9, 0], None, EUNSUPPORTED), ([ops.ACT_LEAKY_RELU, 0], [-0.5, 0, 0, 0], EINVAL)):
        k, p = _arrays(kinds, params)
        assert lib.gpde_nnconv_fwd_chain_act(None, 3, None, 3, 1, None, 4, None, None, 3, _lib.dims_array(DIMS), k, p, w, None, None, None,
                                             _lib.GPDE_AGGR_MEAN, *WIDTHS, t.data_ptr(), 2, None, None, None, 0, None) == want
        assert lib.gpde_nnconv_bwd_chain_act(None, 3, None, 3, 1, None, 4, None, None, 3, _lib.dims_array(DIMS), k, p, w, None, None,
                                             _lib.GPDE_AGGR_MEAN, *WIDTHS, None, None, None, None, None, None, None, None, None, None,
                                             t.data_ptr(), 2, None, None, 0, None) == want
    k, p = _arrays([ops.ACT_GELU, ops.ACT_SIN])
    assert lib.gpde_nnconv_fwd_chain_act(None, 3, None, 3, 1, None, 4, None, None, 3, _lib.dims_array(DIMS), k, p, w, None, None, None,
                                         _lib.GPDE_AGGR_MEAN, *WIDTHS, t.data_ptr(), 2, None, None, None, 0, None) == -3      # GPDE_EWORKSPACE
    assert "gpde_nnconv_chain_act_plan" in err()


def test_host_wrappers_key_their_plans_by_acts():
    rp = torch.tensor([0] + torch.tensor(DEGREES).cumsum(0).tolist(), dtype=torch.int32)
    none = torch.empty(0, dtype=torch.int32)
    csr = ops.Csr(len(DEGREES), sum(DEGREES), rp, none, none, none, _rowptr_host=rp)          # (host tensors: the plan reads rowptr_host only)
    gelu_acts = [(ops.ACT_GELU, 0.0, 0.0)] * 2
    relu = ops.chain_any_blocks(csr, DIMS, *WIDTHS, budget_bytes=1 << 30)
    gelu = ops.chain_any_blocks(csr, DIMS, *WIDTHS, budget_bytes=1 << 30, acts=gelu_acts)
    assert ops.chain_any_blocks(csr, DIMS, *WIDTHS, budget_bytes=1 << 30, acts=[(ops.ACT_RELU, 0.0, 0.0)] * 2) is relu      # one key, one entry point
    assert ops.chain_any_blocks(csr, DIMS, *WIDTHS, budget_bytes=1 << 30, acts=gelu_acts) is gelu and gelu is not relu
    assert gelu.ws_bwd >= relu.ws_bwd + sum(DEGREES) * (36 + 68) * 4 and gelu.ws_fwd == relu.ws_fwd
    by_table = ops.chain_any_table(gelu.table, len(DEGREES), sum(DEGREES), DIMS, *WIDTHS, acts=gelu_acts)
    assert (by_table.ws_fwd, by_table.ws_bwd) == (gelu.ws_fwd, gelu.ws_bwd)
    with pytest.raises(ValueError, match="one .kind, p0, p1. per hidden layer"):
        ops.chain_any_blocks(csr, DIMS, *WIDTHS, budget_bytes=1 << 30, acts=gelu_acts[:1])
