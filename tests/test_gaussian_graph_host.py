"""Host tier of the sampled graphs (graph_pde_amd.sampled_graph, gpde_gaussian_csr_*; DESIGN.md §6e "The sampled arm"): the ABI
additions, every refusal that needs no device, and the float64 oracle's own graphs on the fixed inputs of
tests/helpers/gaussian_oracle.py - no undecided pair on any of them, and the statistics the definition has to meet."""
import ctypes
import math
import subprocess

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, ops, sampled_graph as sg
from tests.helpers import gaussian_oracle as go

ENTRY_POINTS = ("gpde_gaussian_csr_workspace_bytes", "gpde_gaussian_csr_count", "gpde_gaussian_csr_fill")
ALL_INPUTS = list(go.CASES) + [str(n) for n in go.LONG_ROWS]


def test_the_entry_points_are_in_the_header_the_binding_and_the_library():
    protos = _lib.header_prototypes()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ENTRY_POINTS:
        assert name in protos and name in _lib.SIGNATURES and name in exported, name
        assert hasattr(_lib.lib(), name)
    assert protos["gpde_gaussian_csr_workspace_bytes"][0] == "size_t"
    assert len(protos["gpde_gaussian_csr_fill"][1]) == len(protos["gpde_gaussian_csr_count"][1]) + 5      # rowptr for deg; src, dst, geom, n_edges, max_in_degree
    assert _lib.lib().gpde_version() == 101


def test_the_module_is_exported():
    assert gp.sampled_graph is sg and "sampled_graph" in gp.__all__
    assert sorted(sg.__all__) == ["gaussian_csr", "gaussian_graph", "gaussian_in_degrees", "gaussian_support_radius"]
    for name in sg.__all__:
        assert not hasattr(ops, name), "the sampled-graph functions live in sampled_graph.py, not in ops.py"


BUILDERS = (sg.gaussian_csr, sg.gaussian_graph, sg.gaussian_in_degrees)


@pytest.mark.parametrize("fn", BUILDERS, ids=lambda f: f.__name__)
def test_every_value_error_is_raised_without_a_device(fn):
    pos = torch.rand(10, 2, dtype=torch.float64)                     # CPU tensors: a refusal never reaches the device
    for sigma in (0.0, -1.0, float("nan"), float("inf"), None, "0.1", True, 1e-170, 1e170):
        with pytest.raises(ValueError, match="sigma"):
            fn(pos, sigma)
    for cutoff in (0.0, -0.5, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="cutoff"):
            fn(pos, 0.1, cutoff=cutoff)
    for bad in (torch.rand(10, 4), torch.rand(10, 0), torch.rand(2, 3, 4)):
        with pytest.raises(ValueError, match="dim"):
            fn(bad, 0.1)
    with pytest.raises(ValueError, match="same dimension"):
        fn(pos, 0.1, pos_dst=torch.rand(5, 3))
    with pytest.raises(ValueError, match="same dimension"):
        fn(pos, 0.1, pos_dst=torch.rand(5))
    for seed in (1 << 63, -(1 << 63) - 1, 1.5, True, None):
        with pytest.raises(ValueError, match="seed"):
            fn(pos, 0.1, seed)
    # the periodic rule: 2 min(r_support, cutoff) < period, and the message says what to do
    with pytest.raises(ValueError, match="cutoff="):
        fn(pos, 0.1, period=1.0)                                     # r_support = 0.61
    with pytest.raises(ValueError, match="cutoff="):
        fn(pos, 0.1, period=(0.0, 1.0))
    with pytest.raises(ValueError, match="cutoff="):
        fn(pos, 0.1, period=1.0, cutoff=0.5)
    with pytest.raises(ValueError, match="period"):
        fn(pos, 0.01, period=-1.0)
    with pytest.raises(ValueError, match="entries"):
        fn(pos, 0.01, period=(1.0, 1.0, 1.0))
    # everything in order: the refusal of a CPU tensor, in the other builders' words
    for kw in (dict(), dict(period=1.0, cutoff=0.4), dict(period=1.0, sigma=0.05)):
        sigma = kw.pop("sigma", 0.1)
        with pytest.raises(RuntimeError, match="no CPU / composite fallback exists by design"):
            fn(pos, sigma, **kw)
    with pytest.raises(RuntimeError) as a:
        fn(pos, 0.1)
    with pytest.raises(RuntimeError) as b:
        ops.radius_csr(pos, 0.1)
    assert str(a.value) == str(b.value)


def test_support_radius():
    for s in (1e-9, 0.1, 1.0, 3e7):
        assert sg.gaussian_support_radius(s) == s * math.sqrt(54.0 * math.log(2.0))
    assert abs(sg.gaussian_support_radius(1.0) - 6.118) < 1e-3
    r = sg.gaussian_support_radius(1.0)
    assert math.exp(-r * r) <= 2.0 ** -54 * (1 + 1e-12) and math.exp(-(r * 0.999) ** 2) > 2.0 ** -54
    for bad in (0.0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError):
            sg.gaussian_support_radius(bad)


def _args(n=8, dim=2, sigma=0.1, cutoff=0.0, period=None):
    D = ctypes.c_double * dim
    return dict(D=D, lo=D(*[0.0] * dim), hi=D(*[1.0] * dim), org=D(*[0.0] * dim), per=None if period is None else D(*period))


def test_the_library_refuses_bad_arguments_before_any_device_call():
    l = _lib.lib()
    a = _args()
    q = l.gpde_gaussian_csr_workspace_bytes
    assert q(58081, 2, 0.1, 0.0, a["lo"], a["hi"], None, None) > 4 * 4 * 58081
    assert q(58081, 2, 0.1, 0.0, a["lo"], a["hi"], a["org"], a["D"](0.0, 0.0)) == q(58081, 2, 0.1, 0.0, a["lo"], a["hi"], None, None)
    assert q(100, 2, 1e-9, 0.0, a["lo"], a["hi"], None, None) < 1 << 28         # an absurdly fine grid is coarsened
    assert q(100, 2, 0.05, 0.0, None, None, a["org"], a["D"](1.0, 1.0)) > 0       # every axis periodic: no bounds needed
    for bad in (dict(n=-1), dict(dim=0), dict(dim=4), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
                dict(sigma=1e-170), dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(cutoff=float("inf")), dict(lo=None), dict(hi=None),
                dict(per=a["D"](1.0, 1.0)), dict(per=a["D"](-1.0, 0.0)), dict(per=a["D"](0.0, float("inf"))),
                dict(per=a["D"](1.0, 1.0), cutoff=0.5), dict(org=a["D"](float("nan"), 0.0), per=a["D"](0.0, 0.0))):
        v = dict(n=100, dim=2, sigma=0.1, cutoff=0.0, lo=a["lo"], hi=a["hi"], org=a["org"], per=None)
        v.update(bad)
        assert q(v["n"], v["dim"], v["sigma"], v["cutoff"], v["lo"], v["hi"], v["org"], v["per"]) == 0, bad
        assert l.gpde_last_error(), bad
    assert q(100, 2, 0.1, 0.0, a["lo"], a["hi"], a["org"], a["D"](1.0, 1.0)) == 0 and b"cutoff" in l.gpde_last_error()

    # count / fill: a fake non-null "device" address is never dereferenced - every call below returns before a device call
    P, ws = 0x1000, 1 << 20

    def count(ps=P, ns=8, pd=P, nd=8, dim=2, sigma=0.1, cutoff=0.0, seed=0, lo=a["lo"], hi=a["hi"], org=None, per=None, deg=P, w=P, wb=ws):
        return l.gpde_gaussian_csr_count(ps, ns, pd, nd, dim, sigma, cutoff, seed, lo, hi, org, per, deg, w, wb, None)

    def fill(ps=P, ns=8, pd=P, nd=8, dim=2, sigma=0.1, cutoff=0.0, seed=0, lo=a["lo"], hi=a["hi"], org=None, per=None, rowptr=P, src=P, dst=P,
             geom=None, e=5, maxdeg=0, w=P, wb=ws):
        return l.gpde_gaussian_csr_fill(ps, ns, pd, nd, dim, sigma, cutoff, seed, lo, hi, org, per, rowptr, src, dst, geom, e, maxdeg, w, wb, None)

    for fn in (count, fill):
        for bad in (dict(ps=None), dict(pd=None), dict(ns=-1), dict(nd=-1), dict(ns=1 << 31), dict(nd=1 << 31), dict(sigma=0.0),
                    dict(sigma=float("nan")), dict(sigma=1e170), dict(cutoff=-2.0), dict(lo=None), dict(w=None),
                    dict(per=a["D"](1.0, 0.0)), dict(per=a["D"](0.0, -3.0))):
            assert fn(**bad) == -1, (fn.__name__, bad)
            assert l.gpde_last_error(), bad
        assert fn(dim=0) == -2 and fn(dim=4) == -2                   # GPDE_EUNSUPPORTED
        assert fn(wb=16) == -3                                       # GPDE_EWORKSPACE
        assert fn(nd=0) == 0                                         # nothing to do: no device call
    assert count(deg=None) == -1
    for bad in (dict(rowptr=None), dict(src=None), dict(dst=None), dict(e=-1), dict(e=(1 << 31) - 64), dict(maxdeg=-1)):
        assert fill(**bad) == -1, bad
    assert fill(e=0, src=None, dst=None) == 0


@pytest.mark.parametrize("name", ALL_INPUTS)
def test_no_fixed_input_has_an_undecided_pair(name):
    c, o = go.cached(name)
    assert int(o["undecided"].sum()) == 0                            # (the budget, 1e-6 of the pairs, means zero at these sizes)
    assert float(o["u"].min()) >= 2.0 ** -54 and float(o["u"].max()) < 1.0
    # no pair is kept beyond the support radius (nor beyond the cutoff)
    reach = c["sigma"] * go.SUPPORT if c.get("cutoff") is None else min(c["sigma"] * go.SUPPORT, c["cutoff"])
    assert not o["keep"][o["d2"] > reach * reach].any()
    if "xd" not in c:
        assert o["keep"].diagonal().all(), "a point with itself: d = 0, p = 1, always kept"


def test_the_inputs_are_what_their_names_say():
    c, o = go.cached("cells_1_63_64_65")
    cells = go.grid_cells(c["xs"], c["sigma"] * go.SUPPORT)
    count = {k: cells.count(k) for k in set(cells)}
    assert count == {**go.CELL_MEMBERS, (0, 0): 1, (4, 4): 1}
    c, o = go.cached("self_loops")
    assert np.array_equal(o["keep"], np.eye(len(c["xs"]), dtype=bool))
    c, o = go.cached("empty")
    assert not o["keep"].any()
    c, o = go.cached("one_cell")
    assert c["sigma"] * go.SUPPORT > 1.5 and 0.3 < o["keep"].mean() < 0.9
    c, o = go.cached("cutoff")
    assert c["cutoff"] < c["sigma"] * go.SUPPORT and o["keep"].sum() < go.outcome(c["xs"], c["sigma"], c["seed"])["keep"].sum()
    c, o = go.cached("lattice16")
    assert len(np.unique(o["d2"])) < 300                             # many equal distances
    for n in go.LONG_ROWS:
        c, o = go.cached(str(n))
        assert o["keep"].shape == (1, n) and o["keep"].all()


def _six_sigma(k, p):
    return abs(k - p.sum()) <= 6.0 * math.sqrt(float((p * (1.0 - p)).sum()))


@pytest.mark.parametrize("name", list(go.CASES))
def test_statistics_of_the_oracles_own_graphs(name):
    """The graph the definition gives is the Gaussian-connectivity graph: edge count, its profile over d / sigma, and the
    independence of the two directions of a pair, each inside 6 standard deviations of its expectation on the fixed seeds."""
    c, o = go.cached(name)
    keep, p = o["keep"], o["p"]
    assert _six_sigma(int(keep.sum()), p), (int(keep.sum()), float(p.sum()))
    t = np.sqrt(o["d2"]) / c["sigma"]
    edges = np.concatenate([np.linspace(0.0, 3.5, 8), [np.inf]])     # 8 bins of d / sigma; the last one is the tail
    for b in range(8):
        m = (t >= edges[b]) & (t < edges[b + 1])
        assert _six_sigma(int(keep[m].sum()), p[m]), (b, int(keep[m].sum()), float(p[m].sum()))
    if "xd" not in c:
        iu = np.triu_indices(len(c["xs"]), k=1)
        both, p2 = keep[iu] & keep.T[iu], p[iu] * p.T[iu]
        assert abs(int(both.sum()) - p2.sum()) <= 6.0 * math.sqrt(float((p2 * (1.0 - p2)).sum())), (int(both.sum()), float(p2.sum()))


def test_the_oracle_hash_is_the_headers():
    u = go.pair_u(5, 3, 77)
    for i in range(3):
        for j in range(5):
            key = go.nc.hash_key_bigint(j, i, 77)
            assert u[i, j] == (float(key >> 10) + 0.5) * 2.0 ** -53  # (a 53-bit integer is an exact float; the sum rounds as numpy's)
