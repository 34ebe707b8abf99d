"""Host tier of the k-nearest-neighbour graphs (graph_pde_amd.neighbor_graph, gpde_knn_csr; DESIGN.md §6e "The nearest arm"): the
ABI additions, every refusal that needs no device, the k_eff / rowptr arithmetic, and the oracle of the GPU tier on inputs
whose answer is known by hand."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, neighbor_graph as ng, ops
from tests.helpers import knn_oracle as ko

ENTRY_POINTS = ("gpde_knn_csr_workspace_bytes", "gpde_knn_csr")


def test_the_entry_points_are_in_the_header_the_binding_and_the_library():
    protos = _lib.header_prototypes()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ENTRY_POINTS:
        assert name in protos and name in _lib.SIGNATURES and name in exported, name
        assert hasattr(_lib.lib(), name)
    assert protos["gpde_knn_csr_workspace_bytes"] == ("size_t", ["int64_t", "int64_t", "int", "int64_t", "double", "const double*", "const double*"])
    assert protos["gpde_knn_csr"][1] == ["const double*", "int64_t", "const double*", "int64_t", "int", "int64_t", "int", "double", "const double*",
                                         "const double*", "int32_t*", "int32_t*", "int32_t*", "float*", "void*", "size_t", "void*"]
    header = open(_lib.HEADER_PATH).read()
    assert "#define GPDE_KNN_MAX_K 256" in header and ng.MAX_K == 256
    assert _lib.lib().gpde_version() == 101


def test_the_module_is_exported():
    assert gp.neighbor_graph is ng and "neighbor_graph" in gp.__all__
    assert sorted(ng.__all__) == ["knn_csr", "knn_graph"]
    for name in ng.__all__:
        assert not hasattr(ops, name), "the nearest-neighbour builders live in neighbor_graph.py, not in ops.py"


BUILDERS = (ng.knn_csr, ng.knn_graph)


@pytest.mark.parametrize("fn", BUILDERS, ids=lambda f: f.__name__)
def test_every_value_error_is_raised_without_a_device(fn):
    pos = torch.rand(10, 2, dtype=torch.float64)                     # CPU tensors: a refusal never reaches the device
    for k in (0, -1, 257, 1 << 40, 2.0, None, "3", True):
        with pytest.raises(ValueError, match="k must be"):
            fn(pos, k)
    for loop in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="loop"):
            fn(pos, 3, loop=loop)
    with pytest.raises(ValueError, match="loop=True with pos_dst"):
        fn(pos, 3, pos_dst=torch.rand(4, 2), loop=True)
    for bad in (torch.rand(10, 4), torch.rand(10, 0), torch.rand(2, 3, 4)):
        with pytest.raises(ValueError, match="dim"):
            fn(bad, 3)
    with pytest.raises(ValueError, match="same dimension"):
        fn(pos, 3, pos_dst=torch.rand(5, 3))
    with pytest.raises(ValueError, match="same dimension"):
        fn(pos, 3, pos_dst=torch.rand(5))
    for cell in (0.0, -0.5, float("nan"), float("inf"), 1e-320, "1", True):
        with pytest.raises(ValueError, match="cell_size"):
            fn(pos, 3, cell_size=cell)
    nan, inf = float("nan"), float("inf")
    for bounds in (0.5, (0.0,), (0.0, 1.0, 2.0), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0), (1.0,)), (1.0, 0.0), ((0.0, 1.0), (1.0, 0.5)),
                   (nan, 1.0), (0.0, inf), (-inf, 0.0), (-1e308, 1e308), ("a", "b"), (None, 1.0)):
        with pytest.raises(ValueError, match="bounds"):
            fn(pos, 3, bounds=bounds)
    # everything in order (a box without extent included): the refusal of a CPU tensor, in the other builders' words
    for kw in (dict(), dict(loop=True), dict(bounds=(0.0, 1.0)), dict(bounds=((0.0, 0.5), (1.0, 0.5))), dict(cell_size=0.1),
               dict(pos_dst=torch.rand(4, 2, dtype=torch.float64)), dict(bounds=(torch.zeros(2), torch.ones(2)))):
        with pytest.raises(RuntimeError, match="no CPU / composite fallback exists by design"):
            fn(pos, 3, **kw)
    with pytest.raises(RuntimeError) as a:
        fn(pos, 3)
    with pytest.raises(RuntimeError) as b:
        ops.radius_csr(pos, 0.1)
    assert str(a.value) == str(b.value)


def test_the_int32_edge_limit_is_a_host_refusal():
    pos = torch.rand(300, 2, dtype=torch.float64)
    pd = torch.empty((1 << 24, 2), dtype=torch.float64, device="meta")        # 2^24 destinations x 256 = 2^32 edges, without the memory
    with pytest.raises(ValueError, match="int32 CSR"):
        ng.knn_csr(pos, 256, pos_dst=pd)
    with pytest.raises(ValueError, match="int32 CSR"):
        ng.knn_graph(pos, 256, pos_dst=pd)


def test_k_eff_and_rowptr_arithmetic():
    for n in (0, 1, 2, 5, 300):
        for k in (1, 2, 5, 256):
            assert ng.k_eff(k, n, True, False) == max(0, min(k, n - 1)) == ko.k_eff(k, n, True, False)
            assert ng.k_eff(k, n, True, True) == min(k, n) == ko.k_eff(k, n, True, True)
            assert ng.k_eff(k, n, False, False) == min(k, n) == ko.k_eff(k, n, False, False)
    # the oracle's rows: every one k_eff long, rowptr[i] = i * k_eff, sources ascending
    for name, k, loop in (("n5", 9, False), ("n5", 9, True), ("two_sets", 200, False), ("duplicates", 16, False)):
        c = ko.CASES[name]()
        rowptr, src, dst = ko.oracle(c["xs"], k, c.get("xd"), loop)
        n_dst = len(c["xd"]) if "xd" in c else len(c["xs"])
        ke = ko.k_eff(k, len(c["xs"]), "xd" not in c, loop)
        assert np.array_equal(rowptr, np.arange(n_dst + 1) * ke) and len(src) == len(dst) == n_dst * ke
        rows = src.reshape(n_dst, ke)
        assert (np.diff(rows, axis=1) > 0).all() and np.array_equal(dst.reshape(n_dst, ke), np.repeat(np.arange(n_dst)[:, None], ke, axis=1))


def test_the_oracle_on_inputs_known_by_hand():
    # the 9 x 9 lattice: the centre point (4, 4) = id 40, ids row-major (i * 9 + j)
    xs = ko.lattice9()
    nb = lambda k, loop=False: ko.oracle(xs, k, loop=loop)[1].reshape(81, -1)[40].tolist()
    assert nb(4) == [31, 39, 41, 49]                                 # the 4 axis neighbours
    assert nb(8) == [30, 31, 32, 39, 41, 48, 49, 50]                 # + the 4 diagonal ones
    assert nb(1) == [31] and nb(5) == [30, 31, 39, 41, 49]           # ties go to the smaller source id
    assert nb(1, True) == [40] and nb(5, True) == [31, 39, 40, 41, 49]
    assert nb(80) == [j for j in range(81) if j != 40] and nb(100, True) == list(range(81))
    # duplicates: a copy at distance 0 is kept, the point itself is not
    xs = ko.CASES["duplicates"]()["xs"]
    copies = [i for i in range(36) if (xs[i] == xs[np.argmax((xs[:, None] == xs[None]).all(-1).sum(1))]).all()]
    assert len(copies) == 16
    rows = ko.oracle(xs, 15)[1].reshape(36, 15)
    for i in copies:
        assert rows[i].tolist() == [j for j in copies if j != i]
    rows = ko.oracle(xs, 3)[1].reshape(36, 3)
    for i in copies:
        assert rows[i].tolist() == [j for j in copies if j != i][:3]
    # two_sets_bounds: the caller's box cuts off about a third of each set
    c = ko.CASES["two_sets_bounds"]()
    lo, hi = np.array(c["bounds"][0]), np.array(c["bounds"][1])
    for pts in (c["xs"], c["xd"]):
        outside = ((pts < lo) | (pts > hi)).any(axis=1).mean()
        assert 0.2 < outside < 0.45
    c = ko.CASES["two_sets_far"]()
    assert (c["xd"].min(axis=1) > 30.0).sum() == 10 and c["xs"].max() < 1.0


def _args(dim=2):
    D = ctypes.c_double * dim
    return dict(D=D, lo=D(*[0.0] * dim), hi=D(*[1.0] * dim))


def test_the_library_refuses_bad_arguments_before_any_device_call():
    l = _lib.lib()
    a = _args()
    D = a["D"]
    q = l.gpde_knn_csr_workspace_bytes
    assert q(58081, 58081, 2, 16, 0.0, a["lo"], a["hi"]) > 4 * 4 * 58081
    assert q(100, 100, 2, 16, 1e-12, a["lo"], a["hi"]) < 1 << 28              # an absurdly fine grid is coarsened
    assert q(0, 0, 1, 1, 0.0, a["lo"], a["hi"]) > 0                            # zero points: a valid query
    assert q(100, 100, 2, 16, 0.0, D(0.5, 0.5), D(0.5, 0.5)) > 0               # a box without extent is not empty
    nan, inf = float("nan"), float("inf")
    for bad in (dict(ns=-1), dict(nd=-1), dict(ns=1 << 31), dict(dim=0), dict(dim=4), dict(k=0), dict(k=257), dict(k=-3), dict(cell=-1.0),
                dict(cell=nan), dict(cell=inf), dict(cell=1e-320), dict(lo=None), dict(hi=None), dict(lo=D(0.0, 2.0)), dict(hi=D(nan, 1.0)),
                dict(lo=D(-inf, 0.0)), dict(hi=D(inf, 1.0)), dict(lo=D(-1e308, 0.0), hi=D(1e308, 1.0)), dict(nd=1 << 24, k=256, ns=300)):
        v = dict(ns=100, nd=100, dim=2, k=16, cell=0.0, lo=a["lo"], hi=a["hi"])
        v.update(bad)
        assert q(v["ns"], v["nd"], v["dim"], v["k"], v["cell"], v["lo"], v["hi"]) == 0, bad
        assert l.gpde_last_error(), bad

    # gpde_knn_csr: a fake non-null "device" address is never dereferenced - every call below returns before a device call
    P, ws = 0x1000, 1 << 20

    def knn(ps=P, ns=8, pd=0x2000, nd=8, dim=2, k=3, loop=0, cell=0.0, lo=a["lo"], hi=a["hi"], rowptr=P, src=P, dst=P, geom=None, w=P, wb=ws):
        return l.gpde_knn_csr(ps, ns, pd, nd, dim, k, loop, cell, lo, hi, rowptr, src, dst, geom, w, wb, None)

    for bad in (dict(ps=None), dict(pd=None), dict(ns=-1), dict(nd=-1), dict(ns=1 << 31), dict(nd=1 << 31), dict(k=0), dict(k=257), dict(loop=2),
                dict(loop=-1), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(lo=None), dict(hi=None), dict(lo=D(0.0, 2.0)),
                dict(hi=D(0.0, nan)), dict(hi=D(inf, 1.0)), dict(rowptr=None), dict(src=None), dict(dst=None), dict(w=None),
                dict(nd=1 << 24, k=256, ns=300)):
        assert knn(**bad) == -1, bad
        assert l.gpde_last_error(), bad
    assert knn(dim=0) == -2 and knn(dim=4) == -2                     # GPDE_EUNSUPPORTED
    assert b"dim" in l.gpde_last_error()
    assert knn(wb=16) == -3                                          # GPDE_EWORKSPACE
    assert knn(k=257) == -1 and b"GPDE_KNN_MAX_K" in l.gpde_last_error()
