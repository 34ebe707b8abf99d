"""CPU tier of the capped in-degree (ops.select_in_edges and its keys; gpde_csr_select_k, gpde_edge_keys_sqdist,
gpde_edge_keys_hash): every refusal that needs host values only, the native argument checks through the loaded library, the
float -> int64 key map, the checker's hash against big integers, and the FAIRNESS of every periodic "nearest" input the GPU tier
runs (tests/helpers/neighbor_cap.py) - an unfair input fails here, so the GPU tier leaves no case out."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from graph_pde_amd import _lib, ops
from tests.helpers import neighbor_cap as nc


def _cpu_csr(lens=(3, 0, 5), rect=None):
    rowptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    e = int(rowptr[-1])
    z = torch.zeros(e, dtype=torch.int32)
    return ops.Csr(len(lens), e, rowptr, z, z.clone(), torch.arange(e, dtype=torch.int32), n_src_nodes=rect)


# ---- refusals: ValueError before any device is touched (every tensor here is a host tensor) -------------------------------------
@pytest.mark.parametrize("k", [0, -1, True, 2.5, "3", None])
def test_select_refuses_a_bad_k(k):
    with pytest.raises(ValueError, match="k"):
        ops.select_in_edges(_cpu_csr(), k, torch.zeros(8, dtype=torch.int64))


def test_select_refuses_bad_keys_and_graphs():
    csr = _cpu_csr()
    with pytest.raises(ValueError, match=r"key must be a tensor \[8\]"):
        ops.select_in_edges(csr, 2, torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"key must be a tensor \[8\]"):
        ops.select_in_edges(csr, 2, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"key must be a tensor \[8\]"):
        ops.select_in_edges(csr, 2, [0] * 8)
    for dt in (torch.int32, torch.uint8, torch.bool):
        with pytest.raises(ValueError, match="int64 or floating"):
            ops.select_in_edges(csr, 2, torch.zeros(8, dtype=dt))
    with pytest.raises(ValueError, match="ops.Csr"):
        ops.select_in_edges(torch.zeros(2, 8, dtype=torch.int64), 2, torch.zeros(8, dtype=torch.int64))


def test_key_functions_refuse_on_host_values():
    csr = _cpu_csr()
    pos = torch.rand(3, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"pos must be a tensor \[3, dim\]"):
        ops.edge_sqdist_keys(csr, torch.rand(4, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="dimension 4"):
        ops.edge_sqdist_keys(csr, torch.rand(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"pos_dst must be a tensor \[3, dim\]"):
        ops.edge_sqdist_keys(csr, pos, torch.rand(5, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="same dimension"):
        ops.edge_sqdist_keys(csr, pos, torch.rand(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="needs pos_dst"):
        ops.edge_sqdist_keys(_cpu_csr(rect=7), torch.rand(7, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="period has 3 entries"):
        ops.edge_sqdist_keys(csr, pos, period=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match=r"period\[1\]"):
        ops.edge_sqdist_keys(csr, pos, period=(1.0, -1.0))
    with pytest.raises(ValueError, match="ops.Csr"):
        ops.edge_sqdist_keys(None, pos)
    ids = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(ValueError, match="src_ids must be an int32 vector"):
        ops.edge_hash_keys(ids.long(), ids, 0)
    with pytest.raises(ValueError, match="dst_ids must be an int32 vector"):
        ops.edge_hash_keys(ids, ids.view(2, 4), 0)
    with pytest.raises(ValueError, match="must match"):
        ops.edge_hash_keys(ids, ids[:5], 0)
    for seed in (1 << 63, -(1 << 63) - 1, 1.5, True, None):
        with pytest.raises(ValueError, match="seed"):
            ops.edge_hash_keys(ids, ids, seed)


@pytest.mark.parametrize("kw, what", [
    (dict(max_num_neighbors=0), "must be >= 1"),
    (dict(max_num_neighbors=-3), "must be >= 1"),
    (dict(max_num_neighbors=4.0), "int >= 1"),
    (dict(max_num_neighbors=True), "int >= 1"),
    (dict(max_num_neighbors=4, select="farthest"), "select"),
    (dict(select="farthest"), "select"),
    (dict(max_num_neighbors=4, select="random", seed=1 << 63), "seed"),
    (dict(max_num_neighbors=4, seed="0"), "seed"),
    (dict(max_num_neighbors=4, reference_ties=True), "reference_ties"),
])
def test_the_builders_refuse_cap_arguments_without_a_device(kw, what):
    pos = torch.rand(10, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match=what):
        ops.radius_csr(pos, 0.3, **kw)
    with pytest.raises(ValueError, match=what):
        ops.radius_csr_batched(pos, [0, 4, 10], 0.3, **kw)
    if "reference_ties" not in kw:
        with pytest.raises(ValueError, match=what):
            ops.radius_csr(pos, 0.3, period=1.0, return_geometry=True, **kw)


def test_the_cap_arguments_come_after_the_existing_ones_and_default_to_the_uncapped_build():
    p = list(inspect.signature(ops.radius_csr).parameters.values())
    assert [q.name for q in p] == ["pos", "r", "reference_ties", "pos_dst", "period", "origin", "return_geometry", "max_num_neighbors",
                                   "select", "seed"]
    assert [q.default for q in p[-3:]] == [None, "nearest", 0]
    pb = inspect.signature(ops.radius_csr_batched).parameters
    assert [pb[n].default for n in ("max_num_neighbors", "select", "seed")] == [None, "nearest", 0]
    assert all(pb[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("max_num_neighbors", "select", "seed"))
    for fn in (ops.radius_graph, ops.radius_csr_raw, ops.radius_in_degrees, ops.multilevel_radius_graphs, ops.radius_graph_batched):
        assert "max_num_neighbors" not in inspect.signature(fn).parameters, fn.__name__        # out of scope, as the docstrings say


# ---- the three entry points through the loaded library: host-visible errors, no device --------------------------------------
def test_native_argument_checks():
    l = _lib.lib()
    E, U = -1, -2
    rp = (ctypes.c_int32 * 3)(0, 2, 5)                # host memory: these calls must return before anything dereferences it
    rp_p, keys_p, out_p = (ctypes.cast(rp, ctypes.c_void_p).value,) * 3

    def err():
        return l.gpde_last_error().decode()
    # gpde_csr_select_k(rowptr, keys, n_rows, n_edges, k, rowptr_out, slots_out, n_out, stream)
    assert l.gpde_csr_select_k(None, keys_p, 2, 5, 2, rp_p, out_p, 4, None) == E and "null" in err()
    assert l.gpde_csr_select_k(rp_p, None, 2, 5, 2, rp_p, out_p, 4, None) == E and "keys is null" in err()
    assert l.gpde_csr_select_k(rp_p, keys_p, 2, 5, 2, None, out_p, 4, None) == E and "null" in err()
    assert l.gpde_csr_select_k(rp_p, keys_p, 2, 5, 2, rp_p, None, 4, None) == E and "slots_out is null" in err()
    for k in (0, -1):
        assert l.gpde_csr_select_k(rp_p, keys_p, 2, 5, k, rp_p, out_p, 4, None) == E and "must be >= 1" in err()
    assert l.gpde_csr_select_k(rp_p, keys_p, -1, 5, 2, rp_p, out_p, 4, None) == E
    assert l.gpde_csr_select_k(rp_p, keys_p, 2, -5, 2, rp_p, out_p, 4, None) == E
    assert l.gpde_csr_select_k(rp_p, keys_p, 2, 1 << 31, 2, rp_p, out_p, 4, None) == E and "out of range" in err()
    # n_out cannot be the total of the scan of min(deg, k): negative, more than the edges, more than n_rows * k
    for n_out in (-1, 6, 5):
        assert l.gpde_csr_select_k(rp_p, keys_p, 2, 5, 2, rp_p, out_p, n_out, None) == E and "n_out" in err()
    assert l.gpde_csr_select_k(rp_p, keys_p, 0, 5, 2, rp_p, out_p, 0, None) == E and "without rows" in err()
    # zero rows / zero edges: valid calls, nothing is launched
    assert l.gpde_csr_select_k(rp_p, None, 0, 0, 1, rp_p, None, 0, None) == 0
    assert l.gpde_csr_select_k(rp_p, None, 2, 0, 3, rp_p, None, 0, None) == 0
    # gpde_edge_keys_sqdist(pos_src, pos_dst, dim, period, origin, src, dst, n_edges, keys, stream)
    for dim in (0, 4, -1):
        assert l.gpde_edge_keys_sqdist(rp_p, rp_p, dim, None, None, rp_p, rp_p, 3, keys_p, None) == U and "dim must be 1..3" in err()
    for hole in range(5):
        a = [rp_p] * 5
        a[hole] = None
        assert l.gpde_edge_keys_sqdist(a[0], a[1], 2, None, None, a[2], a[3], 3, a[4], None) == E and "null" in err()
    assert l.gpde_edge_keys_sqdist(rp_p, rp_p, 2, None, None, rp_p, rp_p, -3, keys_p, None) == E
    bad = (ctypes.c_double * 2)(1.0, -1.0)
    assert l.gpde_edge_keys_sqdist(rp_p, rp_p, 2, bad, None, rp_p, rp_p, 3, keys_p, None) == E and "period[1]" in err()
    assert l.gpde_edge_keys_sqdist(None, None, 3, None, None, None, None, 0, None, None) == 0
    # gpde_edge_keys_hash(src_ids, dst_ids, n_edges, seed, keys, stream)
    for hole in range(3):
        a = [rp_p] * 3
        a[hole] = None
        assert l.gpde_edge_keys_hash(a[0], a[1], 3, 7, a[2], None) == E and "null" in err()
    assert l.gpde_edge_keys_hash(rp_p, rp_p, -1, 7, keys_p, None) == E
    assert l.gpde_edge_keys_hash(None, None, 0, -1, None, None) == 0
    assert l.gpde_version() == _lib.GPDE_VERSION == 101          # additions: the version stays


# ---- the float -> int64 key map ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16])
def test_float_keys_map_preserves_the_order(dtype):
    fi = torch.finfo(dtype)
    tiny = {torch.float64: 5e-324, torch.float32: 1e-45, torch.float16: 6e-8, torch.bfloat16: 9.2e-41}[dtype]    # smallest subnormal
    vals = [-float("inf"), fi.min, -1.5, -1.0, -fi.tiny, -fi.tiny / 2 if dtype != torch.bfloat16 else -fi.tiny, -tiny, -0.0, 0.0, tiny,
            fi.tiny, 1.0, 1.5, fi.max, float("inf")]
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.tensor(vals, dtype=torch.float64).to(dtype), torch.randn(200, generator=g, dtype=torch.float64).to(dtype),
                   -torch.rand(50, generator=g, dtype=torch.float64).to(dtype) * tiny * 64])
    assert float(v[vals.index(tiny)]) > 0.0 and float(v[vals.index(-tiny)]) < 0.0, "the subnormals must survive the cast"
    m = ops.float_keys_to_int64(v)
    assert m.dtype == torch.int64 and m.shape == v.shape
    a, b = v.double()[:, None], v.double()[None, :]
    assert torch.equal(a < b, m[:, None] < m[None, :])
    assert torch.equal(a == b, m[:, None] == m[None, :])            # -0.0 and +0.0 are one key
    with pytest.raises(ValueError, match="floating"):
        ops.float_keys_to_int64(torch.zeros(3, dtype=torch.int64))


# ---- the checker itself ----------------------------------------------------------------------------------------------------------
def test_the_header_states_the_hash_constants():
    assert nc.header_constants() == (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)


def test_the_helper_hash_is_the_big_integer_evaluation():
    g = np.random.default_rng(5)
    src = np.concatenate([[0, 0, (1 << 31) - 1, (1 << 31) - 1, 1], g.integers(0, 1 << 31, size=300)])
    dst = np.concatenate([[0, (1 << 31) - 1, 0, (1 << 31) - 1, 2], g.integers(0, 1 << 31, size=300)])
    for seed in (0, 1, -1, (1 << 62) + 3, -(1 << 63), (1 << 63) - 1):
        got = nc.hash_keys(src, dst, seed)
        want = [nc.hash_key_bigint(s, d, seed) for s, d in zip(src.tolist(), dst.tolist())]
        assert got.dtype == np.int64 and got.tolist() == want, seed
        assert (got >= 0).all()
    # (dst, src) is ordered, and the seed matters
    assert nc.hash_key_bigint(1, 2, 0) != nc.hash_key_bigint(2, 1, 0) != nc.hash_key_bigint(2, 1, 1)
    # by hand: seed 0, ids 0 -> z = 0 all the way
    assert nc.hash_key_bigint(0, 0, 0) == 0


def test_the_helper_selection_on_a_row_by_hand():
    rowptr = [0, 5, 5, 7]
    key = np.array([3, 1, 3, 0, 1, 9, 9], dtype=np.int64)
    for k, want_ptr, want in ((1, [0, 1, 1, 2], [3, 5]), (2, [0, 2, 2, 4], [1, 3, 5, 6]), (3, [0, 3, 3, 5], [1, 3, 4, 5, 6]),
                              (4, [0, 4, 4, 6], [0, 1, 3, 4, 5, 6]), (5, [0, 5, 5, 7], list(range(7)))):
        ptr, kept = nc.select(rowptr, key, k)
        assert ptr.tolist() == want_ptr and kept.tolist() == want, k
    assert nc.select(rowptr, np.array([0.0, -0.0, -np.inf, np.inf, -1e-45, 2.0, 2.0]), 2)[1].tolist() == [2, 4, 5, 6]


def test_open_d2_of_the_lattice_is_exact_and_tied():
    from tests.helpers import periodic_oracle as po
    lat = po.lattice16()
    ei = nc.brute_open_edges(lat, 0.2)
    d2 = nc.d2_open(lat, None, ei[0], ei[1])
    assert set((d2 * 256).tolist()) == {0.0, 1.0, 2.0, 4.0, 5.0, 8.0, 9.0, 10.0}        # dx^2 + dy^2 <= 0.04 * 256 = 10.24, exactly
    assert (nc.d2_bits(d2) >= 0).all() and np.array_equal(np.argsort(nc.d2_bits(d2), kind="stable"), np.argsort(d2, kind="stable"))


# ---- fairness of every periodic "nearest" input of the GPU tier ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nc.PERIODIC_NEAREST))
def test_periodic_nearest_inputs_are_fair(name):
    c, rowptr, src, dst, d2 = nc.periodic_case(name)
    deg = np.diff(rowptr)
    for k in nc.PERIODIC_NEAREST[name]:
        assert (deg > k).any(), f"{name}: no row is longer than k = {k}: the cap would not be exercised"
        bad = nc.unfair_rows(rowptr, d2, k, c["r"])
        assert not bad, f"{name}, k = {k}: rows {bad[:5]} have their k-th and (k + 1)-th smallest d2 within 1e-12 r^2: not a fair input"


def test_every_periodic_shape_of_the_oracle_is_covered():
    from tests.helpers import periodic_oracle as po
    left_out = set(po.CASES) - set(nc.PERIODIC_NEAREST)
    # one point has no row to cap; the coincident set holds pairs of EQUAL distance by construction (40 points twice): with
    # d2 computed two ways, no cap of it is fair
    assert left_out == {"1d_one_point", "coincident"}
