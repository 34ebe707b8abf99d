"""Expected values for the batched radius-graph builders (ops.radius_csr_batched / radius_graph_batched), from code that is
not under test: per-graph results - of the single-graph builders, or of the CPU oracle - concatenated with their node offsets.
The assembly itself is pinned in the CPU tier (tests/test_batched_graph_host.py) against the oracle and the reference
generator's own multi-level graphs (tests/golden/mgkn_graphs_s20.npz).  numpy only."""
import numpy as np

from oracle import radius_oracle


def concat_sets(sets, dim=None):
    """(pos float64 [n, dim], ptr int64 [B + 1]) of a list of point sets [n_b, dim] (empty sets allowed)."""
    if dim is None:
        dim = next((np.asarray(s).reshape(len(s), -1).shape[1] for s in sets if len(s)), 1)
    sets = [np.asarray(s, dtype=np.float64).reshape(len(s), dim) for s in sets]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    pos = np.concatenate(sets) if sets else np.zeros((0, dim))
    return np.ascontiguousarray(pos.reshape(-1, dim)), ptr


def assemble_csr(per_graph, ptr_src, ptr_dst=None):
    """The block-diagonal destination CSR of per-graph CSRs with LOCAL node ids: per_graph[b] = (rowptr [nd_b + 1], src, dst).
    Returns (rowptr int64 [n_dst + 1], src int64 [E], dst int64 [E], edge_ptr int64 [B + 1]) with global ids: sources offset
    by ptr_src[b], destination rows by ptr_dst[b], slots by the edges of the graphs before."""
    ptr_dst = ptr_src if ptr_dst is None else ptr_dst
    rowptr, src, dst, edge_ptr = [np.zeros(1, dtype=np.int64)], [], [], [0]
    for b, (rp, s, d) in enumerate(per_graph):
        rp, s, d = (np.asarray(v).astype(np.int64) for v in (rp, s, d))
        assert len(rp) == ptr_dst[b + 1] - ptr_dst[b] + 1 and rp[0] == 0 and rp[-1] == len(s) == len(d), b
        rowptr.append(rp[1:] + edge_ptr[-1])
        src.append(s + ptr_src[b])
        dst.append(d + ptr_dst[b])
        edge_ptr.append(edge_ptr[-1] + len(s))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return np.concatenate(rowptr), cat(src), cat(dst), np.asarray(edge_ptr, dtype=np.int64)


def assemble_edge_index(per_graph, ptr_src, ptr_dst=None):
    """(edge_index int64 [2, E], edge_ptr int64 [B + 1]): per-graph edge lists [2, E_b] with local ids, each offset into the
    global numbering, graph after graph - what a DataLoader's collate makes of them."""
    ptr_dst = ptr_src if ptr_dst is None else ptr_dst
    parts = [np.asarray(ei).astype(np.int64) + np.array([[ptr_src[b]], [ptr_dst[b]]], dtype=np.int64) for b, ei in enumerate(per_graph)]
    edge_ptr = np.concatenate([[0], np.cumsum([p.shape[1] for p in parts])]).astype(np.int64)
    return (np.concatenate(parts, axis=1) if parts else np.zeros((2, 0), dtype=np.int64)), edge_ptr


def csr_of_edges(ei, n_dst):
    """Destination CSR (rowptr, src, dst) of a source-major edge list [2, E]: stable sort by destination = rows in ascending
    source order."""
    ei = np.asarray(ei).astype(np.int64)
    order = np.argsort(ei[1], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=n_dst))]).astype(np.int64)
    return rowptr, ei[0][order], ei[1][order]


def split(pos, ptr):
    return [pos[ptr[b]:ptr[b + 1]] for b in range(len(ptr) - 1)]


def oracle_edge_lists(pos, ptr, radii, pos_dst=None, ptr_dst=None, reference_ties=False):
    """Per-graph source-major edge lists (local ids) by the CPU oracle, one call per graph; a graph without sources or
    without destinations has none."""
    out = []
    ss = split(pos, ptr)
    dd = [None] * len(ss) if pos_dst is None else split(pos_dst, ptr_dst)
    for s, d, r in zip(ss, dd, radii):
        if len(s) == 0 or (d is not None and len(d) == 0):
            out.append(np.zeros((2, 0), dtype=np.int64))
        else:
            out.append(radius_oracle.radius_edges(s, float(r), y=d, reference_ties=reference_ties))
    return out


def oracle_csr(pos, ptr, radii, pos_dst=None, ptr_dst=None, reference_ties=False):
    """(rowptr, src, dst, edge_ptr) of the batch by the CPU oracle."""
    lists = oracle_edge_lists(pos, ptr, radii, pos_dst, ptr_dst, reference_ties)
    pd = ptr if ptr_dst is None else ptr_dst
    return assemble_csr([csr_of_edges(ei, int(pd[b + 1] - pd[b])) for b, ei in enumerate(lists)], ptr, ptr_dst)


def unit_box_batch(sizes=(37, 0, 1, 64, 130), dim=2, seed=11):
    """Self graphs that all lie in one unit box (any leak across a graph boundary makes wrong edges); every seventh point on a
    1/8 lattice, so that pairs at exactly representable distances exist."""
    rng = np.random.default_rng(seed)
    sets = []
    for n in sizes:
        p = rng.random((n, dim))
        p[::7] = np.round(p[::7] * 8) / 8
        sets.append(p)
    return concat_sets(sets, dim)
