"""GPU tier: property-based random graphs in EVERY branch of the native backward (bwd_impl, csrc/gpde_bwd.hip).  A regime is
chosen first, then a structure sized so that the library must take it - and the test asserts, chunk by chunk, from the
backward's own trace (_lib.bwd_trace_begin / bwd_trace_end: each field is written where bwd_impl takes that decision) that it did:

  eb1              gpde_edge_bwd_kernel                   mean in-degree < 4 (rows < 4 nn); 2 - 5 Linear layers
  eb3_multi        gpde_edge_bwd3_kernel, groups of 128 slots spanning > 2 destinations (its multi-pass loop): most nodes
                   of in-degree 1 - 2 next to a few heavy ones, mean in-degree >= 4
  zagg32 / zagg16  Z re-aggregated on the fp32 / split-f16 kernel: no kept Z, 3 Linear layers, E below / above 32768
  kept_z, kept_h   Z of the keep-Z forward; plus the last hidden activations kept by the forward (hidden_saved)
  big_chunk        one chunk of >= 8192 rows, k0 <= 7: H_1 generated inside the dW_2 GEMM, dW_1 in the dU_1 GEMM's epilogue,
                   dU_2^T left by the per-edge kernel (du_pre), one attribute bound for the call
  k0_8, wide_k0    k0 == 8 (no call-wide bound, no epilogue dW_1); 9 <= k0 <= 32 (neither first-layer kernel)
  grad_attr        dL/d edge_attr against float64 autograd
  node_table       attributes from a node table (NodeAttr): float64, and bitwise the tensor path
  mixed_chunks     one call with a chunk of >= 8192 rows and a last chunk of < 1024 (in some examples < 64) rows
  big_chunks       two chunks of >= 8192 rows: the second epilogue dW_1 adds to the first
  generic_chunked  2, 4 or 5 Linear layers in >= 2 chunks
  conv_mlp         the split phases: nnconv_backward_hidden_raw (with and without accumulate) + hidden_backward_raw
  light_deferred   L applications: light passes + the deferred pass, with a partial H whose end falls inside the graph
  eb2_forced       gpde_edge_bwd2_kernel, reachable only through GPDE_EDGE_BWD=2 (K2P is a multiple of 128)

Every structure carries duplicate edges, self-loops, nodes without in-edges, an unsorted edge order, add / mean, root and bias
each on or off; edges on the ReLU kink of a hidden layer (tests/helpers/kinks.py) are removed.  Every gradient <= 2e-5 relative
L2 against float64; the chunked regimes also run the same inputs as one chunk: grad_x bitwise (within 5e-6 only where H_1 feeds
the last hidden layer and a chunk formed H_1 on another path than the one-chunk call), weight gradients within 5e-6.
The chunk split of a call is the one ops.bwd_plan gives for its workspace (the test walks the CSR the way bwd_impl does).
GPDE_HYP_EXAMPLES examples per regime (default 3)."""
import collections
import os

import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from graph_pde_amd import _lib, ops
from oracle.nnconv_oracle import nnconv_grads, nnconv_grads_shared, rel_l2
from tests.helpers.bwd_walk import traced as _traced, walk as _walk, ws_for as _ws_for
from tests.helpers.kinks import edges_off_the_kink

pytestmark = pytest.mark.gpu
TOL, TOL_CHUNKS = 2e-5, 5e-6
N_EXAMPLES = int(os.environ.get("GPDE_HYP_EXAMPLES", "3"))
REGIMES = ["eb1", "eb3_multi", "zagg32", "zagg16", "kept_z", "kept_h", "big_chunk", "k0_8", "wide_k0", "grad_attr",
           "node_table", "mixed_chunks", "big_chunks", "generic_chunked", "conv_mlp", "light_deferred", "eb2_forced"]
CHUNKED = ("mixed_chunks", "big_chunks", "generic_chunked")
TAKEN = collections.Counter()
K1_SPLIT, K2_SPLIT = [128, 256, 384], [256, 384]        # widths of the split-f16 backward GEMMs and the fused store kernel
ORACLE_CHUNK = 4096


def _dev():
    return torch.device("cuda:0")


@st.composite
def structures(draw, regime):
    c = {"regime": regime, "aggr": draw(st.sampled_from(["mean", "add"])), "root": draw(st.booleans()),
         "bias": draw(st.booleans()), "dup": draw(st.integers(2, 16)), "loops": draw(st.integers(1, 16)),
         "seed": draw(st.integers(0, 2 ** 31 - 1)), "k0": draw(st.integers(1, 7)), "tail": 0, "shape": "random"}
    split = [draw(st.sampled_from(K1_SPLIT)), draw(st.sampled_from(K2_SPLIT))]
    c["mid"] = split
    if regime == "eb1":
        c["mid"] = [draw(st.integers(16, 320)) for _ in range(draw(st.integers(2, 5)) - 1)]
        c["n"] = draw(st.integers(300, 3000))
        c["e"] = draw(st.integers(c["n"] // 2, 3 * c["n"]))
    elif regime == "eb3_multi":
        c["shape"] = "skew_low"
        c["n"] = draw(st.integers(1500, 4000))
        c["heavy"] = draw(st.integers(3, 6))
        c["e"] = int(draw(st.floats(4.4, 5.0)) * c["n"])
    elif regime in ("zagg32", "kept_z", "kept_h", "node_table", "grad_attr", "k0_8", "eb2_forced"):
        c["n"] = draw(st.integers(50, 1500))
        c["e"] = draw(st.integers(1000, 16000))
        if regime == "k0_8":        # (>= 8192 rows: the split dW_2 GEMM gets an H_1 spec without the call-wide bound)
            c["k0"], c["e"] = 8, draw(st.integers(9500, 16000))
        if regime == "grad_attr":
            c["k0"] = draw(st.integers(1, 8))
        if regime == "eb2_forced":
            c["mid"] = [draw(st.integers(16, 320)), draw(st.integers(16, 320))]
        if regime == "node_table":       # (the node-table backward runs on the one-wave-per-SIMD store kernel: k1 >= 225)
            c["mid"] = [draw(st.sampled_from([256, 384])), split[1]]
    elif regime == "zagg16":
        c["n"] = draw(st.integers(300, 3000))
        c["e"] = draw(st.integers(35500, 42000))
    elif regime == "big_chunk":
        c["e"] = draw(st.integers(9500, 20000))
        c["n"] = draw(st.integers(100, c["e"] // 6))
    elif regime == "wide_k0":
        c["k0"] = draw(st.integers(9, 32))
        c["mid"] = [draw(st.integers(16, 320)), draw(st.integers(16, 320))]
        c["n"] = draw(st.integers(50, 1500))
        c["e"] = draw(st.integers(500, 12000))
    elif regime == "mixed_chunks":
        c["n"] = draw(st.integers(60, 150))
        c["e"] = draw(st.integers(9800, 14000))
        c["tail"] = draw(st.sampled_from([draw(st.integers(12, 60)), draw(st.integers(200, 900))]))
    elif regime == "big_chunks":
        c["n"] = draw(st.integers(100, 250))
        c["e"] = draw(st.integers(19000, 28000))
    elif regime == "generic_chunked":
        c["mid"] = [draw(st.integers(16, 300)) for _ in range(draw(st.sampled_from([2, 4, 5])) - 1)]
        c["n"] = draw(st.integers(50, 400))
        c["e"] = draw(st.integers(3000, 12000))
    elif regime == "conv_mlp":
        c["mid"] = [draw(st.integers(16, 320)), draw(st.integers(16, 320))]
        c["k0"] = draw(st.integers(1, 8))
        c["n"] = draw(st.integers(50, 1500))
        c["e"] = draw(st.integers(500, 12000))
        c["accumulate"] = draw(st.booleans())
    elif regime == "light_deferred":
        c["n"] = draw(st.integers(100, 1500))
        c["e"] = draw(st.integers(2000, 14000))
        c["L"] = draw(st.integers(2, 4))
        c["hfrac"] = draw(st.floats(0.1, 0.9))
    c["n_dst"] = max(2, min(c["n"] - 1, int(draw(st.floats(0.5, 0.95)) * c["n"])))     # the rest: nodes without in-edges
    return c


def _graph(c, g):
    n = c["n"]
    if c["shape"] == "skew_low":
        # ~85 % of the nodes receive 1 or 2 edges, `heavy` nodes the rest: mean in-degree >= 4, CSR groups of many destinations
        nodes = torch.randperm(n, generator=g)
        light = nodes[:int(0.85 * n)]
        heavy = nodes[int(0.85 * n):int(0.85 * n) + c["heavy"]]
        dl = light.repeat_interleave(torch.randint(1, 3, (light.numel(),), generator=g))
        dh = heavy[torch.randint(0, heavy.numel(), (max(0, c["e"] - dl.numel()),), generator=g)]
        dst = torch.cat([dl, dh])
    else:
        hi = n - 1 if c["tail"] else n                   # the tail node n - 1 receives exactly `tail` edges
        targets = torch.randperm(hi, generator=g)[:min(c["n_dst"], hi)]
        dst = targets[torch.randint(0, targets.numel(), (c["e"] - c["tail"],), generator=g)]
        dst = torch.cat([torch.full((c["tail"],), n - 1, dtype=torch.int64), dst])
    e = dst.numel()
    src = torch.randint(0, n, (e,), generator=g)
    lo = c["tail"]
    dup, loops = min(c["dup"], (e - lo) // 4), min(c["loops"], (e - lo) // 4)
    src[lo + 1:lo + 1 + dup], dst[lo + 1:lo + 1 + dup] = src[lo].item(), dst[lo].item()     # `dup` copies of one edge
    src[e - loops:] = dst[e - loops:]                                                         # self-loops
    perm = torch.randperm(e, generator=g)                                                     # unsorted edge order
    return src[perm], dst[perm]


def _params(c, g):
    dims = [c["k0"]] + c["mid"] + [4096]
    W = [torch.empty(dims[i + 1], dims[i]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    B = [torch.empty(dims[i + 1]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    root = torch.empty(64, 64).uniform_(-0.125, 0.125, generator=g) if c["root"] else None
    bias = torch.empty(64).uniform_(-0.125, 0.125, generator=g) if c["bias"] else None
    return dims, W, B, root, bias


def _check_chunks(recs, want, phase):
    got = [(r["na"], r["nb"]) for r in recs if r["phase"] == phase]
    assert got == want, (phase, got, want)


def _max_dst_per_group(dst_csr, e0, rows):
    d = dst_csr[e0:e0 + rows]
    return max((int(torch.unique(d[i:i + 128]).numel()) for i in range(0, rows, 128)), default=0)


def _edge_kernel_ok(r):
    nn, rows = r["nb"] - r["na"], r["rows"]
    if rows == 0:
        return r["edge_kernel"] == 0
    return r["edge_kernel"] == (3 if rows >= 4 * nn else 1)


def _errs(got, ref, names):
    return {k: rel_l2(a.cpu(), b) for k, a, b in zip(names, got, ref) if b is not None}


def _grad_names(nl):
    return ["dx"] + [f"dW{l + 1}" for l in range(nl)] + [f"db{l + 1}" for l in range(nl)] + ["droot", "dbias"]


def _flat(res):
    gx, gW, gb, groot, gbias = res[:5]
    return [gx] + list(gW) + list(gb) + [groot, gbias]


def _run_example(c, monkeypatch):
    d = _dev()
    g = torch.Generator().manual_seed(c["seed"])
    src, dst = _graph(c, g)
    dims, W, B, root, bias = _params(c, g)
    n, r = c["n"], c["regime"]
    if r == "node_table":
        table = torch.randn(n, 3, generator=g)
        sel = [(int(torch.randint(0, 2, (1,), generator=g)), int(torch.randint(0, 3, (1,), generator=g))) for _ in range(c["k0"])]
        ea = torch.stack([table[(dst if ep else src), col] for ep, col in sel], dim=1)
    else:
        ea = torch.randn(src.numel(), c["k0"], generator=g)
    x, gout = torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)
    keep = edges_off_the_kink(ea, W, B) if src.numel() else torch.ones(0, dtype=torch.bool)
    src, dst, ea = src[keep], dst[keep], ea[keep].contiguous()
    ei = torch.stack([src, dst])
    e = src.numel()
    nl = len(W)
    csr = ops.build_csr(ei.to(d), n)
    rowptr = csr.rowptr_host.tolist()
    dst_csr = torch.sort(dst, stable=True).values
    Wd, Bd = [w.to(d) for w in W], [b.to(d) for b in B]
    rootd = None if root is None else root.to(d)
    biasd = None if bias is None else bias.to(d)
    xd, gd, ead = x.to(d), gout.to(d), ea.to(d)
    lib, dims_c = _lib.lib(), _lib.dims_array(dims)
    default_ws = int(lib.gpde_nnconv_bwd_workspace_bytes(n, e, nl, dims_c))
    need_attr = r == "grad_attr"

    if r in ("conv_mlp", "light_deferred"):
        return _run_split(c, d, x, gout, ei, ea, csr, rowptr, dims, W, B, root, bias, g)
    if r == "eb2_forced":
        monkeypatch.setenv("GPDE_EDGE_BWD", "2")

    ws_bytes, ws = default_ws, None
    if r == "mixed_chunks":
        ws_bytes = _ws_for(n, e, dims, rowptr[n - 1])                 # everything but the tail node in the first chunk
    elif r == "big_chunks":
        m = next(i for i in range(n + 1) if rowptr[i] >= e // 2)
        ws_bytes = _ws_for(n, e, dims, rowptr[m])
    elif r == "generic_chunked":
        ws_bytes = _ws_for(n, e, dims, max(e // 3, max(rowptr[i + 1] - rowptr[i] for i in range(n))))
    if r in CHUNKED:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d)
    plan = ops.bwd_plan(n, e, dims, ws_bytes, h_given=r == "kept_h")
    want = _walk(rowptr, plan["edges_per_chunk"], plan["nodes_per_chunk"])

    z = hidden = None
    if r in ("kept_z", "kept_h"):
        pm = ops.pack_mlp(Wd, Bd)
        z = torch.zeros(n, 64 * ops.hidden_width(dims), dtype=torch.float32, device=d)
        ops.nnconv_forward_raw(xd, csr, ead, pm, rootd, biasd, c["aggr"], z_keep=z)
        if r == "kept_h":
            hidden = ops.hidden_forward_raw(csr, ead, pm, Wd, Bd)[0]
    attr_in = ops.NodeAttr(table.to(d), sel) if r == "node_table" else ead
    call = lambda ws_: ops.nnconv_backward_raw(xd, csr, attr_in, Wd, Bd, rootd, c["aggr"], gd, need_bias=bias is not None,
                                               ws=ws_, z_saved=z, need_attr=need_attr, hidden_saved=hidden)
    res, recs = _traced(lambda: call(ws))
    _check_chunks(recs, want, "full")
    assert len(recs) == len(want), recs
    _assert_regime(c, recs, dims, dst_csr)

    ref = nnconv_grads(x, ei, ea, W, B, root, bias, c["aggr"], gout, chunk_edges=ORACLE_CHUNK, need_attr=need_attr)
    errs = _errs(_flat(res), _flat(ref), _grad_names(nl))
    if need_attr:
        errs["dattr"] = rel_l2(res[5].cpu(), ref[5])
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, (c, bad)

    if r == "node_table":        # the tensor the node table describes: the same bits
        tres = ops.nnconv_backward_raw(xd, csr, ead, Wd, Bd, rootd, c["aggr"], gd, need_bias=bias is not None)
        torch.cuda.synchronize()
        for k, p_, q_ in zip(_grad_names(nl), _flat(res), _flat(tres)):
            assert (p_ is None) == (q_ is None) and (p_ is None or torch.equal(p_, q_)), k
    if r in CHUNKED:             # the same inputs as one chunk: grad_x bitwise, the weight gradients to the split-K order
        one_ws = torch.empty(int(lib.gpde_nnconv_bwd_workspace_bytes_one_chunk(n, e, nl, dims_c)), dtype=torch.uint8, device=d)
        one, orecs = _traced(lambda: call(one_ws))
        assert [(q["na"], q["nb"]) for q in orecs] == [(0, n)], orecs
        # per-edge rows, one owner per element, the per-source sums continued chunk after chunk in slot order: the bits.  The one
        # exception: the last hidden layer comes from the layer loop (hlast 'layers') - H_1 then feeds it - and a chunk formed H_1
        # on another path than the one-chunk call (k_first_layer from 1024 rows on, the fp32 GEMM below).  With the fused store
        # kernel (hlast 'store', the 3-Linear split form) H_1 reaches dW_2 / dU_1 only, never grad_x: bitwise whatever the chunks.
        h1_feeds_dx = any(q["hlast"] == "layers" for q in recs + orecs if q["rows"])
        if not h1_feeds_dx or all(q["h1"] == orecs[0]["h1"] for q in recs if q["rows"]):
            assert torch.equal(res[0], one[0]), (c, rel_l2(res[0].cpu(), one[0].cpu()))
        else:
            assert rel_l2(res[0].cpu(), one[0].cpu()) <= TOL_CHUNKS, (c, rel_l2(res[0].cpu(), one[0].cpu()))
        for k, p_, q_ in list(zip(_grad_names(nl), _flat(res), _flat(one)))[1:]:
            if p_ is not None:
                assert rel_l2(p_.cpu(), q_.cpu()) <= TOL_CHUNKS, (c, k, rel_l2(p_.cpu(), q_.cpu()))
    TAKEN[r] += 1


def _assert_regime(c, recs, dims, dst_csr):
    """The branches the regime was drawn for are the ones the trace says ran (per chunk)."""
    r, k0 = c["regime"], dims[0]
    split = len(dims) == 4 and ops.deferred_supported(dims)
    for q in recs:
        rows = q["rows"]
        assert q["ordered"] == (rows > 0), q
        assert q["grad_attr"] == (r == "grad_attr" and rows > 0), q
        if r == "eb2_forced":
            assert q["edge_kernel"] == (2 if rows else 0), q
        else:
            assert _edge_kernel_ok(q), q
        if rows == 0:
            continue
        if r in ("kept_z", "kept_h"):
            assert q["z"] == "kept", q
        elif r == "zagg16":
            assert q["z"] == "zagg16", q
        else:
            assert q["z"] == "zagg32", q
        if r == "kept_h":
            assert q["hlast"] == "given" and q["from_h"] == 1, q
        else:
            assert q["from_h"] == 0, q
            if split and k0 <= 7:
                assert q["hlast"] == "store", q               # the fused store kernel of the 3-Linear split form
            if k0 >= 8:
                assert q["hlast"] == "layers", q              # (no packed MLP image for 8+ attribute slots)
        if split and k0 <= 7:
            assert q["call_amax"] == 1, q
        big = split and rows >= 8192
        if big and k0 <= 7 and r != "grad_attr":
            assert (q["h1"], q["dw1"], q["dw2"], q["du1"]) == ("on_the_fly", "epilogue", "tn_split", "f16s"), q
            assert q["du_pre"] == (q["edge_kernel"] == 3), q
        if split and rows < 8192:
            assert q["dw2"] == "tn_acc" and q["du_pre"] == 0 and q["dw1"] != "epilogue", q
            assert q["du1"] == ("f16s" if rows >= 64 else "f32"), q
            if k0 <= 8:
                assert q["h1"] == ("first_layer" if rows >= 1024 else "gemm"), q
        if r == "k0_8":
            assert q["call_amax"] == 0 and q["dw1"] == ("dw_first" if rows >= 1024 else "tn_acc"), q
            assert q["h1"] == ("first_layer" if rows >= 1024 else "gemm"), q
            assert q["dw2"] == ("tn_split" if rows >= 8192 else "tn_acc"), q
        if r == "wide_k0":
            assert q["call_amax"] == 0 and q["h1"] == "gemm" and q["dw1"] == "tn_acc", q
        if r == "grad_attr":
            assert q["dw1"] in ("dw_first", "tn_acc"), q
        if r == "eb3_multi":
            assert q["edge_kernel"] == 3 and _max_dst_per_group(dst_csr, q["e0"], rows) > 2, (q, c)
        if r == "eb1":
            assert q["edge_kernel"] == 1, q
    if r == "big_chunk":
        assert len(recs) == 1 and recs[0]["rows"] >= 8192 and recs[0]["dw1"] == "epilogue" and recs[0]["du_pre"] == 1, recs
    if r == "mixed_chunks":
        assert len(recs) == 2 and recs[0]["rows"] >= 8192 and recs[-1]["rows"] < 1024, recs
        assert recs[0]["dw1"] == "epilogue" and recs[1]["dw1"] == "tn_acc", recs
        assert recs[1]["du1"] == ("f32" if recs[1]["rows"] < 64 else "f16s"), recs
    if r == "big_chunks":
        assert len(recs) == 2 and all(q["rows"] >= 8192 and q["dw1"] == "epilogue" for q in recs), recs
    if r == "generic_chunked":
        assert len(recs) >= 2, recs
    if r == "k0_8":
        assert any(q["rows"] >= 8192 and (q["dw2"], q["dw1"]) == ("tn_split", "dw_first") for q in recs), recs
    if r == "eb3_multi":
        assert any(q["edge_kernel"] == 3 for q in recs), recs


def _run_split(c, d, x, gout, ei, ea, csr, rowptr, dims, W, B, root, bias, g):
    """conv_mlp: the conv phase (given H, dL/dU out) and the hidden layers' backward; light_deferred: L light passes and one
    deferred pass on a partial H.  Both against float64 autograd of the L applications (nnconv_grads_shared)."""
    r, n, e, nl = c["regime"], c["n"], ei.shape[1], len(W)
    Wd, Bd = [w.to(d) for w in W], [b.to(d) for b in B]
    rootd = None if root is None else root.to(d)
    ead = ea.to(d)
    pm = ops.pack_mlp(Wd, Bd)
    L = c.get("L", 2 if c.get("accumulate") else 1)
    xs = [x] + [torch.randn(n, 64, generator=g) for _ in range(L - 1)]
    gs = [gout] + [torch.randn(n, 64, generator=g) for _ in range(L - 1)]
    H = ops.hidden_forward_raw(csr, ead, pm, Wd, Bd)[0]
    gx, gw, gbl, groot, gbias = [], 0, 0, 0, 0
    if r == "conv_mlp":
        def run():
            nonlocal gw, gbl, groot, gbias
            gh = None
            for l in range(L):
                out = ops.nnconv_backward_hidden_raw(xs[l].to(d), csr, H, dims, Wd[-1], Bd[-1], rootd, c["aggr"], gs[l].to(d),
                                                     need_bias=bias is not None, grad_hidden_acc=gh)
                gh = out[1] if c.get("accumulate") else None
                gx.append(out[0]); gw = gw + out[2]; gbl = gbl + out[3]
                groot = groot + (0 if out[4] is None else out[4]); gbias = gbias + (0 if out[5] is None else out[5])
                if not c.get("accumulate"):
                    last_gh = out[1]
            return ops.hidden_backward_raw(csr, ead, dims, Wd[:-1], Bd[:-1], gh if c.get("accumulate") else last_gh)
        (hW, hb), recs = _traced(run)
        conv = [q for q in recs if q["phase"] == "conv"]
        assert len(conv) == L and all((q["hlast"], q["from_h"], q["z"]) == ("given", 1, "zagg32") for q in conv if q["rows"]), recs
        assert all(_edge_kernel_ok(q) or (c.get("accumulate") and q["edge_kernel"] == 3) for q in conv), recs
        mlp = [q for q in recs if q["phase"] == "mlp"]
        assert mlp and sum(q["rows"] for q in mlp) == e and all(q["hlast"] == "none" for q in mlp), recs
        if c.get("accumulate"):         # the applications after the first ADD their dL/dU: built into the split-f16 kernel only
            assert all(q["edge_kernel"] == 3 for q in conv[1:] if q["rows"]), recs
    else:
        h_nodes = next(i for i in range(1, n) if rowptr[i] >= int(c["hfrac"] * e))
        assert 0 < rowptr[h_nodes] < e
        want = _walk(rowptr, e, n, h_nodes)

        def run():
            nonlocal gw, gbl, groot, gbias
            for l in range(L):
                out = ops.nnconv_backward_light_raw(xs[l].to(d), csr, ead, Wd, Bd, rootd, c["aggr"], gs[l].to(d),
                                                    need_bias=bias is not None, hidden_part=H, hidden_nodes=h_nodes)
                gx.append(out[0]); gw = gw + out[1]; gbl = gbl + out[2]
                groot = groot + (0 if out[3] is None else out[3]); gbias = gbias + (0 if out[4] is None else out[4])
            return ops.nnconv_backward_deferred_raw([t.to(d) for t in xs], [t.to(d) for t in gs], csr, ead, Wd, Bd, c["aggr"],
                                                    hidden_part=H, hidden_nodes=h_nodes)
        (hW, hb), recs = _traced(run)
        light = [q for q in recs if q["phase"] == "light"]
        assert [(q["na"], q["nb"]) for q in light] == want * L, (light, want)
        _check_chunks([q for q in recs if q["phase"] == "deferred"], want, "deferred")
        for q in recs:
            if q["rows"]:
                assert (q["hlast"], q["from_h"]) == (("given", 1) if q["na"] < h_nodes else ("store", 0)), q
        for q in light:
            assert q["z"] == "zagg32" and q["du1"] == "none" and q["dw1"] == "none" and _edge_kernel_ok(q), q
        for q in recs:
            if q["phase"] == "deferred" and q["rows"]:
                assert q["edge_kernel"] == 0 and q["dw2"] != "none" and q["dw1"] != "none", q
    torch.cuda.synchronize()
    rxs, rW, rb, rroot, rbias = nnconv_grads_shared(xs, ei, ea, W, B, root, bias, c["aggr"], gs, chunk_edges=ORACLE_CHUNK)
    errs = {f"dx{l}": rel_l2(gx[l].cpu(), rxs[l]) for l in range(L)}
    errs[f"dW{nl}"], errs[f"db{nl}"] = rel_l2(gw.cpu(), rW[-1]), rel_l2(gbl.cpu(), rb[-1])
    for l in range(nl - 1):
        errs[f"dW{l + 1}"], errs[f"db{l + 1}"] = rel_l2(hW[l].cpu(), rW[l]), rel_l2(hb[l].cpu(), rb[l])
    if root is not None:
        errs["droot"] = rel_l2(groot.cpu(), rroot)
    if bias is not None:
        errs["dbias"] = rel_l2(gbias.cpu(), rbias)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, (c, bad)
    TAKEN[r] += 1


@pytest.mark.parametrize("regime", REGIMES)
@settings(max_examples=N_EXAMPLES, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
@given(data=st.data())
def test_bwd_regime_gradients_vs_float64(regime, data, monkeypatch):
    _run_example(data.draw(structures(regime)), monkeypatch)


def test_every_bwd_regime_drew_its_examples():
    """Each regime ran at least min(3, GPDE_HYP_EXAMPLES) examples to the end (a regime that stops being taken fails its own test
    above; this one fails if a regime's examples stopped being drawn at all)."""
    if not TAKEN:
        pytest.skip("no regime example ran in this process")
    short = {r: TAKEN[r] for r in REGIMES if TAKEN[r] < min(3, N_EXAMPLES)}
    assert not short, short


# ---- edges of the chunk walk ----------------------------------------------------------------------------------------------------

def _small_case(n, src, dst, dims, seed=0):
    g = torch.Generator().manual_seed(seed)
    W = [torch.empty(dims[i + 1], dims[i]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    B = [torch.empty(dims[i + 1]).uniform_(-1, 1, generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    ea = torch.randn(src.numel(), dims[0], generator=g)
    keep = edges_off_the_kink(ea, W, B) if src.numel() else torch.ones(0, dtype=torch.bool)
    ei = torch.stack([src[keep], dst[keep]])
    root, bias = torch.empty(64, 64).uniform_(-0.125, 0.125, generator=g), torch.empty(64).uniform_(-0.125, 0.125, generator=g)
    return ei, ea[keep].contiguous(), W, B, root, bias, torch.randn(n, 64, generator=g), torch.randn(n, 64, generator=g)


@pytest.mark.parametrize("n,e", [(37, 0), (1, 3000)])
def test_bwd_without_edges_and_with_one_node(n, e):
    """E == 0: only the node-side terms (no chunk is walked); n_nodes == 1: every edge is a self-loop of node 0."""
    d = _dev()
    dims = [5, 256, 256, 4096]
    z = torch.zeros(e, dtype=torch.int64)
    ei, ea, W, B, root, bias, x, gout = _small_case(n, z, z, dims)
    csr = ops.build_csr(ei.to(d), n)
    for aggr in ("add", "mean"):
        res, recs = _traced(lambda: ops.nnconv_backward_raw(x.to(d), csr, ea.to(d), [w.to(d) for w in W], [b.to(d) for b in B],
                                                            root.to(d), aggr, gout.to(d)))
        assert [(q["na"], q["nb"], q["rows"]) for q in recs] == ([] if e == 0 else [(0, 1, ei.shape[1])]), recs
        ref = nnconv_grads(x, ei, ea, W, B, root, bias, aggr, gout, chunk_edges=ORACLE_CHUNK)
        errs = _errs(_flat(res), _flat(ref), _grad_names(3))
        assert all(v <= TOL for v in errs.values()), (n, e, aggr, errs)


def test_bwd_refuses_a_node_whose_in_degree_exceeds_the_chunk():
    """A destination with more in-edges than a chunk holds cannot be split: GPDE_EWORKSPACE with the node named, no numbers."""
    d = _dev()
    dims = [6, 256, 256, 4096]
    n, e = 100, 6000
    g = torch.Generator().manual_seed(11)
    dst = torch.randint(0, n, (e,), generator=g)
    dst[:3000] = 7
    src = torch.randint(0, n, (e,), generator=g)
    ei = torch.stack([src, dst])
    csr = ops.build_csr(ei.to(d), n)
    ws_bytes = _ws_for(n, e, dims, 1000)
    assert ops.bwd_plan(n, e, dims, ws_bytes)["edges_per_chunk"] < 3000
    W = [torch.randn(dims[i + 1], dims[i]).to(d) / 16 for i in range(3)]
    B = [torch.zeros(dims[i + 1], device=d) for i in range(3)]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d)
    with pytest.raises(_lib.GpdeError, match="in-degree"):
        ops.nnconv_backward_raw(torch.randn(n, 64, device=d), csr, torch.randn(e, 6, device=d), W, B, None, "mean",
                                torch.randn(n, 64, device=d), ws=ws)
    torch.cuda.synchronize()
