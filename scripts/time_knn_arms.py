"""Developer probe of the two further arms of the k-nearest-neighbour builder (graph_pde_amd.neighbor_graph.knn_csr_batched,
knn_csr(period=...); gpde_knn_arms.hip) at k = 16, in the method of scripts/time_knn.py: HIP events around each piece, `--warmup`
calls, then `--reps` calls with the pieces alternating; median [min .. max] are printed.
    (a) batched    knn_csr_batched(pos, ptr, k) and the same with bounds= given (no synchronisation), against a loop over knn_csr
                   with its concatenation (the open arm, one build and one bounds read-back per graph), on
                       b64_1024    64 graphs of 1,024 uniform points;
                       b8_58081    8 graphs of the 241 x 241 lattice (58,081 points each, jittered per graph);
    (b) periodic   knn_csr(pos, k, period=1) against the open knn_csr(pos, k, bounds=(0, 1)) on the same points, on the 241 x 241
                   lattice and on 10^6 uniform points;
    (c) open arm   gpde_knn_csr of THIS library against the same entry point of another build of the library (--parent-lib: the
                   parent commit's libgpde.so), through the C ABI on identical buffers, on the three inputs of
                   profiles/knn_build.txt.  The parent is timed twice per round (parent_a, parent_b): the distance of their
                   medians is the spread two runs of one build show in this session, the bar for |this - parent|.
(a) and (b) are records of what the arms cost; (c) is the acceptance bar of the change that added the arms.
usage: time_knn_arms.py [--k 16] [--reps 10] [--warmup 3] [--parts a,b,c] [--parent-lib PATH] [--out profiles/knn_arms.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from graph_pde_amd import _lib, neighbor_graph as ng, ops, synth
from time_knn import make_input, timed


def run_pieces(pieces, warmup, reps):
    """{name: [ms]} with the pieces alternating, and the outputs of the last warm-up round."""
    outs = {}
    for _ in range(warmup):
        for name, fn in pieces.items():
            outs[name] = timed(fn)[1]
    ms = {name: [] for name in pieces}
    for _ in range(reps):
        for name, fn in pieces.items():
            ms[name].append(timed(fn)[0])
    return ms, outs


def report(lines, ms, n_dst):
    for name, v in ms.items():
        med = statistics.median(v)
        lines.append(f"{name:>14} | {med:>10.3f} [{min(v):>9.3f} .. {max(v):>9.3f}] ms | {n_dst / med / 1e3:8.2f} M destinations/s")


def loop_over_knn_csr(pos, ptr, k):
    """What a kNN user did before: one knn_csr per graph, concatenated with the graphs' offsets."""
    rowptr, src, dst, off = [torch.zeros(1, dtype=torch.int32, device=pos.device)], [], [], 0
    for b in range(len(ptr) - 1):
        csr = ng.knn_csr(pos[ptr[b]:ptr[b + 1]], k)
        rowptr.append(csr.rowptr[1:] + off)
        src.append(csr.src + ptr[b])
        dst.append(csr.dst + ptr[b])
        off += csr.n_edges
    return torch.cat(rowptr), torch.cat(src), torch.cat(dst)


def part_a(lines, k, warmup, reps, dev):
    g = torch.Generator().manual_seed(72)
    lattice = synth.lattice_positions(241, dev).double()
    batches = {"b64_1024": [torch.rand(1024, 2, generator=g, dtype=torch.float64).to(dev) for _ in range(64)],
               "b8_58081": [lattice + 1e-4 * torch.rand(lattice.shape, generator=g, dtype=torch.float64).to(dev) for _ in range(8)]}
    for name, sets in batches.items():
        pos = torch.cat(sets)
        ptr = [0]
        for s in sets:
            ptr.append(ptr[-1] + int(s.size(0)))
        bounds = torch.stack([torch.stack([s.min(dim=0).values, s.max(dim=0).values]) for s in sets]).cpu()
        ptr_t = torch.tensor(ptr)
        pieces = {"batched": lambda: ng.knn_csr_batched(pos, ptr_t, k)[0],
                  "batched_bounds": lambda: ng.knn_csr_batched(pos, ptr_t, k, bounds=bounds)[0],
                  "loop": lambda: loop_over_knn_csr(pos, ptr, k)}
        ms, outs = run_pieces(pieces, warmup, reps)
        ref = outs["loop"]
        lines.append(f"(a) {name}: {len(sets)} graphs, {int(pos.size(0))} points, k = {k}, {int(ref[1].numel())} edges")
        for pname in ("batched", "batched_bounds"):
            c = outs[pname]
            same = torch.equal(c.rowptr, ref[0]) and torch.equal(c.src, ref[1]) and torch.equal(c.dst, ref[2])
            lines.append(f"{'':>14} {pname}: graph {'IDENTICAL to' if same else 'DIFFERS from'} the loop over knn_csr")
        report(lines, ms, int(pos.size(0)))
        del outs, ref
        torch.cuda.empty_cache()


def part_b(lines, k, warmup, reps, dev):
    for name in ("lattice241", "uniform_1m"):
        pos = make_input(name, dev)
        n = int(pos.size(0))
        pieces = {"periodic": lambda: ng.knn_csr(pos, k, period=1.0), "open_bounds": lambda: ng.knn_csr(pos, k, bounds=(0.0, 1.0))}
        ms, outs = run_pieces(pieces, warmup, reps)
        differ = int((outs["periodic"].src != outs["open_bounds"].src).view(n, -1).any(dim=1).sum())
        lines.append(f"(b) {name}: {n} points, k = {k}; {differ} rows of the torus graph differ from the open one (the rows at the seam)")
        report(lines, ms, n)
        del outs
        torch.cuda.empty_cache()


def bind(path):
    """Another build of the library, with the argument types of this header for the two entry points of the open arm."""
    lib = ctypes.CDLL(path)
    for name in ("gpde_knn_csr_workspace_bytes", "gpde_knn_csr"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def part_c(lines, k, warmup, reps, dev, parent_path):
    libs = {"this": _lib.lib(), "parent_a": bind(parent_path), "parent_b": bind(parent_path)}
    D = ctypes.c_double * 2
    lo, hi = D(0.0, 0.0), D(1.0, 1.0)
    for name in ("lattice241", "uniform_1m", "clustered_1m"):
        pos = make_input(name, dev)
        n = int(pos.size(0))
        nbytes = max(int(l.gpde_knn_csr_workspace_bytes(n, n, 2, k, 0.0, lo, hi)) for l in libs.values())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        bufs = {pname: (torch.empty(n * k, dtype=torch.int32, device=dev), torch.empty(n * k, dtype=torch.int32, device=dev)) for pname in libs}
        stream = ops._stream_ptr(dev)

        def call(pname):
            src, dst = bufs[pname]
            _lib.check(libs[pname].gpde_knn_csr(pos.data_ptr(), n, pos.data_ptr(), n, 2, k, 1, 0.0, lo, hi, rowptr.data_ptr(), src.data_ptr(),
                                                dst.data_ptr(), None, ws.data_ptr(), nbytes, stream), "gpde_knn_csr")
            return src

        pieces = {pname: (lambda p=pname: call(p)) for pname in libs}
        ms, outs = run_pieces(pieces, warmup, reps)
        same = torch.equal(outs["this"], outs["parent_a"])
        med = {p: statistics.median(v) for p, v in ms.items()}
        lines.append(f"(c) {name}: {n} points, k = {k}, gpde_knn_csr(loop = 1, bounds (0, 1)) through the C ABI; the graph is "
                     f"{'IDENTICAL to' if same else 'DIFFERENT from'} the parent build's")
        report(lines, ms, n)
        parent = 0.5 * (med["parent_a"] + med["parent_b"])
        lines.append(f"{'':>14} this - parent = {med['this'] - parent:+.3f} ms ({100.0 * (med['this'] - parent) / parent:+.2f} %); "
                     f"|parent_a - parent_b| = {abs(med['parent_a'] - med['parent_b']):.3f} ms ({100.0 * abs(med['parent_a'] - med['parent_b']) / parent:.2f} %)")
        del bufs, ws, outs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--parent-lib", default=None, help="libgpde.so of the commit to compare the open arm with (part c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: there is no CPU figure"
    dev = torch.device("cuda:0")
    lines = [f"scripts/time_knn_arms.py --k {args.k} --reps {args.reps} --warmup {args.warmup} --parts {args.parts}: {torch.cuda.get_device_name(0)}",
             f"ms between HIP events, {args.warmup} warm-up calls, median [min .. max] over {args.reps} calls, the pieces alternating"]
    parts = args.parts.split(",")
    if "a" in parts:
        part_a(lines, args.k, args.warmup, args.reps, dev)
    if "b" in parts:
        part_b(lines, args.k, args.warmup, args.reps, dev)
    if "c" in parts:
        if not args.parent_lib:
            raise SystemExit("part c compares with another build of the library: pass --parent-lib PATH")
        part_c(lines, args.k, args.warmup, args.reps, dev, args.parent_lib)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
