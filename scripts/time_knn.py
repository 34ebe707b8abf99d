"""Developer probe of the k-nearest-neighbour builder (graph_pde_amd.neighbor_graph.knn_csr, gpde_knn.hip) at k = 16 on
    lattice241   the 241 x 241 lattice (58,081 points, the headline point set);
    uniform_1m   10^6 uniform points in the unit square;
    clustered_1m 10^6 points: 9 of 10 in 64 Gaussian blobs of sigma = 0.01 (centres uniform in [0.1, 0.9]^2), the rest uniform in
                 the unit square - about 20 times the mean density at a blob's centre, a tenth of it between the blobs.
HIP events around each piece, `--warmup` calls, then `--reps` calls with the pieces alternating; median [min .. max] are printed:
    knn            knn_csr(pos, k, loop=True)                       - bounds read from the points (one synchronisation);
    knn_bounds     knn_csr(pos, k, loop=True, bounds=(0, 1))        - no synchronisation at all;
    composite      what the library offered before: ops.radius_csr(pos, r, max_num_neighbors=k, select="nearest") at the SMALLEST
                   radius at which every destination has k sources (read off the kNN graph itself: nobody knows it beforehand).
                   It includes the point itself, hence loop=True on the other side; where it runs the two graphs are compared.
                   Where its candidate graph cannot be formed, the count of candidate pairs is reported instead.
No bar is set: nobody had measured either route.
usage: time_knn.py [--k 16] [--reps 10] [--warmup 3] [--inputs lattice241,uniform_1m,clustered_1m] [--out profiles/knn_build.txt]"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from graph_pde_amd import neighbor_graph as ng, ops, synth

N_BLOBS, BLOB_SIGMA, BLOB_SHARE = 64, 0.01, 0.9


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def make_input(name, dev):
    g = torch.Generator().manual_seed(71)
    if name == "lattice241":
        return synth.lattice_positions(241, dev).double()
    if name == "uniform_1m":
        return torch.rand(1_000_000, 2, generator=g, dtype=torch.float64).to(dev)
    if name == "clustered_1m":
        n_in = int(1_000_000 * BLOB_SHARE)
        centres = 0.1 + 0.8 * torch.rand(N_BLOBS, 2, generator=g, dtype=torch.float64)
        blob = torch.randint(0, N_BLOBS, (n_in,), generator=g)
        pts = torch.cat([centres[blob] + BLOB_SIGMA * torch.randn(n_in, 2, generator=g, dtype=torch.float64),
                         torch.rand(1_000_000 - n_in, 2, generator=g, dtype=torch.float64)])
        return pts[torch.randperm(len(pts), generator=g)].to(dev)
    raise SystemExit(f"unknown input {name!r}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inputs", default="lattice241,uniform_1m,clustered_1m")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: there is no CPU figure"
    dev = torch.device("cuda:0")
    k = args.k
    lines = [f"scripts/time_knn.py --k {k} --reps {args.reps} --warmup {args.warmup} --inputs {args.inputs}: {torch.cuda.get_device_name(0)}",
             f"ms between HIP events, {args.warmup} warm-up calls, median [min .. max] over {args.reps} calls, the pieces alternating"]
    for name in args.inputs.split(","):
        pos = make_input(name, dev)
        n = int(pos.size(0))
        csr = ng.knn_csr(pos, k, loop=True)
        d2 = ops.edge_sqdist_keys(csr, pos).view(torch.float64)
        r = math.sqrt(float(d2.max())) * (1.0 + 1e-12)          # the smallest radius that holds k sources around every destination
        r_typ = math.sqrt(float(d2.view(n, -1).max(dim=1).values.median()))
        lines.append(f"{name}: {n} points, k = {k}, {csr.n_edges} edges; k-th neighbour distance: median {r_typ:.4g}, largest {r:.4g} = the composite's radius")
        pieces = {"knn": lambda: ng.knn_csr(pos, k, loop=True), "knn_bounds": lambda: ng.knn_csr(pos, k, loop=True, bounds=(0.0, 1.0))}
        candidates = int(ops.radius_in_degrees(pos, r).long().sum())      # the COUNT pass of the radius builder: no edge is formed
        fits = candidates < (1 << 31) - 64
        lines.append(f"{'':>12} composite candidates: {candidates} pairs within r (ops.radius_in_degrees): {candidates / csr.n_edges:.1f} x the graph, "
                     f"{'fit' if fits else 'do NOT fit'} the int32 CSR")
        if fits:
            pieces["composite"] = lambda: ops.radius_csr(pos, r, max_num_neighbors=k, select="nearest")
        outs = {}
        for _ in range(args.warmup):
            for pname, fn in pieces.items():
                outs[pname] = timed(fn)[1]
        for pname, got in outs.items():
            same = torch.equal(got.rowptr, csr.rowptr) and torch.equal(got.src, csr.src) and torch.equal(got.dst, csr.dst)
            lines.append(f"{'':>12} {pname}: graph {'IDENTICAL to' if same else 'DIFFERS from'} the first knn_csr build")
        del outs
        ms = {pname: [] for pname in pieces}
        for _ in range(args.reps):
            for pname, fn in pieces.items():
                ms[pname].append(timed(fn)[0])
        for pname, v in ms.items():
            med = statistics.median(v)
            lines.append(f"{pname:>12} | {med:>10.3f} [{min(v):>9.3f} .. {max(v):>9.3f}] ms | {n / med / 1e3:8.2f} M destinations/s")
        if not fits:
            lines.append(f"{'composite':>12} | not run: ops.radius_csr refuses {candidates} candidate edges (int32 CSR)")
        del csr, d2
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
