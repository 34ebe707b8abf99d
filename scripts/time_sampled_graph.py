"""Developer probe of the sampled graphs (graph_pde_amd.sampled_graph.gaussian_csr, the sampled arm of gpde_cellgraph.hip) at
sigma = 0.1 on the s x s lattices, s = 61, 121, 241 (the headline point set: 58,081 points).  HIP events around each piece, one
warm-up, `--reps` repetitions with the pieces alternating; median [min .. max] are printed:
    native     sampled_graph.gaussian_csr(pos, sigma, seed) - cell binning, COUNT, the scan and its one sync, FILL;
    count      sampled_graph.gaussian_in_degrees - the COUNT pass alone;
    composite  what the library offered before: ops.radius_csr at r_support = sigma sqrt(54 ln 2), ops.edge_hash_keys and
               ops.edge_sqdist_keys over its edges, u < exp(-d2 / sigma^2) as a torch mask in float64, ops.csr_for of the kept
               edges.  Run only where the candidate graph fits the int32 CSR (ops.radius_in_degrees tells without building it);
               where it runs, its edge set is compared with the native one (as sets: the composite inherits the cell order of
               ball rows longer than 4,096 edges).  The peak of device memory of each piece is taken during its warm-up.
No bar is set: nobody had measured either route.
usage: time_sampled_graph.py [--sizes 61,121,241] [--sigma 0.1] [--seed 0] [--reps 5] [--out profiles/gaussian_graph.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from graph_pde_amd import ops, sampled_graph as sg, synth


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def composite(pos, sigma, seed):
    ball = ops.radius_csr(pos, sg.gaussian_support_radius(sigma))
    u = ((ops.edge_hash_keys(ball.src, ball.dst, seed) >> 10).double() + 0.5) * 2.0 ** -53
    p = torch.exp(-(ops.edge_sqdist_keys(ball, pos).view(torch.float64) / (sigma * sigma)))
    keep = u < p
    return ops.csr_for(ball.edge_index[:, keep], ball.n_nodes), (u - p).abs() <= 4.0 * torch.finfo(torch.float64).eps * p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="61,121,241")
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: there is no CPU figure"
    dev = torch.device("cuda:0")
    sigma, seed = args.sigma, args.seed
    r_sup = sg.gaussian_support_radius(sigma)
    lines = [f"scripts/time_sampled_graph.py --sizes {args.sizes} --sigma {sigma} --seed {seed} --reps {args.reps}: {torch.cuda.get_device_name(0)}",
             f"r_support = {r_sup:.4f}; ms between HIP events, one warm-up, median [min .. max] over {args.reps} repetitions, the pieces alternating"]
    for s in (int(t) for t in args.sizes.split(",")):
        pos = synth.lattice_positions(s, dev).double()
        n = int(pos.size(0))
        candidates = int(ops.radius_in_degrees(pos, r_sup).long().sum())
        fits = candidates < (1 << 31) - 64
        pieces = {"native": lambda: sg.gaussian_csr(pos, sigma, seed), "count": lambda: sg.gaussian_in_degrees(pos, sigma, seed)}
        if fits:
            pieces["composite"] = lambda: composite(pos, sigma, seed)
        outs, peak = {}, {}
        for name, fn in pieces.items():                                  # warm-up of every piece; its peak of device memory
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            outs[name] = timed(fn)[1]
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
        csr = outs["native"]
        lines.append(f"s = {s}: {n} points, {candidates} candidate pairs within r_support "
                     f"({'fit' if fits else 'do NOT fit'} the int32 CSR), {csr.n_edges} sampled edges "
                     f"(pi sigma^2 n^2 = {3.141592653589793 * sigma * sigma * n * n:.4g}), largest in-degree {csr.max_in_degree}")
        if fits:
            comp, undecided = outs["composite"]
            # as sets: a ball row of more than 4,096 edges is in cell order, and the composite inherits that order
            code = lambda g: g.dst.long() * n + g.src.long()
            same = comp.n_edges == csr.n_edges and torch.equal(comp.rowptr, csr.rowptr) and torch.equal(code(comp).sort().values, code(csr))
            lines.append(f"{'':>12} composite edge set {'IDENTICAL to' if same else 'DIFFERS from'} the native one "
                         f"({comp.n_edges} edges; {int(undecided.sum())} candidate pairs within 4 ulp of the threshold)")
            del comp, undecided
        del outs
        ms = {name: [] for name in pieces}
        for _ in range(args.reps):
            for name, fn in pieces.items():
                ms[name].append(timed(fn)[0])
        for name, v in ms.items():
            med = statistics.median(v)
            line = f"{name:>12} | {med:>10.3f} [{min(v):>9.3f} .. {max(v):>9.3f}] ms"
            line += f" | peak {peak[name]:7.2f} GiB above the positions"
            if name == "native":
                line += f" | {csr.n_edges / med / 1e3:8.1f} M edges/s"
            lines.append(line)
        if not fits:
            lines.append(f"{'composite':>12} | not run: ops.radius_csr refuses {candidates} edges (int32 CSR)")
        del csr
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
