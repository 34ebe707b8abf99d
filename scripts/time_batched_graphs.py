"""The radius graphs of B sampled point sets: ONE ops.radius_csr_batched call against the per-graph loop of ops.radius_csr
(what a training script had before: one build per sample, UAI3_resolution.py:131-145).  B in {64, 1024} self graphs of 200 and
1,000 random points in the unit square at r = 0.1.  Each figure is a host clock around work that ends in a device synchronise;
one warm-up of every shape, then `--reps` alternating repetitions of both forms; median, minimum and maximum are printed.
The two forms are compared edge for edge before anything is timed.
usage: time_batched_graphs.py [--reps 5] [--out profiles/batched_graphs.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from graph_pde_amd import ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: there is no CPU figure"
    dev = torch.device("cuda:0")
    r = 0.1
    lines = [f"scripts/time_batched_graphs.py --reps {args.reps}: {torch.cuda.get_device_name(0)}, self graphs of random points in [0, 1]^2, r = {r}",
             "ms per batch, wall clock ending in a synchronise; median [min .. max] over the repetitions, the two forms alternating",
             f"{'B':>5} {'points':>7} {'edges':>10} | {'batched call':>28} | {'loop of radius_csr':>28} | {'loop / batched':>14} | {'ms per graph':>22}"]

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    for n_graphs in (64, 1024):
        for n in (200, 1000):
            g = torch.Generator().manual_seed(1000 * n_graphs + n)
            pos = torch.rand(n_graphs * n, 2, generator=g, dtype=torch.float64).to(dev)
            ptr = torch.arange(n_graphs + 1, dtype=torch.int64) * n                    # host tensor: no copy back inside the call
            parts = [pos[b * n:(b + 1) * n] for b in range(n_graphs)]
            batched = lambda: ops.radius_csr_batched(pos, ptr, r)
            loop = lambda: [ops.radius_csr(p, r) for p in parts]
            (csr, edge_ptr), per = batched(), loop()                                  # warm-up of both shapes, and the comparison
            assert csr.n_edges == sum(c.n_edges for c in per)
            assert torch.equal(csr.src, torch.cat([c.src + b * n for b, c in enumerate(per)]))
            assert torch.equal(csr.rowptr[1:], torch.cat([c.rowptr[1:] + int(e) for c, e in zip(per, edge_ptr.tolist())]))
            tb, tl = [], []
            for _ in range(args.reps):
                tb.append(clock(batched)[0])
                tl.append(clock(loop)[0])
            mb, ml = statistics.median(tb), statistics.median(tl)
            lines.append(f"{n_graphs:>5} {n:>7} {csr.n_edges:>10} | {mb:>9.3f} [{min(tb):>7.3f} .. {max(tb):>7.3f}] | {ml:>9.3f} [{min(tl):>7.3f} .. {max(tl):>7.3f}] | "
                         f"{ml / mb:>13.1f}x | {mb / n_graphs:>8.4f} vs {ml / n_graphs:>8.4f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
