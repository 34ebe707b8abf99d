"""Developer probe of the diagonal-kernel operator (csrc/gpde_diagconv.hip; ops.diagconv_forward_raw / DiagConvFunction) against
the stock-torch chain `x[src] * k`, `index_add`, `mm`, on radius graphs of the s x s unit-square lattice.  bench.py does not call it.
    forward            w = 64 on the 241^2 r = 0.10 graph (the headline graph, 95.5 M edges: k is 24 GB)
    forward            w = 32 / 128 / 256 on the s = 61 graph
    forward+backward   w = 64 on the s = 121 graph (gradients of x, k, root and bias)
The per-edge kernel k [E, w] is given (random): what is timed is gather, message, aggregation (mean) and update().
HIP events, warm-up first, `--reps` windows with the arms alternating, median [min .. max] of the ms per call.  Next to each native
forward: the rate at 8 w + 4 bytes per edge (the k row, one gathered x row, the source index) and the rate with the x table read once
(4 w + 4 bytes per edge that must come from memory, plus x and out): the tables here fit the caches, so the second is the HBM traffic.
usage: bench_diag.py [--reps 7] [--quick] [--out profiles/diag_bench.txt]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

from graph_pde_amd import ops
from graph_pde_amd.autograd import DiagConvFunction


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def fmt(v):
    return f"{statistics.median(v):>9.3f} [{min(v):>8.3f} .. {max(v):>8.3f}] ms"


def lattice_csr(s, r, dev):
    g = torch.linspace(0, 1, s, device=dev)
    pos = torch.stack(torch.meshgrid(g, g, indexing="ij"), dim=-1).reshape(-1, 2).contiguous()
    return ops.radius_csr(pos, r), s * s


def chain_forward(x, src, dst, k, root, bias, n, inv_deg):
    out = torch.zeros(n, x.size(1), dtype=x.dtype, device=x.device).index_add_(0, dst, x.index_select(0, src) * k) * inv_deg
    return out + torch.mm(x, root) + bias


def run(lines, s, r, widths, reps, backward, dev):
    csr, n = lattice_csr(s, r, dev)
    e = csr.n_edges
    src, dst = csr.src.long(), csr.dst.long()
    inv_deg = (1.0 / torch.bincount(dst, minlength=n).clamp(min=1).float()).unsqueeze(1)
    lines.append(f"s = {s}, r = {r}: {n} nodes, {e} edges, largest in-degree {csr.max_in_degree}")
    inner = 1 if e > 20_000_000 else 5
    for w in widths:
        torch.manual_seed(w)
        x, k = torch.randn(n, w, device=dev), torch.randn(e, w, device=dev)
        root, bias, g = torch.randn(w, w, device=dev) / w ** 0.5, torch.randn(w, device=dev), torch.randn(n, w, device=dev)
        if not backward:
            arms = {"native": lambda: ops.diagconv_forward_raw(x, ops._ONE_SET, csr, k, root, bias, "mean"),
                    "torch chain": lambda: chain_forward(x, src, dst, k, root, bias, n, inv_deg)}
        else:
            lv = [t.clone().requires_grad_(True) for t in (x, k, root, bias)]

            def native_step():
                for t in lv:
                    t.grad = None
                (DiagConvFunction.apply(lv[0], ops._ONE_SET, lv[1], csr, lv[2], lv[3], "mean") * g).sum().backward()

            def chain_step():
                for t in lv:
                    t.grad = None
                (chain_forward(lv[0], src, dst, lv[1], lv[2], lv[3], n, inv_deg) * g).sum().backward()
            arms = {"native": native_step, "torch chain": chain_step}
        with torch.no_grad() if not backward else torch.enable_grad():
            if not backward:
                a, b = arms["native"](), arms["torch chain"]()
                err = float((a - b).norm() / b.norm())
                del a, b
            for fn in arms.values():
                timed(fn)
            ms = {name: [] for name in arms}
            for _ in range(reps):
                for name, fn in arms.items():
                    ms[name].append(timed(fn, inner))
        p = ops.diag_plan(w)
        per_edge = 8 * w + 4
        lines.append(f"  w = {w} ({'forward + backward' if backward else 'forward'}; V = {p['V']}, LC = {p['LC']}, ES = {p['ES']}): "
                     f"{per_edge} B per edge forward = {per_edge * e / 1e9:.2f} GB")
        for name, v in ms.items():
            line = f"{name:>16} | {fmt(v)}"
            if name == "native" and not backward:
                med = statistics.median(v)
                line += (f" | {per_edge * e / med / 1e9:6.2f} TB/s at 8 w + 4 B per edge; {((4 * w + 4) * e + 8 * n * w) / med / 1e9:6.2f} TB/s with x read and "
                         "out written once (4 w + 4 B per edge from memory)")
            lines.append(line)
        if not backward:
            lines.append(f"{'|native - chain|':>16} | {err:9.2e} of |chain| (float32 both)")
        lines.append(f"{'chain / native':>16} | {statistics.median(ms['torch chain']) / statistics.median(ms['native']):9.2f} x")
        del x, k, arms
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="without the 241^2 graph")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: there is no CPU figure"
    dev = torch.device("cuda:0")
    lines = [f"scripts/bench_diag.py --reps {args.reps}: {torch.cuda.get_device_name(0)}",
             "ms per call between HIP events, warm-up first, median [min .. max] over the windows, the arms alternating; aggr = mean"]
    print("\n".join(lines), flush=True)
    jobs = [(61, [32, 128, 256], False), (121, [64], True)] + ([] if args.quick else [(241, [64], False)])
    for s, widths, backward in jobs:
        done = len(lines)
        run(lines, s, 0.10, widths, args.reps, backward, dev)
        print("\n".join(lines[done:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
