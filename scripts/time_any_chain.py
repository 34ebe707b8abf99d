"""Developer probe: the streamed any-width route against the re-associated one on one device.

    python scripts/time_any_chain.py [--s 31] [--r 0.1] [--steps 10] [--warmup 3] [--out FILE]

The shapes of scripts/time_any_reassoc.py - (in, out) in 32 -> 32, 128 -> 128, 24 -> 40, last hidden width K in 64, 1024, kernel
network DenseNet([6, 32, K, in * out]), aggr='mean', synth.darcy_graph(s, r) - under GPDE_ANY_REASSOC=on (re-associated: torch
evaluates the hidden layers as [E, K], gpde_reassoc_any.hip the rest) and =streamed (gpde_chain_any.hip: the hidden rows by block of
destination nodes), the latter at one block and at a budget of E / 8 hidden rows per block.  The two modes alternate, call for call
group for group: `on` runs first and last and both of its times are printed - their difference is the spread of the run.  ms per
whole module call (torch's part included), HIP events over `steps` calls after `warmup` calls.  Nothing in the tests depends on
these times (DESIGN.md §7 records one run)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_pde_amd as gp                                       # noqa: E402
from graph_pde_amd import ops, synth                             # noqa: E402
from time_any_reassoc import dense_net, timed                    # noqa: E402


def per_edge_bytes(dims):
    """Bytes per hidden row of a backward block: what gpde_nnconv_chain_any_plan spends its budget in."""
    kp = [(k + 3) // 4 * 4 for k in dims[1:-1]]
    return (sum(kp) + kp[-1] + 2 * max(kp)) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=31)
    ap.add_argument("--r", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = torch.device("cuda:0")
    ei, ea, n = synth.darcy_graph(a.s, a.r, device=d)
    e = ei.shape[1]
    lines = [f"# 1 x {torch.cuda.get_device_name(0)}; ms per module call (HIP events over {a.steps} calls after {a.warmup}); aggr mean; "
             f"kernel network [6, 32, K, in * out]; one run on one box - no default route moves on it",
             f"graph s={a.s} r={a.r}: N={n} E={e}",
             f"{'widths':>10} {'K':>5} {'route':>22} {'blocks':>6} {'fwd ms':>9} {'fwd+bwd ms':>11} {'ws bwd MiB':>11} {'[E,K] MiB':>10}"]
    mode0, budget0 = ops.ANY_REASSOC, ops.CHAIN_ANY_PREF_BUDGET
    for cin, cout in ((32, 32), (128, 128), (24, 40)):
        for k in (64, 1024):
            torch.manual_seed(0)
            dims = [6, 32, k, cin * cout]
            conv = gp.NNConv_old(cin, cout, dense_net(dims), aggr="mean").to(d)
            x = torch.randn(n, cin, device=d)
            g = torch.randn(n, cout, device=d)
            csr = ops.csr_for(ei, n)

            def fwd():
                with torch.no_grad():
                    return conv(x, ei, ea)

            def step():
                conv.zero_grad(set_to_none=True)
                xin = x.clone().requires_grad_(True)
                (conv(xin, ei, ea) * g).sum().backward()
            runs = (("on", "re-associated", None), ("streamed", "streamed, one block", 1 << 40),
                    ("streamed", "streamed, E/8 per block", max(1, e // 8) * per_edge_bytes(dims)), ("on", "re-associated (again)", None))
            for mode, label, budget in runs:
                ops.ANY_REASSOC = mode
                blocks, ws = "-", "-"
                if budget is not None:
                    ops.CHAIN_ANY_PREF_BUDGET = budget
                    plan = ops.chain_any_blocks(csr, dims, cin, cin, cout, budget_bytes=budget)
                    blocks, ws = str(plan.n_blocks), f"{plan.ws_bwd / 2**20:.1f}"
                f, b = timed(fwd, a.steps, a.warmup), timed(step, a.steps, a.warmup)
                lines.append(f"{cin:>4} -> {cout:<3} {k:>5} {label:>22} {blocks:>6} {f:>9.3f} {b:>11.3f} {ws:>11} {e * k * 4 / 2**20:>10.1f}")
                torch.cuda.empty_cache()
    ops.ANY_REASSOC, ops.CHAIN_ANY_PREF_BUDGET = mode0, budget0
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
