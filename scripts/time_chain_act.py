"""Developer probe: the streamed any-width route per hidden activation on one device.

    python scripts/time_chain_act.py [--kinds all|relu,gelu,..] [--s 31] [--r 0.1] [--steps 50] [--warmup 5] [--reps 3]
                                     [--tree DIR] [--json FILE] [--baseline JSON [JSON ..]] [--out FILE]

The shapes of scripts/time_any_chain.py - (in, out) in 32 -> 32, 128 -> 128, 24 -> 40, last hidden width K in 64, 1024, kernel
network [6, 32, K, in * out], aggr='mean', synth.darcy_graph(s, r) - under GPDE_ANY_REASSOC=streamed with the default block budget,
once per activation kind (ops.ACT_NAMES; `relu` is the route of the `_chain_any` entry points).  ms per whole module call, forward
(no gradient) and forward + backward, HIP events over `steps` calls after `warmup` calls, `reps` windows per figure: the median is
reported, the windows' min .. max beside it.

The baseline is another BUILD's ReLU time on the same box: `--tree DIR` imports the package from DIR (a checkout of the parent commit
with its library built; only `--kinds relu` is meaningful there) and `--json` keeps the windows; a later run of this tree with
`--baseline` those files prints each kind as a ratio to the baseline's median and the baseline's own run-to-run spread.  Alternate the
two builds process by process in one job.  Nothing in the tests depends on these times (DESIGN.md records one run)."""
import argparse
import json
import os
import statistics
import sys

import torch


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="all")
    ap.add_argument("--s", type=int, default=31)
    ap.add_argument("--r", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default=None)
    ap.add_argument("--baseline", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import graph_pde_amd as gp
    from graph_pde_amd import ops, synth
    nn = torch.nn
    modules = {"relu": nn.ReLU, "leaky_relu": lambda: nn.LeakyReLU(0.2), "elu": nn.ELU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "gelu": nn.GELU,
               "gelu_tanh": lambda: nn.GELU(approximate="tanh"), "silu": nn.SiLU, "sin": getattr(gp, "Sin", None)}
    kinds = list(modules) if a.kinds == "all" else a.kinds.split(",")
    d = torch.device("cuda:0")
    ei, ea, n = synth.darcy_graph(a.s, a.r, device=d)
    e = ei.shape[1]
    ops.ANY_REASSOC = "streamed"
    res = {}
    for cin, cout in ((32, 32), (128, 128), (24, 40)):
        for k in (64, 1024):
            dims = [6, 32, k, cin * cout]
            csr = ops.csr_for(ei, n)
            x, g = torch.randn(n, cin, device=d), torch.randn(n, cout, device=d)
            for kind in kinds:
                torch.manual_seed(0)
                net = nn.Sequential(nn.Linear(6, 32), modules[kind](), nn.Linear(32, k), modules[kind](), nn.Linear(k, cin * cout))
                conv = gp.NNConv_old(cin, cout, net, aggr="mean").to(d)

                def fwd():
                    with torch.no_grad():
                        return conv(x, ei, ea)

                def step():
                    conv.zero_grad(set_to_none=True)
                    xin = x.clone().requires_grad_(True)
                    (conv(xin, ei, ea) * g).sum().backward()
                calls0 = ops._lib.n_native_calls
                step()
                assert ops._lib.n_native_calls - calls0 == 2, "not the streamed route: one native forward, one native backward"
                if kind == "relu":
                    plan = ops.chain_any_blocks(csr, dims, cin, cin, cout)
                else:
                    plan = ops.chain_any_blocks(csr, dims, cin, cin, cout, acts=ops.mlp_chain(net)[1])
                res[f"{cin}->{cout} K={k} {kind}"] = {"fwd": [timed(fwd, a.steps, a.warmup) for _ in range(a.reps)],
                                                      "step": [timed(step, a.steps, a.warmup) for _ in range(a.reps)],
                                                      "blocks": plan.n_blocks, "ws_bwd": plan.ws_bwd}
                torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    base = [json.load(open(p)) for p in a.baseline]
    med = statistics.median
    lines = [f"# 1 x {torch.cuda.get_device_name(0)}; GPDE_ANY_REASSOC=streamed, default block budget; ms per module call (HIP events over {a.steps} "
             f"calls after {a.warmup}, median of {a.reps} windows [min .. max]); aggr mean; kernel network [6, 32, K, in * out]",
             f"graph s={a.s} r={a.r}: N={n} E={e}"]
    if base:
        lines.append(f"# baseline: the ReLU chain of {len(base)} runs of another build (the parent commit) in the same job, alternating with this one; "
                     f"ratio = this build's median / the baseline's median of all its windows; its [min .. max] is its run-to-run spread")
    lines.append(f"{'shape':>18} {'kind':>10} {'blocks':>6} {'ws bwd MiB':>10} {'fwd ms':>24} {'fwd+bwd ms':>24}" + ("  fwd ratio  f+b ratio" if base else ""))
    for key, r in res.items():
        shape, kind = key.rsplit(" ", 1)
        row = f"{shape:>18} {kind:>10} {r['blocks']:>6} {r['ws_bwd'] / 2**20:>10.1f}"
        for w in ("fwd", "step"):
            row += f" {med(r[w]):>8.3f} [{min(r[w]):.3f} .. {max(r[w]):.3f}]"
        bkey = f"{shape} relu"
        if base and all(bkey in b for b in base):
            if kind == "relu":
                brow = f"{shape:>18} {'(baseline)':>10} {'':>6} {'':>10}"
                for w in ("fwd", "step"):
                    allw = [v for b in base for v in b[bkey][w]]
                    brow += f" {med(allw):>8.3f} [{min(allw):.3f} .. {max(allw):.3f}]"
                lines.append(brow)
            for w in ("fwd", "step"):
                row += f" {med(r[w]) / med([v for b in base for v in b[bkey][w]]):>10.3f}"
        lines.append(row)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
