"""Developer probe: the two routes of an any-width NNConv module against each other on one device.

    python scripts/time_any_reassoc.py [--s 31] [--r 0.1] [--steps 10] [--warmup 3] [--out FILE]

For (in, out) in 32 -> 32, 128 -> 128, 24 -> 40 and last hidden width K in 64, 1024 on synth.darcy_graph(s, r), a module
NNConv_old(in, out, DenseNet([6, 32, K, in * out]), aggr='mean') runs forward (no_grad) and forward + backward under
GPDE_ANY_REASSOC=off (materialised: `nn(pseudo)` as [E, in * out], gpde_weconv_any.hip) and =on (re-associated: torch evaluates the
hidden layers, gpde_reassoc_any.hip the rest).  ms per call, HIP events over `steps` calls after `warmup` calls, whole module
calls - torch's part of each route included.  A route whose tensors do not fit the free memory is reported as refused.
Nothing in the tests depends on these times (DESIGN.md §7 records one run)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_pde_amd as gp                                       # noqa: E402
from graph_pde_amd import ops, synth                             # noqa: E402


def dense_net(dims):
    layers = []
    for j in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[j], dims[j + 1]))
        if j != len(dims) - 2:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers)


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
             f"kernel network [6, 32, K, in * out]",
             f"graph s={a.s} r={a.r}: N={n} E={e}",
             f"{'widths':>10} {'K':>5} {'route':>13} {'fwd ms':>9} {'fwd+bwd ms':>11} {'per-edge MiB':>13} {'last-layer GFLOP':>17}"]
    mode0 = ops.ANY_REASSOC
    for cin, cout in ((32, 32), (128, 128), (24, 40)):
        for k in (64, 1024):
            torch.manual_seed(0)
            conv = gp.NNConv_old(cin, cout, dense_net([6, 32, k, cin * cout]), aggr="mean").to(d)
            x = torch.randn(n, cin, device=d)
            g = torch.randn(n, cout, device=d)
            free, _ = ops.device_free_bytes(d)
            info = ops.any_width_route(n, e, cin, cout, k, "mean", True, free, mode="on")
            for mode, route, nbytes, flops in (("off", "materialised", info["bytes_materialised"], info["flops_materialised"]),
                                               ("on", "re-associated", info["bytes_reassociated"], info["flops_reassociated"])):
                ops.ANY_REASSOC = mode

                def fwd():
                    with torch.no_grad():
                        return conv(x, ei, ea)

                def step():
                    conv.zero_grad(set_to_none=True)
                    xin = x.clone().requires_grad_(True)
                    (conv(xin, ei, ea) * g).sum().backward()
                try:
                    f, b = timed(fwd, a.steps, a.warmup), timed(step, a.steps, a.warmup)
                    lines.append(f"{cin:>4} -> {cout:<3} {k:>5} {route:>13} {f:>9.3f} {b:>11.3f} {nbytes / 2**20:>13.1f} {flops / 1e9:>17.2f}")
                except torch.OutOfMemoryError as exc:
                    lines.append(f"{cin:>4} -> {cout:<3} {k:>5} {route:>13}   out of memory: {str(exc).splitlines()[0][:120]}")
                except RuntimeError as exc:
                    # the routing refusal alone is a row of the table; anything else (a HIP error, the library's own) ends the probe
                    if "the per-edge weights are materialised as in the reference" not in str(exc):
                        raise
                    lines.append(f"{cin:>4} -> {cout:<3} {k:>5} {route:>13}   refused: {str(exc).splitlines()[0][:120]}")
                torch.cuda.empty_cache()
    ops.ANY_REASSOC = mode0
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
