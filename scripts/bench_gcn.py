"""Developer probe of the native GCNConv (gpde_gcn.hip) at the size of the reference's GCN baseline: `GCN_Net` of
multipole-graph-neural-operator/neurips4_GCN.py (width 128, four GCNConv modules applied `depth` = 4 times: 16 convs per forward)
on the 421 x 421 four-neighbour grid (177,241 nodes, 707,280 edges).  bench.py does not call it.  HIP events, warm-up first,
`--reps` repetitions with the arms alternating; a timed window holds `--inner` back-to-back calls of a conv (a single call is
0.1 - 2 ms: a window that short would time the launch as much as the kernel), 5 forwards or 3 steps of the net, and is reported
per call; median [min .. max] of the windows are printed:
    forward    one inference forward of the net (no_grad), native
    step       one training step (forward, loss, backward, Adam), native
    conv       ONE conv by itself at each width pair of --widths under the arms
                 (a) composite        the stock-torch chain of tests/helpers/composite_gcn.py
                 (b) aggregate + mm   the native aggregation kernel (W = NULL) followed by torch.mm   (route 'aggregate_mm')
                 (c) fused            the fused kernel: aggregation, then the multiply on the LDS tile (route 'aggregate_first')
                 (t) transform first  torch.mm, then the native aggregation kernel at width out       (route 'transform_first')
Bytes the fused conv must move, for its achieved bytes/s: x read once and out written once (N * (in + out) * 4), src and coef per
edge (E * 8), rowptr and self_coef (N * 8), W (in * out * 4) - gathered rows that miss the caches are not counted.
With --script the unmodified script itself is run at its own size (r = 1, ntrain = 2, two epochs), native and composite, and the
wall time per epoch it prints is reported.
usage: bench_gcn.py [--s 421] [--reps 7] [--inner 20] [--widths 128x128,64x64,...] [--script] [--out profiles/gcn_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
import torch.nn.functional as F

import graph_pde_amd as gp
from graph_pde_amd import ops
from tests.helpers import composite_gcn


def grid_edges(s):
    """int64 [2, E] of the s x s four-neighbour grid, both directions."""
    idx = torch.arange(s * s).view(s, s)
    right = torch.stack([idx[:, :-1].reshape(-1), idx[:, 1:].reshape(-1)])
    down = torch.stack([idx[:-1].reshape(-1), idx[1:].reshape(-1)])
    return torch.cat([right, right.flip(0), down, down.flip(0)], dim=1)


class GCNNet(torch.nn.Module):                       # neurips4_GCN.py:20-54
    def __init__(self, width=128, ker_width=1024, depth=4, in_width=6):
        super().__init__()
        self.depth = depth
        self.fc_in = torch.nn.Linear(in_width, width)
        self.convs = torch.nn.ModuleList([gp.GCNConv(width, width) for _ in range(4)])
        self.fc_out1, self.fc_out2 = torch.nn.Linear(width, ker_width), torch.nn.Linear(ker_width, 1)

    def forward(self, x, edge_index):
        x = self.fc_in(x)
        for _ in range(self.depth):
            for conv in self.convs:
                x = F.relu(conv(x, edge_index))
        return self.fc_out2(F.relu(self.fc_out1(x)))


def timed(fn, inner=1):
    """ms per call of `inner` back-to-back calls between two HIP events."""
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


def script_epoch_seconds(composite):
    cmd = [sys.executable, os.path.join(REPO, "scripts", "run_reference_script.py"), "neurips4_GCN.py", "--set", "ntrain=2", "--set", "ntest=1",
           "--set", "epochs=2"] + (["--composite"] if composite else [])
    r = subprocess.run(cmd, cwd="/tmp", capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        return f"failed: {r.stderr[-400:]}"
    secs = [float(t[1]) for t in (l.split() for l in r.stdout.splitlines()) if len(t) == 4 and t[0].isdigit()]
    return "epoch wall times printed by the script (s): " + ", ".join(f"{v:.3f}" for v in secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=421)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="conv calls per timed window")
    ap.add_argument("--widths", default="16x16,32x32,64x64,128x128,256x256,33x65,64x128,128x256,256x128,128x64")
    ap.add_argument("--script", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: there is no CPU figure"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ei = grid_edges(args.s).to(dev)
    n, e = args.s * args.s, int(ei.size(1))
    lines = [f"scripts/bench_gcn.py --s {args.s} --reps {args.reps} --inner {args.inner}: {torch.cuda.get_device_name(0)}",
             f"{n} nodes, {e} edges; ms per call between HIP events ({args.inner} conv calls, 5 forwards, 3 steps per window), warm-up first, "
             "median [min .. max] over the windows, the arms alternating",
             f"default routing of this tree: ops.gcn_route(128, 128) = {ops.gcn_route(128, 128)} (the net and the script run on it)"]

    net = GCNNet().to(dev)
    x6, y = torch.randn(n, 6, device=dev), torch.randn(n, 1, device=dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=5e-4)

    def forward():
        with torch.no_grad():
            net(x6, ei)

    def step():
        opt.zero_grad()
        F.mse_loss(net(x6, ei), y).backward()
        opt.step()
    for fn in (forward, step, forward, step):
        timed(fn)
    tf, ts = [], []
    for _ in range(args.reps):
        tf.append(timed(forward, 5))
        ts.append(timed(step, 3))
    lines += [f"{'GCN_Net forward (16 convs)':>34} | {fmt(tf)}", f"{'GCN_Net training step':>34} | {fmt(ts)}"]

    norm = ops.gcn_norm(ops.csr_for(ei, n))
    for wp in args.widths.split(","):
        cin, cout = (int(v) for v in wp.split("x"))
        conv = gp.GCNConv(cin, cout).to(dev)
        x = torch.randn(n, cin, device=dev)
        w, b = conv.weight.detach(), conv.bias.detach()
        arms = {
            "(a) composite": lambda: composite_gcn.composite_forward(conv, x, ei),
            "(b) aggregate + mm": lambda: ops.gcn_forward_raw(x, norm, w, b, route="aggregate_mm"),
            "(c) fused": lambda: ops.gcn_forward_raw(x, norm, w, b, route="aggregate_first"),
            "(t) transform first": lambda: ops.gcn_forward_raw(x, norm, w, b, route="transform_first"),
        }
        with torch.no_grad():
            ref = arms["(c) fused"]()
            for name, fn in arms.items():
                err = float((fn() - ref).norm() / ref.norm())
                assert err < 1e-4, (name, err)
                timed(fn)
            ms = {name: [] for name in arms}
            for _ in range(args.reps):
                for name, fn in arms.items():
                    ms[name].append(timed(fn, args.inner))
        need = 4.0 * n * (cin + cout) + 8.0 * e + 8.0 * n + 4.0 * cin * cout
        flop = 2.0 * n * cin * cout + 2.0 * (e + n) * cin
        lines.append(f"conv {cin} -> {cout} (ops.gcn_route: {ops.gcn_route(cin, cout)}); {need / 1e6:.1f} MB to move, {flop / 1e9:.2f} GFLOP")
        for name, v in ms.items():
            med = statistics.median(v)
            line = f"{name:>34} | {fmt(v)}"
            if name.startswith("(c)"):
                line += f" | {need / med / 1e6:8.1f} GB/s of the bytes it must move, {flop / med / 1e9:6.2f} TFLOP/s"
            lines.append(line)
    if args.script:
        lines.append("neurips4_GCN.py unmodified at its own size (r = 1, s = 421), ntrain = 2, two epochs of two steps:")
        lines.append(f"{'native':>34} | {script_epoch_seconds(False)}")
        lines.append(f"{'composite':>34} | {script_epoch_seconds(True)}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
