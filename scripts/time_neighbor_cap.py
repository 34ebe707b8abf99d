"""Developer probe of the capped in-degree (ops.radius_csr(..., max_num_neighbors=k), gpde_select.hip) on the headline graph: the
s x s lattice at radius r (s = 241, r = 0.10: 58,081 points, 95.5 M edges) capped to k = 64 in-edges, both modes.  HIP events
around each piece, one warm-up, `--reps` repetitions with the pieces alternating; median [min .. max] are printed:
    build      ops.radius_csr(pos, r) - the uncapped build, the same calls as before the cap existed;
    capped     ops.radius_csr(pos, r, max_num_neighbors=k, select=mode) - build + key + select + the gathers of src / dst;
    key        the key pass alone (gpde_edge_keys_sqdist / gpde_edge_keys_hash);
    select     gpde_csr_select_k alone, on a given rowptr_out.
Traffic the two passes must move, for orientation: the key pass writes 8 B per input edge (and reads the two int32 ids), the
select pass reads those 8 B and writes 4 B per kept edge; achieved bytes/s are reported against that.
usage: time_neighbor_cap.py [--s 241] [--r 0.1] [--k 64] [--reps 5] [--out profiles/neighbor_cap.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from graph_pde_amd import _lib, ops, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=241)
    ap.add_argument("--r", type=float, default=0.10)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: there is no CPU figure"
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    pos = synth.lattice_positions(args.s, dev)
    k = args.k

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    full = ops.radius_csr(pos, args.r)
    e = full.n_edges
    rp = full.rowptr.long()
    rowptr_out64 = torch.zeros(full.n_nodes + 1, dtype=torch.int64, device=dev)
    torch.cumsum((rp[1:] - rp[:-1]).clamp(max=k), 0, out=rowptr_out64[1:])
    e_new = int(rowptr_out64[-1])
    rowptr_out = rowptr_out64.to(torch.int32)
    slots = torch.empty(e_new, dtype=torch.int32, device=dev)
    keys = {"nearest": ops.edge_sqdist_keys(full, pos), "random": ops.edge_hash_keys(full.src, full.dst, 0)}

    def select_alone(mode):
        with torch.cuda.device(dev):
            _lib.check(lib.gpde_csr_select_k(full.rowptr.data_ptr(), keys[mode].data_ptr(), full.n_nodes, e, k, rowptr_out.data_ptr(),
                                             slots.data_ptr(), e_new, ops._stream_ptr(dev)), "gpde_csr_select_k")

    pieces = {"build": lambda: ops.radius_csr(pos, args.r)}
    for mode in ("nearest", "random"):
        pieces[f"capped {mode}"] = lambda mode=mode: ops.radius_csr(pos, args.r, max_num_neighbors=k, select=mode)
        pieces[f"select {mode}"] = lambda mode=mode: select_alone(mode)
    pieces["key nearest"] = lambda: ops.edge_sqdist_keys(full, pos)
    pieces["key random"] = lambda: ops.edge_hash_keys(full.src, full.dst, 0)
    for fn in pieces.values():                       # warm-up of every piece
        timed(fn)
    capped = ops.radius_csr(pos, args.r, max_num_neighbors=k)
    assert capped.n_edges == e_new and capped.max_in_degree == k
    ms = {name: [] for name in pieces}
    for _ in range(args.reps):
        for name, fn in pieces.items():
            ms[name].append(timed(fn)[0])
    lines = [f"scripts/time_neighbor_cap.py --s {args.s} --r {args.r} --k {k} --reps {args.reps}: {torch.cuda.get_device_name(0)}",
             f"{full.n_nodes} points, {e} edges (largest in-degree {full.max_in_degree}) -> {e_new} kept edges at k = {k}",
             "ms between HIP events, one warm-up, median [min .. max] over the repetitions, the pieces alternating"]
    for name, v in ms.items():
        med = statistics.median(v)
        line = f"{name:>16} | {med:>9.3f} [{min(v):>8.3f} .. {max(v):>8.3f}] ms"
        if name.startswith("key"):
            line += f" | {8.0 * e / med / 1e6:8.1f} GB/s of keys written, {16.0 * e / med / 1e6:8.1f} GB/s with the ids read"
        if name.startswith("select"):
            line += f" | {(8.0 * e + 4.0 * e_new) / med / 1e6:8.1f} GB/s (keys read once + kept slots written)"
        lines.append(line)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
