"""Time the any-width per-edge-weight operator (csrc/gpde_weconv_any.hip) - developer probe, nothing gates on it.

    python scripts/time_weconv_any.py [--out profiles/weconv_any_widths.txt] [--sizes 31,61] [--iters 20]

For each Darcy graph (s x s lattice, r = 0.10) and each width (32 x 32, 64 x 64, 128 x 128, 64 -> 32) the forward
(gpde_nnconv_fwd_edgeweights_any) and the backward (gpde_nnconv_bwd_edgeweights_any: the per-edge kernel, the ordered grad_x sum,
grad_root / grad_bias) are called through the C ABI on preallocated tensors; the time is the HIP-event span of `iters` back-to-back
calls after 3 warm-up calls, divided by `iters` (a CALL time: launch gaps included).  Reported: ms per call, bytes of W_e moved per
second (forward E * in * out * 4 read once; backward the same read once + grad_W_e written once) and that rate's share of the
6.3 TB/s a float4 copy achieves on the MI355X.  At 64 x 64 the specialised kernels (gpde_weconv_kernel / gpde_weconv_bwd_kernel)
run on the SAME tensors in the same process, alternating with the general ones, as the yardstick.  A W_e smaller than the 256 MiB
last-level cache is flagged: its rate is not an HBM rate."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from graph_pde_amd import _lib, ops, synth

HBM_ACHIEVABLE = 6.3e12
WIDTHS = [(32, 32), (64, 64), (128, 128), (64, 32)]


def span_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="31,61")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_weconv_any.py needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    st = ops._stream_ptr(dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; ms per CALL (HIP events over {args.iters} calls after 3 warm-up calls); "
             f"rate = bytes of W_e moved / time; share of {HBM_ACHIEVABLE / 1e12:.1f} TB/s (achievable HBM rate)"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for s in [int(v) for v in args.sizes.split(",")]:
        ei, ea, n = synth.darcy_graph(s, 0.10, device=dev)
        csr = ops.csr_for(ei, n)
        e = csr.n_edges
        srp, ssl = csr.src_order
        emit(f"graph s={s}: N={n} E={e} mean in-degree {e / n:.1f} max {csr.max_in_degree}")
        for cin, cout in WIDTHS:
            torch.manual_seed(0)
            x, g = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
            we = torch.empty(e, cin * cout, device=dev).uniform_(-0.1, 0.1)
            gwe = torch.empty_like(we)
            root, bias = torch.randn(cin, cout, device=dev) / 8, torch.randn(cout, device=dev)
            out, gx = torch.empty(n, cout, device=dev), torch.empty(n, cin, device=dev)
            groot, gbias = torch.empty(cin, cout, device=dev), torch.empty(cout, device=dev)
            ws = torch.empty(int(lib.gpde_nnconv_bwd_edgeweights_any_workspace_bytes(n, e, cin, cout)), dtype=torch.uint8, device=dev)
            nbytes = e * cin * cout * 4
            note = "  [W_e fits the 256 MiB last-level cache: not an HBM rate]" if nbytes < (256 << 20) else ""

            def fwd_any():
                _lib.check(lib.gpde_nnconv_fwd_edgeweights_any(x.data_ptr(), n, we.data_ptr(), e, csr.rowptr.data_ptr(), csr.src.data_ptr(),
                                                               root.data_ptr(), bias.data_ptr(), None, 0, _lib.GPDE_AGGR_MEAN, cin, cout,
                                                               out.data_ptr(), st), "fwd_any")

            def bwd_any():
                _lib.check(lib.gpde_nnconv_bwd_edgeweights_any(x.data_ptr(), n, we.data_ptr(), e, csr.rowptr.data_ptr(), csr.src.data_ptr(),
                                                               srp.data_ptr(), ssl.data_ptr(), root.data_ptr(), _lib.GPDE_AGGR_MEAN, cin, cout,
                                                               g.data_ptr(), gx.data_ptr(), gwe.data_ptr(), groot.data_ptr(), gbias.data_ptr(),
                                                               ws.data_ptr(), ws.numel(), st), "bwd_any")

            def report(tag, ms, moved):
                rate = moved / (ms * 1e-3)
                emit(f"  {cin:>3} -> {cout:<3} {tag:<22} {ms:9.4f} ms  {moved / 2**20:10.1f} MiB  {rate / 1e12:6.3f} TB/s  "
                     f"{100 * rate / HBM_ACHIEVABLE:5.1f} %{note}")

            if (cin, cout) != (64, 64):
                report("forward  (any-width)", span_ms(fwd_any, args.iters), nbytes)
                report("backward (any-width)", span_ms(bwd_any, args.iters), 2 * nbytes)
            else:
                desc = (_lib.GpdeWeConvDesc * 1)()
                d = desc[0]
                d.x, d.edge_weights, d.rowptr, d.src = x.data_ptr(), we.data_ptr(), csr.rowptr.data_ptr(), csr.src.data_ptr()
                d.root, d.bias, d.residual, d.out = root.data_ptr(), bias.data_ptr(), None, out.data_ptr()
                d.n_nodes, d.aggr, d.relu, d.reserved = n, _lib.GPDE_AGGR_MEAN, 0, 0
                ws64 = torch.empty(int(lib.gpde_nnconv_bwd_edgeweights_workspace_bytes(n, e)), dtype=torch.uint8, device=dev)

                def fwd_64():
                    _lib.check(lib.gpde_nnconv_fwd_edgeweights_group(desc, 1, st), "fwd_64")

                def bwd_64():
                    _lib.check(lib.gpde_nnconv_bwd_edgeweights(x.data_ptr(), n, we.data_ptr(), e, csr.rowptr.data_ptr(), csr.src.data_ptr(),
                                                               srp.data_ptr(), ssl.data_ptr(), root.data_ptr(), _lib.GPDE_AGGR_MEAN, g.data_ptr(),
                                                               gx.data_ptr(), gwe.data_ptr(), groot.data_ptr(), gbias.data_ptr(), ws64.data_ptr(),
                                                               ws64.numel(), st), "bwd_64")
                # alternating: general, specialised, general, specialised - the two of each kind show the spread
                for rep in range(2):
                    report(f"forward  (any-width) #{rep}", span_ms(fwd_any, args.iters), nbytes)
                    report(f"forward  (64-wide)   #{rep}", span_ms(fwd_64, args.iters), nbytes)
                for rep in range(2):
                    report(f"backward (any-width) #{rep}", span_ms(bwd_any, args.iters), 2 * nbytes)
                    report(f"backward (64-wide)   #{rep}", span_ms(bwd_64, args.iters), 2 * nbytes)
            del we, gwe, ws
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
