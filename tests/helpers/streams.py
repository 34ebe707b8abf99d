"""Stream tools of tests/test_gpu_streams.py (DESIGN.md "Streams").

`hold(stream, ms)` keeps a stream busy with a spinning kernel (torch.cuda._sleep) so that everything queued on it afterwards
starts late - the window in which another stream could read what has not been written yet.  `zeroed_pool(stream, ...)` leaves
the caching allocator's free blocks of that stream zero-filled, so that a buffer allocated there and read too early holds
zeros: a wrong number, and - should a test ever be wrong about what it races - a valid index.  Nothing here provokes a fault:
the racing tests race float buffers only (see the safety rule at the top of the test file)."""
import time

import torch

# The holds of the racing tests, from host times measured on the MI355X at the commit before the stream contract existed (a
# time.perf_counter difference around the racing sequence, no device synchronisation inside); a hold is at least ten times the
# slowest sequence it covers (a noisy shared host).
#   * cross-stream hits, entry points on a side stream: the slowest sequence was the GCN normalisation built and hit through
#     ops.gcn_norm, 4.60 ms (the module cases 0.27 - 2.56 ms); every entry point of the table issued in 0.04 - 0.29 ms.
#   * eviction under a queued reader: 103.3 ms for the slowest case (pack_mlp) and 74 - 79 ms for the others - the sequence contains
#     gc.collect(), a full collection of a process that has imported torch and pytest.
# Every racing test asserts that its window was still open after its last call was issued, whatever these numbers say.
ISSUE_MS_MEASURED, HOLD_MS = 4.60, 100.0
ISSUE_EVICT_MS_MEASURED, HOLD_EVICT_MS = 103.3, 1100.0

_cycles_per_ms = None


def cycles_per_ms() -> float:
    """Spin cycles of torch.cuda._sleep per millisecond, measured once per process with two events around a short sleep."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(100_000)                       # (the kernel's first launch loads its code object)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20_000_000
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        _cycles_per_ms = n / max(a.elapsed_time(b), 1e-3)
    return _cycles_per_ms


def hold(stream: torch.cuda.Stream, ms: float = HOLD_MS) -> torch.cuda.Event:
    """Keep `stream` busy for about `ms`; the event returned is recorded after that work (`not event.query()`: still held)."""
    cycles = int(cycles_per_ms() * ms)
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        done.record(stream)
    return done


def zeroed_pool(stream: torch.cuda.Stream, small: int = 48, large: int = 64 << 20, also=()):
    """After this the next allocations on `stream` come from zero-filled memory: the allocator's cache is emptied, then one block
    of `large` bytes (larger than everything the case allocates) and `small` sub-megabyte blocks (the allocator keeps small and
    large blocks in separate pools) are allocated, zeroed and freed under `stream`.  `also`: further streams whose pools are
    prepared the same way - a stream that finds its blocks cached asks the driver for nothing while another stream is held."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    for s in (stream,) + tuple(also):
        with torch.cuda.stream(s):
            blocks = [torch.zeros(large, dtype=torch.uint8, device="cuda")]
            blocks += [torch.zeros(256 << 10, dtype=torch.uint8, device="cuda") for _ in range(small)]
            blocks += [torch.zeros(2048, dtype=torch.uint8, device="cuda") for _ in range(small)]
            del blocks
    torch.cuda.synchronize()


def runs_while_held(held: torch.cuda.Stream, other: torch.cuda.Stream, ms: float = 20.0) -> bool:
    """Whether work queued on `other` executes while `held` is busy.  Two streams can share a hardware queue (the runtime maps
    its streams onto GPU_MAX_HW_QUEUES of them), and the queue runs them in order: a racing test on such a pair sees no race
    whatever the library does.  Harmless work only: a spin on `held`, one zero-fill of a float on `other`."""
    buf = torch.empty(64, device="cuda")
    torch.cuda.synchronize()
    done = hold(held, ms)
    with torch.cuda.stream(other):
        buf.zero_()
        ev = torch.cuda.Event()
        ev.record(other)
    ev.synchronize()
    free = not done.query()
    torch.cuda.synchronize()
    return free


def stream_beside(held: torch.cuda.Stream, tries: int = 8) -> torch.cuda.Stream:
    """A pool stream whose work runs while `held` is busy (`runs_while_held`)."""
    for _ in range(tries):
        s = torch.cuda.Stream()
        if s != held and runs_while_held(held, s):
            return s
    raise AssertionError(f"none of {tries} pool streams ran beside the held stream: the racing tests cannot see a race on this machine")


def stream_pair():
    """(A, B): two pool streams, B running while A is held and A while B is held."""
    a = torch.cuda.Stream()
    for _ in range(8):
        b = stream_beside(a)
        if runs_while_held(b, a):
            return a, b
    raise AssertionError("no pair of pool streams that run beside each other")


class IssueTimer:
    """Host time spent issuing a racing sequence (no device synchronisation inside): `with IssueTimer() as t: ...; t.ms`."""

    def __enter__(self):
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        self.ms = (time.perf_counter() - self.t0) * 1e3
        return False


# ---------------------------------------------------------------------------------------------------------------------------
# the side-stream table (tests/test_gpu_streams.py::test_entry_point_on_a_side_stream) and what it leaves out, by name: every
# public function of ops.py from which a launch of libgpde.so can be reached is in one of the two (tests/test_streams_host.py)
# ---------------------------------------------------------------------------------------------------------------------------
SIDE_STREAM_TABLE = (
    "nnconv_forward_raw", "nnconv_forward_nodeattr_raw", "nnconv_forward_per_edge_raw", "nnconv_backward_raw",
    "nnconv_backward_light_raw", "nnconv_backward_deferred_raw", "hidden_forward_raw", "nnconv_forward_hidden_raw",
    "nnconv_forward_mixed_raw", "edge_weights_raw", "nnconv_forward_edgeweights_raw", "nnconv_forward_edgeweights_group",
    "nnconv_backward_edgeweights_raw", "edge_weights_backward_raw", "nnconv_backward_hidden_raw", "hidden_backward_raw", "gather_rows",
    "nnconv_forward_edgeweights_any_raw", "nnconv_backward_edgeweights_any_raw", "nnconv_forward_hidden_any_raw",
    "nnconv_backward_hidden_any_raw", "nnconv_forward_edgeweights_bip_raw", "nnconv_backward_edgeweights_bip_raw",
    "nnconv_forward_hidden_bip_raw", "nnconv_backward_hidden_bip_raw", "diagconv_forward_raw", "diagconv_backward_raw",
    "gcn_forward_raw", "gcn_norm", "edge_sqdist_keys", "edge_hash_keys",
)
_BUILDER = ("graph builder: count, read-back and fill passes - its fill kernels write by the counts, and a test that raced its "
            "producers could write out of bounds; it synchronises the host by design")
EXCLUDED = {
    "build_csr": _BUILDER,
    "csr_for": "the CSR cache over build_csr (" + _BUILDER + "); its cross-stream bookkeeping is test 3 of the GPU file",
    "radius_graph": _BUILDER,
    "radius_csr": _BUILDER,
    "radius_csr_raw": _BUILDER,
    "radius_in_degrees": _BUILDER,
    "radius_csr_batched": _BUILDER,
    "radius_graph_batched": _BUILDER,
    "multilevel_radius_graphs": _BUILDER,
    "select_in_edges": "neighbour cap: " + _BUILDER,
    "pack_mlp": "a cache, not an operator: raced as a float cache in tests 1 and 2 of the GPU file",
    "attr_in_slot_order": "a cache, not an operator: raced as a float cache in test 1 of the GPU file (its identity probe "
                          "synchronises by design)",
}
