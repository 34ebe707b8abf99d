"""GPU tier: `gp.capture` - a model function's native calls recorded into one HIP graph (graph-pde_amd/capture.py).

The MGKN V-cycles (/root/reference/multipole-graph-neural-operator/MGKN_orthogonal_burgers1d.py:65-82,
MGKN_general_darcy2d.py:76-90) are 52 / 65 unmodified module calls per forward whose GPU work is shorter than the time the
host needs to issue them.  Recorded once and replayed, the SAME kernels run with the same arguments: results must be the bits
of the direct call, for new inputs as well, and stay so after an in-place weight update."""
import pytest
import torch

import graph_pde_amd as gp
from graph_pde_amd import _lib, hidden_cache, mgkn_workloads

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(mgkn_workloads.WORKLOADS))
def test_captured_mgkn_forward_is_bitwise_the_direct_calls(name):
    d = torch.device("cuda:0")
    hidden_cache.clear()
    wl = mgkn_workloads.WORKLOADS[name](d)
    for _ in range(3):
        ref = [t.clone() for t in wl.forward()]           # the default policy has settled (per-edge weight cache built)
    cap = gp.capture(wl.forward)
    calls = _lib.n_native_calls
    out = cap()
    torch.cuda.synchronize()
    assert _lib.n_native_calls == calls                   # a replay issues no native call from the host
    assert len(out) == len(ref) and all(torch.equal(a, b) for a, b in zip(out, ref))
    out2 = [t.clone() for t in cap()]
    assert all(torch.equal(a, b) for a, b in zip(out2, ref)) and cap.replays == 2
    # an in-place weight update (what an optimizer step does) is seen by the replay: compare with fresh direct calls
    with torch.no_grad():
        for m in wl.modules:
            for p in m.parameters():
                p.mul_(1.01)
    # the OLD recording replayed after the update.  Its packed weights / H / W_e were derived from the old values:
    # the replay notices the moved version counters and records again first - the result is the direct call's for the NEW weights
    assert cap.stale() and cap.recordings == 1
    out3 = [t.clone() for t in cap()]
    assert cap.recordings == 2 and not cap.stale()
    for _ in range(3):
        ref2 = [t.clone() for t in wl.forward()]           # (the caches rebuild for the new weight versions and settle again)
    assert all(torch.equal(a, b) for a, b in zip(out3, ref2))
    cap2 = gp.capture(wl.forward)                          # an explicit new recording agrees
    assert all(torch.equal(a, b) for a, b in zip(cap2(), ref2))
    assert not torch.equal(ref2[0], ref[0])


@pytest.mark.parametrize("name", sorted(mgkn_workloads.WORKLOADS))
def test_a_recording_keeps_the_cached_buffers_it_reads_alive(name):
    """the recorded kernels read CSR arrays, slot-ordered attributes, packed weights and cached H / W_e at the
    addresses they had at recording time, and only the library's caches owned them.  Everything that empties those caches -
    a second capture (hidden_cache.clear), release_all under memory pressure, ops.clear_caches - followed by allocations that
    would recycle the freed blocks must leave the first recording's replays unchanged."""
    from graph_pde_amd import ops
    d = torch.device("cuda:0")
    hidden_cache.clear()
    wl = mgkn_workloads.WORKLOADS[name](d)
    for _ in range(3):
        ref = [t.clone() for t in wl.forward()]
    cap = gp.capture(wl.forward, copy_outputs=True)
    assert all(torch.equal(a, b) for a, b in zip(cap(), ref))
    wl_b = mgkn_workloads.WORKLOADS[name](d)               # another model + another recording alive beside the first
    cap_b = gp.capture(wl_b.forward, copy_outputs=True)
    ref_b = cap_b()
    hidden_cache.release_all()
    hidden_cache.clear()
    ops.clear_caches()
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    junk = [torch.full((1 << 26,), float("nan"), device=d) for _ in range(8)]      # 2 GiB of NaN over whatever was freed
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(cap(), ref))
    assert all(torch.equal(a, b) for a, b in zip(cap_b(), ref_b))
    del junk


def test_captured_call_takes_new_inputs_and_checks_shapes():
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    n, e = 300, 6000
    ei = torch.stack([torch.randint(0, n, (e,)), torch.randint(0, n, (e,))]).to(d)
    ea = torch.randn(e, 6, device=d)
    mlp = torch.nn.Sequential(torch.nn.Linear(6, 64), torch.nn.ReLU(), torch.nn.Linear(64, 128), torch.nn.ReLU(), torch.nn.Linear(128, 4096))
    conv = gp.NNConv_old(64, 64, mlp, aggr="mean").to(d)

    def model(x):
        with torch.no_grad():
            for _ in range(3):
                x = torch.relu(conv(x, ei, ea))
            return x
    x0, x1 = torch.randn(n, 64, device=d), torch.randn(n, 64, device=d)
    cap = gp.capture(model, x0, copy_outputs=True)
    y0, y1 = cap(x0), cap(x1)
    assert torch.equal(y0, model(x0)) and torch.equal(y1, model(x1)) and not torch.equal(y0, y1)
    with pytest.raises(ValueError):
        cap(torch.randn(n + 1, 64, device=d))
    with pytest.raises(ValueError):
        gp.capture(model, x0.cpu())


@pytest.mark.parametrize("name,twin_between", [pytest.param(n, False, id=n) for n in sorted(mgkn_workloads.WORKLOADS)] +
                         [pytest.param("mgkn_orthogonal_burgers1d", True, id="mgkn_orthogonal_burgers1d-twin_between")])
def test_captured_training_step_follows_the_direct_steps(name, twin_between):
    """A whole optimisation step (forward with autograd, loss, native backward of every call, Adam with its step count on the
    device) recorded once: four replays leave the weights where four direct steps of a twin model leave them (to the summation-order
    level) with the same losses, and a DIRECT forward afterwards sees the updated weights (the replay drops the host-side caches).
    `twin_between`: the twin's direct steps run between the recording and the first replay instead of in front of both."""
    d = torch.device("cuda:0")
    hidden_cache.clear()
    wl_a = mgkn_workloads.WORKLOADS[name](d, capturable=True)
    wl_b = mgkn_workloads.WORKLOADS[name](d, capturable=True)
    for ma, mb in zip(wl_a.modules, wl_b.modules):
        mb.load_state_dict(ma.state_dict())
    warm = 3
    # the twin's direct steps in front of the recording, or between the recording and its first replay.  (Round 6 saw the first replay
    # return another loss in the second order - 59.3 for 72.9 - and left it unexplained; run again in that order later (DESIGN.md
    # §6h), the replays gave the direct steps' losses to the last digit, and the order became a case of this test.)
    def twin_steps():
        lb_warm = [float(wl_b.train_step().detach()) for _ in range(warm)]
        assert len(lb_warm) == warm
        return [float(wl_b.train_step().detach()) for _ in range(4)]
    if not twin_between:
        lb = twin_steps()
        torch.cuda.synchronize()
    cap = gp.capture(wl_a.train_step, warmup=warm, updates_parameters=True)          # (recording executes nothing: 3 steps so far)
    if twin_between:
        torch.cuda.synchronize()
        lb = twin_steps()
        torch.cuda.synchronize()
    calls = _lib.n_native_calls
    la = []
    for _ in range(4):
        loss = cap()
        la.append(float(loss.detach()))
    torch.cuda.synchronize()
    assert _lib.n_native_calls == calls and torch.isfinite(loss)
    print(name, "losses captured", la, "direct", lb)
    worst = 0.0
    for pa, pb in zip([p for m in wl_a.modules for p in m.parameters()], [p for m in wl_b.modules for p in m.parameters()]):
        worst = max(worst, float((pa - pb).abs().max() / pb.abs().max().clamp_min(1e-30)))
    # (the recorded step froze ONE settled call sequence; the twin's direct steps pass through the cache policies again after every
    # weight update - first call of a forward direct, later ones on the shared nodes - i.e. other summation orders at the 1e-7 level,
    # which four Adam steps carry to ~2e-6 of the weights: same arithmetic class, not the same bits)
    assert worst <= 1e-5, (worst, la, lb)
    assert all(abs(a - b) <= 1e-4 * abs(b) for a, b in zip(la, lb)), (la, lb)
    ya, yb = wl_a.forward(), wl_b.forward()
    assert all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(ya, yb))
