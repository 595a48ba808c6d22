"""v3 pipelined fused MLP step (csrc/mlp_step3.hip) and the FusedMLPEngine.

The GPU tests check, step by step across epoch boundaries, that the gradients
the v3 kernels produce equal a bf16-rounding emulation of the fp32 math on the
batch that DistributedSampler semantics select -- which exercises the whole
pipeline: layer-1 pre-activations computed by the previous step's tail from its
freshly updated W1 tile, the X-tile ring, the double-buffered epoch order and
the device counters.  CPU tests cover the engine's reference path.
"""
import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices
import mlp_reference
from helpers import update_worst

gpu = pytest.mark.gpu


def _rel(a, b):
    return (a.float() - b.float()).norm().item() / max(b.float().norm().item(), 1e-12)


def _bf(x):
    return x.to(torch.bfloat16).float()


def _fixed_h1pre(X, W1b):
    """X . W1^T as the kernels sum it: 49 16-pixel tile partials, each rounded to the
    12.20 fixed point of csrc/mlp_step3.hip (saturating at +-32), added exactly."""
    xt = X.double().view(X.size(0), 49, 16)
    wt = W1b.double().view(W1b.size(0), 49, 16)
    part = torch.einsum("bti,mti->tbm", xt, wt).float().double()  # fp32 MFMA partials
    q = torch.round(part * 2.0 ** 20).clamp(-(2.0 ** 25), 2.0 ** 25)
    return (q.sum(0) / 2.0 ** 20).float()


def _emulate_bf16_grads(params, x, y, L1, L2, B):
    p = fused_mlp.mlp_unpack(params.cpu(), L1, L2)
    W1, b1, W2, b2, W3, b3 = [p[k] for k in p]
    X = _bf(x)
    h1 = _bf(torch.relu(_fixed_h1pre(X, _bf(W1)) + b1))
    h2 = _bf(torch.relu(h1 @ _bf(W2).T + b2))
    z = h2 @ _bf(W3).T + b3
    pr = torch.softmax(z, 1)
    dz = _bf((pr - F.one_hot(y, 10).float()) / B)
    dh2 = _bf((dz @ _bf(W3)) * (h2 > 0))
    dh1 = _bf((dh2 @ _bf(W2)) * (h1 > 0))
    g = [dh1.T @ X, dh1.sum(0), dh2.T @ h1, dh2.sum(0), dz.T @ h2, dz.sum(0)]
    return torch.cat([t.reshape(-1) for t in g])


@gpu
def test_mlp3_h1_copies_mirror():
    """The Python buffer sizing mirrors the kernels' H1pre copy count."""
    from ray_lightning_accelerators_amd import ops

    for L1 in (32, 64, 128):
        assert ops.require().mlp3_h1_copies(L1) == fused_mlp.mlp3_h1_copies(L1)


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=g)
    return x, y


# ------------------------------------------------------------------ CPU path
def test_engine_reference_order_and_counters():
    """CPU engine: batches follow the per-epoch DistributedSampler order across epochs."""
    x, y = _data(100)
    B = 16
    eng = FusedMLPEngine(32, 32, B, lr=1e-3, world_size=2, rank=1, allreduce=lambda g: g.mul_(2))
    eng.set_data(x, y)
    nb = eng.n_batches
    assert nb == 50 // B
    seen = []
    for _ in range(2 * nb + 1):
        seen.append((eng.epoch, int(eng.counters[1]), int(eng.counters[4])))
        eng.step()
    assert seen[0] == (0, 0, 0) and seen[nb] == (1, 0, 1) and seen[2 * nb] == (2, 0, 0)
    assert eng.counters[0].item() == 2 * nb + 1
    # buffer 1 now holds epoch 3's order (filled when epoch 2 began)
    want = shard_indices(100, 2, 1, 3, 0, True)[: nb * B]
    assert torch.equal(eng.order[1].cpu(), want)


def test_engine_reference_world2_matches_world1():
    """Split path (grads -> allreduce(SUM of 2 identical ranks) -> Adam/2) == fused path."""
    x, y = _data(200, seed=3)
    a = FusedMLPEngine(32, 64, 32, lr=1e-2)
    b = FusedMLPEngine(32, 64, 32, lr=1e-2, allreduce=lambda g: g.mul_(2))
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2  # after set_data: same shard, split optimizer path (< 2 epochs below)
    for _ in range(5):
        a.step()
        b.step()
    assert torch.allclose(a.params, b.params, atol=1e-6)


def test_engine_reference_converges():
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    x, y = synthetic_mnist(1024, seed=0)
    eng = FusedMLPEngine(32, 64, 32, lr=1e-3)
    eng.set_data(x, y)
    eng.run(120)
    assert eng.recent_stats(10)[:, 0].mean() < 1.0


# ------------------------------------------------------------------ GPU path
def _assert_same(pa, pb):
    """The v3 step is bitwise reproducible: the 49-way layer-1 split-K sum uses
    12.20 fixed-point integer atomics (order-independent), everything else a
    fixed reduction order."""
    d = (pa - pb).abs()
    assert torch.equal(pa, pb), (d.max().item(), (d > 0).float().mean().item())


def _dev():
    return torch.device("cuda", 0)


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (32, 32, 20), (64, 128, 64), (128, 256, 100),
                                     (128, 64, 256), (64, 256, 48)])
def test_mlp3_pipeline_grads_vs_emulation(L1, L2, B):
    """Per step across 2+ epochs: v3 gradients == bf16 emulation on the expected batch."""
    dev = _dev()
    n_data = 3 * B + B // 2
    x, y = _data(n_data, seed=L1 + L2 + B)
    captured = []

    def allreduce(g):
        captured.append(g.detach().cpu().clone())
        g.mul_(2)  # two identical ranks

    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, device=dev, world_size=2, rank=0, allreduce=allreduce)
    eng.set_data(x, y)
    nb = eng.n_batches
    steps = 2 * nb + 2
    for s in range(steps):
        epoch, cur = eng.epoch, eng.step_in_epoch
        p_before = eng.params.detach().cpu().clone()
        eng.step()
        torch.cuda.synchronize()
        idx = shard_indices(n_data, 2, 0, epoch, 0, True)[cur * B:(cur + 1) * B]
        emu = _emulate_bf16_grads(p_before, x[idx].float() / 255.0, y[idx], L1, L2, B)
        err = _rel(captured[-1][: emu.numel()], emu)  # the comm bucket is padded to 16 B
        assert err < 2e-2, (s, err)
    assert eng.counters[0].item() == steps


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (64, 128, 64), (128, 256, 128), (32, 32, 48)])
def test_mlp3_fused_matches_split(L1, L2, B):
    """World-size-1 fused step == head + tail(grad) + allreduce + tail(adam) (identical ranks)."""
    dev = _dev()
    n_data = 8 * B
    x, y = _data(n_data, seed=7)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, device=dev)
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, device=dev, allreduce=lambda g: g.mul_(2))
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2  # after set_data: same shard, split optimizer path (6 steps < 2 epochs)
    for _ in range(6):
        a.step()
        b.step()
    torch.cuda.synchronize()
    # different Adam code paths (fused epilogues vs post-allreduce kernel), one adam1
    # (csrc/mlp_common.h: explicit FMAs, no contraction) on the same fp32 gradient --
    # 2 g / 2 is exact -- so both routes write the same bits
    # (tests/test_mlp3_stages_fp64.py::test_split_route_gradients holds the gradient itself)
    assert torch.equal(a.params, b.params), (a.params - b.params).abs().max()
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    for e in (a, b):
        ref = torch.zeros_like(e.shadow)
        fused_mlp.mlp_refresh_shadow(e.params, ref, L1, L2)
        torch.cuda.synchronize()
        lay = fused_mlp.mlp_shadow_layout(L1, L2)
        assert torch.equal(e.shadow[: lay["np"]], ref[: lay["np"]])
        assert torch.equal(e.shadow[lay["w2t"]:], ref[lay["w2t"]:])


@gpu
@pytest.mark.parametrize("L1,L2,B", [(128, 256, 128), (32, 64, 100), (64, 128, 256)])
def test_mlp3_multiblock_head_stats(L1, L2, B):
    """Batches above 32 rows run one head workgroup per 32 rows; the step's loss /
    correct / count (reduced by tail block 0 in block order) match an fp32 forward
    of the consumed batch, and are identical across repeated runs."""
    import torch.nn.functional as F

    dev = _dev()
    n_data = 4 * B
    x, y = _data(n_data, seed=B)
    runs = []
    for _ in range(2):
        eng = FusedMLPEngine(L1, L2, B, lr=1e-2, device=dev)
        eng.set_data(x, y)
        rows = []
        for s in range(5):
            epoch, cur = eng.epoch, eng.step_in_epoch
            p_before = eng.params.detach().cpu().clone()
            eng.step()
            torch.cuda.synchronize()
            idx = shard_indices(n_data, 1, 0, epoch, 0, True)[cur * B:(cur + 1) * B]
            pv = fused_mlp.mlp_unpack(p_before, L1, L2)
            h = torch.relu(F.linear(x[idx].float() / 255.0, pv["layer_1.weight"], pv["layer_1.bias"]))
            h = torch.relu(F.linear(h, pv["layer_2.weight"], pv["layer_2.bias"]))
            logp = F.log_softmax(F.linear(h, pv["layer_3.weight"], pv["layer_3.bias"]), dim=1)
            st = eng.recent_stats(1)[0]
            assert int(st[2]) == B and int(st[3]) == s + 1, st
            assert abs(float(st[0]) - float(F.nll_loss(logp, y[idx]))) < 3e-2 * max(1.0, float(st[0])), (s, st)
            assert abs(int(st[1]) - int((logp.argmax(1) == y[idx]).sum())) <= max(2, B // 25), (s, st)
            rows.append(st.clone())
        runs.append(torch.stack(rows))
    assert torch.equal(runs[0], runs[1])


def _one_vs_two(L1, L2, B, kinds, n_steps, seed=3):
    """Engine A runs the one-launch step (or the per-step kinds given), B the
    two-launch step; every state tensor must match bit for bit."""
    dev = _dev()
    x, y = _data(2 * B + B // 2 + 3, seed=seed)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, device=dev)
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, device=dev)
    b.one_launch = False
    a.set_data(x, y)
    b.set_data(x, y)
    for s in range(n_steps):
        a.one_launch = kinds(s)
        a.step()
        b.step()
    torch.cuda.synchronize()
    a.check()
    tn1, tn2 = L1 // 16, L2 // 16
    ntask = tn1 * tn2 + tn2 + (L1 + L2 + 10 + 63) // 64
    blocks = 1 + 49 + (ntask + 7) // 8
    assert int(a.hand[0]) == int(a.counters[10]) * blocks  # one acknowledgement per block per launch
    assert torch.equal(a.counters[:10].cpu(), b.counters[:10].cpu()), (a.counters, b.counters)
    w1 = L1 * 784
    for k in ("params", "exp_avg", "exp_avg_sq", "shadow", "stats", "h1pre", "xring"):
        pa, pb = getattr(a, k).float(), getattr(b, k).float()
        if k in ("params", "exp_avg", "exp_avg_sq"):
            bad = (pa != pb).nonzero().flatten().cpu()
            assert bad.numel() == 0, (k, bad.numel(), int((bad < w1).sum()), bad[:8].tolist(),
                                      (pa - pb).abs().max().item())
        _assert_same(pa, pb)
    return a


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (32, 32, 20), (128, 256, 32), (64, 128, 1), (128, 64, 17)])
def test_mlp3_one_launch_matches_two_launch(L1, L2, B):
    """The one-launch step (every block replays the head's chain, then does its
    tail share) is the same computation as head + tail: bitwise-equal over 2+ epochs."""
    a = _one_vs_two(L1, L2, B, lambda s: True, 7)
    assert int(a.counters[10]) == 7  # one sequence number per one-launch step


@gpu
def test_mlp3_one_launch_interleaves_with_two_launch():
    """The device state between steps is the same for both forms, so they mix
    freely (graph remainders, fallbacks): alternate them every step / every other."""
    _one_vs_two(32, 64, 32, lambda s: s % 2 == 0, 9)
    _one_vs_two(64, 128, 24, lambda s: s % 3 != 1, 9, seed=4)


@gpu
@pytest.mark.parametrize("nb,gsteps,remainders", [(5, 3, False), (5, 3, True), (7, 5, True)])
def test_mlp3_graph_replay_matches_eager(nb, gsteps, remainders):
    dev = _dev()
    # nb batches per epoch, gsteps steps per graph: replays, remainders (eager, or
    # replays of the 1/2/4-step graphs) and several epoch switches
    x, y = _data(32 * nb + 8, seed=5)
    a = FusedMLPEngine(32, 64, 32, lr=1e-3, device=dev)
    b = FusedMLPEngine(32, 64, 32, lr=1e-3, device=dev)
    a.set_data(x, y)
    b.set_data(x, y)
    assert b.capture(gsteps, remainders=remainders)
    assert sorted(b._tail_graphs) == ([k for k in (1, 2, 4) if k < gsteps] if remainders else [])
    a.run(1)  # capture() ran one real step
    a.run(23)
    for n in (6, 1, 9, 7):  # dispatches that are not multiples of gsteps
        b.run(n)
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 24
    assert torch.equal(a.counters.cpu(), b.counters.cpu())
    _assert_same(a.params, b.params)
    _assert_same(a.stats, b.stats)


@gpu
def test_mlp3_training_converges_and_tracks_reference():
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    x, y = synthetic_mnist(4096, seed=0)
    g = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev())
    c = FusedMLPEngine(32, 64, 32, lr=1e-3)
    g.set_data(x, y)
    c.set_data(x, y)
    g.capture(8)
    g.run(299)
    c.run(300)
    torch.cuda.synchronize()
    lg, lc = g.recent_stats(50)[:, 0].mean().item(), c.recent_stats(50)[:, 0].mean().item()
    assert lg < 0.5 and abs(lg - lc) < 0.1 * max(lc, 0.05), (lg, lc)


@gpu
def test_mlp3_reload_params_reprimes():
    """Params changed outside a step (load / broadcast) -> H1pre is recomputed."""
    dev = _dev()
    x, y = _data(256, seed=9)
    captured = []
    eng = FusedMLPEngine(32, 64, 32, lr=1e-2, device=dev, world_size=2,
                         allreduce=lambda gr: (captured.append(gr.cpu().clone()), gr.mul_(2)))
    eng.set_data(x, y)
    eng.run(3)
    newp = fused_mlp.init_mlp_params(32, 64, torch.Generator().manual_seed(123))
    eng.load_params(newp)
    epoch, cur = eng.epoch, eng.step_in_epoch
    eng.step()
    torch.cuda.synchronize()
    idx = shard_indices(256, 2, 0, epoch, 0, True)[cur * 32:(cur + 1) * 32]
    emu = _emulate_bf16_grads(newp, x[idx].float() / 255.0, y[idx], 32, 64, 32)
    assert _rel(captured[-1][: emu.numel()], emu) < 2e-2


def _loopback_ctx(world, L1=32, L2=64):
    """A world-1 communicator's aux region presented as `world` ranks that all live
    in this process (loopback: every region pointer is our own)."""
    from ray_lightning_accelerators_amd.parallel.comm import native_comm_module

    mod = native_comm_module()
    c = mod.Communicator(0, 1, 0)
    c.aux_open([c.aux_handle(fused_mlp.mlp3_dp_capacity(L1, L2))])
    ctx = [int(v) for v in c.aux_context()]
    return c, [world] + ctx[1:6] + [ctx[6]] * world


@gpu
@pytest.mark.parametrize("proto", ["packed", "owner"])
@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_mlp3_dp_loopback_tracks_single_rank(proto, world):
    """Loopback world-N (one process writes every rank's source slots, polls N
    granules per value, sums, and -- owner -- plays every owner): the exchange of N
    identical contributions averages back to this rank's own gradient, so the run
    follows the plain one-launch step up to the protocol's wire rounding (4 ulp of
    fp32 per value).  Exercises every in-kernel path of the N-rank exchange on one GPU."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    dev = _dev()
    x, y = synthetic_mnist(2048, seed=0)
    c, ctx = _loopback_ctx(world)
    lb = FusedMLPEngine(32, 64, 32, lr=1e-3, device=dev, dp_context=ctx, dp_proto=proto, dp_loop=True)
    ref = FusedMLPEngine(32, 64, 32, lr=1e-3, device=dev)
    assert lb.one_launch_dp and lb.dp_ctx[0] == world
    lb.set_data(x, y)
    ref.set_data(x, y)
    p0 = ref.params.clone()
    lb.run(1)
    ref.run(1)
    torch.cuda.synchronize()
    # one step: Adam's first update is ~lr * sign(g), blind to 2^-22 wire rounding
    d1 = (lb.params - ref.params).abs().max().item()
    assert d1 < 1e-6, d1
    lb.run(2)  # eager, then graph replays
    ref.run(2)
    assert lb.capture(8)
    ref.run(1)
    lb.run(96)
    ref.run(96)
    torch.cuda.synchronize()
    assert c.error_state() == 0, c.error_message()
    lb.check()
    # later steps: a rounding difference that flips one bf16 weight shadow perturbs
    # the next forward, so the runs separate slowly (as any two bf16 runs whose
    # inputs differ in the last fp32 bits do); bound the separation by the distance
    # travelled
    sep = (lb.params - ref.params).norm().item() / (ref.params - p0).norm().item()
    assert sep < 0.05, sep
    ll, lr_ = lb.recent_stats(20)[:, 0].mean().item(), ref.recent_stats(20)[:, 0].mean().item()
    assert abs(ll - lr_) < 0.02 * lr_ + 1e-3, (ll, lr_)


@gpu
def test_mlp3_dp_loopback_timeout_is_reported():
    """Rank 1 of a 2-rank packed exchange whose peer never runs: its polls give up
    after the bound and set the error word instead of hanging the GPU."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    dev = _dev()
    x, y = synthetic_mnist(512, seed=0)
    c, ctx = _loopback_ctx(2)
    ctx[1] = 1  # rank 1 of 2, not loopback: it waits for rank 0, which never runs
    c.set_spin_limit(1 << 12)
    ctx[3] = 1 << 12
    e = FusedMLPEngine(32, 64, 32, lr=1e-3, device=dev, world_size=2, rank=1, dp_context=ctx, dp_proto="packed")
    e.set_data(x, y)
    e.run(1)
    torch.cuda.synchronize()
    assert c.error_state() != 0
    c.reset_error()


# ------------------------------------------------- fp32 fidelity
_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
# Normwise relative error of each gradient tensor against fp32 autograd on the same
# batch, max over every step of 2+ epochs.  The kernels compute in bf16 (inputs,
# weights, activations and deltas rounded to 8 significant bits, fp32 accumulation),
# as stock PyTorch bf16 autocast does; the one-launch test measures autocast's own
# error on the same batches and holds the kernel to 1.5x of it (+0.01), and every
# test to these absolute ceilings (~1.7x the kernel's measured maxima, 32-64 model:
# W1 0.053, b1 0.091, W2 0.068, b2 0.068, W3 0.0055, b3 0.0065 -- profiles/r3_fidelity/)
GRAD_BOUND = {"W1": 0.1, "b1": 0.15, "W2": 0.12, "b2": 0.12, "W3": 0.015, "b3": 0.015}


def _autocast_grads(flat, x_u8, y, L1, L2, dev):
    """The stock bf16 path's gradient (nn.Linear under torch.autocast bf16, fp32
    params, fp32 log_softmax / NLL) -- the precision the reference runs at."""
    p = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in
         zip(_NAMES, fused_mlp.mlp_unpack(flat.detach().float(), L1, L2).values())}
    x = x_u8.to(dev).float() / 255.0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h = torch.relu(F.linear(x, p["W1"], p["b1"]))
        h = torch.relu(F.linear(h, p["W2"], p["b2"]))
        z = F.linear(h, p["W3"], p["b3"])
    F.nll_loss(torch.log_softmax(z.float(), 1), y.to(dev)).backward()
    return torch.cat([p[k].grad.reshape(-1) for k in _NAMES]).cpu()


def _fp32_ref_grads(flat, x_u8, y, L1, L2):
    """fp32 nn.Linear MLP + log_softmax + NLL (the reference model's math) at the
    flat parameters; returns the flat gradient (arena order)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in
         zip(_NAMES, fused_mlp.mlp_unpack(flat.detach().cpu().float(), L1, L2).values())}
    x = x_u8.float() / 255.0
    h = torch.relu(F.linear(x, p["W1"], p["b1"]))
    h = torch.relu(F.linear(h, p["W2"], p["b2"]))
    loss = F.nll_loss(torch.log_softmax(F.linear(h, p["W3"], p["b3"]), 1), y)
    loss.backward()
    return torch.cat([p[k].grad.reshape(-1) for k in _NAMES])


def _per_tensor_rel(g, ref, L1, L2):
    a = fused_mlp.mlp_unpack(g.cpu(), L1, L2)
    b = fused_mlp.mlp_unpack(ref.cpu(), L1, L2)
    return {k: _rel(x, y) for k, x, y in zip(_NAMES, a.values(), b.values())}


_STATE = ("params", "exp_avg", "exp_avg_sq", "shadow", "h1pre", "xring", "yring", "counters", "hand", "order")


def _snapshot(eng):
    """Clone of every device buffer a one-launch step reads (pre-step state)."""
    return {k: getattr(eng, k).clone() for k in _STATE}


def _h1pre_dense(h1pre_slot, L1, Bp=32):
    """[Bp, L1] fp64 view of one H1pre ring slot (12.20 fixed point, MFMA-fragment order)."""
    b = torch.arange(Bp).view(-1, 1)
    m = torch.arange(L1).view(1, -1)
    pos = (((b // 16) * (L1 // 16) + m // 16) * 4 + b % 4) * 64 + ((b % 16) // 4) * 16 + m % 16
    return h1pre_slot.cpu()[pos].double() / 2.0 ** 20  # 12.20 fixed point


def _pre_step_check(snap, x, y, idx, L1, L2, B, cur, epoch):
    """Which input of the coming step is inconsistent?  Every word the step reads is
    checked against what the engine's invariants say it must hold."""
    Bp = 32
    out = {}
    c = snap["counters"].cpu()
    slot = int(c[3])
    out["counters"] = c[:11].tolist()
    out["counters_ok"] = bool(torch.equal(c[0:5], c[5:10]) and int(c[1]) == cur and int(c[4]) == epoch % 2)
    yr = snap["yring"].view(2, Bp).cpu()[slot]
    out["yring_ok"] = bool(torch.equal(yr[:B].long(), y[idx]) and bool((yr[B:] == -1).all()))
    xr = snap["xring"].view(2, 49, Bp, 16).cpu()[slot].float().permute(1, 0, 2).reshape(Bp, 784)
    xe = (x[idx].float() * (1.0 / 255.0)).to(torch.bfloat16).float()
    out["xring_ok"] = bool(torch.equal(xr[:B], xe) and bool((xr[B:] == 0).all()))
    h1 = snap["h1pre"].view(2, fused_mlp.mlp3_h1_copies(L1), Bp * L1).sum(1)  # the copies add up
    cur_h = _h1pre_dense(h1[slot], L1)
    w1 = snap["shadow"][: L1 * 784].view(L1, 784).cpu().double()
    ref_h = xe.double() @ w1.T
    out["h1pre_rel_err"] = float((cur_h[:B] - ref_h).norm() / max(ref_h.norm(), 1e-30))
    # element by element: tests/mlp_reference.py's layer-1 rule (49 2^-21 + sum_tiles 32 U24 amp_tile)
    try:
        c = mlp_reference.cmp_bound(cur_h[:B], *mlp_reference.ref_layer1(xe.double(), w1))
        out["h1pre_elementwise_ok"], out["h1pre_worst_err_over_bound"], out["h1pre_elementwise"] = c.ok, c.ratio, c.detail
    except AssertionError as e:  # weights whose tile partials reach the clamp: the rule does not apply
        out["h1pre_elementwise_ok"], out["h1pre_elementwise"] = False, repr(e)
    out["h1pre_pad_rows_zero"] = bool((cur_h[B:] == 0).all())
    out["h1pre_next_slot_zero"] = bool((h1[slot ^ 1] == 0).all())
    np_ = fused_mlp.mlp_param_count(L1, L2)
    out["shadow_ok"] = bool(torch.equal(snap["shadow"][:np_].cpu(), snap["params"].cpu().to(torch.bfloat16)))
    out["params_finite"] = bool(torch.isfinite(snap["params"]).all())
    out["adam_state_finite"] = bool(torch.isfinite(snap["exp_avg"]).all() and torch.isfinite(snap["exp_avg_sq"]).all())
    return out


def _session_facts(eng):
    """Process-level facts at a failing step: buffer addresses, allocator state,
    threads and child processes alive (a long GPU session differs from a short one
    in exactly these)."""
    import threading

    facts = {"ptrs": {k: hex(getattr(eng, k).data_ptr()) for k in _STATE},
             "mem_alloc_mb": torch.cuda.memory_allocated() >> 20, "mem_reserved_mb": torch.cuda.memory_reserved() >> 20,
             "threads": sorted(t.name for t in threading.enumerate()),
             "stream": hex(torch.cuda.current_stream().cuda_stream)}
    try:
        import psutil

        facts["children"] = [(c.pid, " ".join(c.cmdline())[:120]) for c in psutil.Process().children(recursive=True)]
    except Exception as e:  # noqa: BLE001 - diagnostics only
        facts["children"] = repr(e)
    return facts


def _alloc_history(lo, hi, limit=12):
    """Allocator history (RLA_MEMHIST=1, tests/conftest.py) of device addresses [lo, hi):
    the segment holding them and the last alloc / free events of blocks overlapping
    them, each with its innermost Python frames -- the previous owners of a corrupted
    range."""
    try:
        return _alloc_history_impl(lo, hi, limit)
    except Exception as e:  # noqa: BLE001 - diagnostics only
        return {"error": repr(e)[:300]}


def _alloc_history_impl(lo, hi, limit):
    snap = torch.cuda.memory._snapshot()
    out = {"segments": [], "events": []}
    for seg in snap.get("segments", []):
        a, n = seg["address"], seg["total_size"]
        if a < hi and lo < a + n:
            out["segments"].append({"address": hex(a), "size": n, "pool": str(seg.get("segment_pool_id")),
                                    "stream": seg.get("stream"),
                                    "frames": [f"{f['filename'].split('/')[-1]}:{f['line']} {f['name']}"
                                               for f in (seg.get("frames") or [])[:6]]})
    ev = []
    for dev_trace in snap.get("device_traces", []):
        for i, t in enumerate(dev_trace):
            a, n = t.get("addr", 0), t.get("size", 0)
            if a < hi and lo < a + max(n, 1):
                ev.append((i, t))
    for i, t in ev[-limit:]:
        out["events"].append({"seq": i, "action": t.get("action"), "addr": hex(t.get("addr", 0)),
                              "size": t.get("size"), "stream": t.get("stream"),
                              "frames": [f"{f['filename'].split('/')[-1]}:{f['line']} {f['name']}"
                                         for f in (t.get("frames") or [])
                                         if "site-packages" not in f["filename"]][:8]})
    out["n_events"] = len(ev)
    return out


def _fidelity_log(name, rows):
    import json
    import os

    path = os.environ.get("RLA_FIDELITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": name, **rows}) + "\n")


def _diff_summary(a, b):
    """Elements that differ between two engines' buffers (count, first indices)."""
    out = {}
    for k in _STATE:
        ta, tb = getattr(a, k), getattr(b, k)
        ne = (ta != tb) if ta.dtype != torch.bfloat16 else (ta.view(torch.int16) != tb.view(torch.int16))
        n = int(ne.sum())
        if n:
            out[k] = {"n": n, "first": ne.nonzero().flatten()[:6].tolist()}
    return out


def _word_diff(a, b, k=12):
    """The raw 32-bit words where two same-shaped buffers differ: index and both values
    (hex and as fp32) -- a stray writer's values name it (a counter, a flag, a float)."""
    wa, wb = a.contiguous().view(torch.int32).flatten(), b.contiguous().view(torch.int32).flatten()
    ne = (wa != wb).nonzero().flatten()
    out = {"n": int(ne.numel())}
    idx = ne[:k]
    if idx.numel():
        va, vb = wa[idx].cpu(), wb[idx].cpu()
        out["words"] = [(int(i), f"{int(p) & 0xFFFFFFFF:08x}", f"{int(q) & 0xFFFFFFFF:08x}",
                         float(p.view(torch.float32)), float(q.view(torch.float32)))
                        for i, p, q in zip(idx.tolist(), va, vb)]
    return out


def _fidelity_run(eng, x, y, L1, L2, B, n_steps, world=1, autocast=False, make=None):
    """Step ``eng`` n_steps times; every step, the gradient it applied (recovered from
    Adam's first moment: m_t = b1 m_{t-1} + (1 - b1) g_t) against fp32 autograd on the
    same batch at the same parameters, per tensor, normwise.  Non-finite errors count
    as +inf (helpers.update_worst).  Between steps the test reads only what the error
    needs (params, exp_avg), as a production run would.

    The first step that breaks a bound is documented post mortem: ``make()`` builds a
    FRESH engine with the same init and data, stepped to the same point (one-launch,
    and two-launch), and every buffer is compared with the failing engine's --
    equal means the result is a deterministic function of the inputs (then the
    inputs, or the oracle, are what to look at); different names the buffers and
    first elements the failing run got wrong.  The failing engine's post-step state is
    checked against the engine's invariants for the NEXT step (_pre_step_check)."""
    b1 = eng.betas[0]
    worst = {k: 0.0 for k in _NAMES}
    worst_ac = {k: 0.0 for k in _NAMES}
    first_bad = None
    for step in range(n_steps):
        epoch, cur = eng.epoch, eng.step_in_epoch
        idx = shard_indices(x.size(0), world, 0, epoch, eng.seed, True)[cur * B:(cur + 1) * B]
        p0, m0 = eng.params.clone(), eng.exp_avg.clone()
        eng.step()
        g = (eng.exp_avg - b1 * m0) / (1 - b1)
        ref = _fp32_ref_grads(p0, x[idx], y[idx], L1, L2)
        errs = _per_tensor_rel(g, ref, L1, L2)
        update_worst(worst, errs)
        if step < 3:
            print(f"STEP {step} errs " + " ".join(f"{k}={v:.4g}" for k, v in errs.items()), flush=True)
        if autocast:
            update_worst(worst_ac, _per_tensor_rel(_autocast_grads(p0, x[idx], y[idx], L1, L2, _dev()), ref, L1, L2))
        if first_bad is None and not all(errs[k] < GRAD_BOUND[k] for k in _NAMES):
            torch.cuda.synchronize()
            # do the bulk device->host copies the oracle used return what the device holds?
            # (a checksum reduced ON the device, 8 bytes back, against the host copy's)
            dma = {}

            def csum(t):  # exact, order-independent integer checksum of the raw words
                return int(t.contiguous().view(torch.int32).long().sum())

            for name, t in (("p0", p0), ("m0", m0), ("g", g), ("params", eng.params), ("exp_avg", eng.exp_avg)):
                dev_sum, host_sum, host2 = csum(t), csum(t.cpu()), csum(t.cpu())
                # the device checksum again AFTER the copies: equal to the host's means the
                # device content changed in between (an asynchronous writer); equal to the
                # first means the copies returned data the device never held
                dev_again = csum(t)
                dma[name] = {"device": dev_sum, "host": host_sum, "host_again": host2, "device_again": dev_again,
                             "equal": dev_sum == host_sum, "ptr": hex(t.data_ptr()), "bytes": t.numel() * 4}
            # where p0 / g are not finite or are zero while the pre-step params are not: the
            # corrupted ranges, on the device and in a host copy, with the allocator history
            p0h = p0.cpu()
            for name, t in (("p0", p0), ("g", g)):
                bad_d = (~torch.isfinite(t)).nonzero().flatten()
                if name == "p0":
                    bad_d = torch.cat([bad_d, ((t == 0) & (eng.params != 0)).nonzero().flatten()]).unique()
                if bad_d.numel():
                    lo_i, hi_i = int(bad_d.min()), int(bad_d.max()) + 1
                    dma[name]["corrupt_words"] = [lo_i, hi_i, int(bad_d.numel())]
                    lo, hi = t.data_ptr() + 4 * lo_i, t.data_ptr() + 4 * hi_i
                    dma[name]["alloc_history"] = _alloc_history(lo, hi)
            dma["p0_host_nonfinite"] = int((~torch.isfinite(p0h)).sum())
            dma["p0_host_zero_where_params_nonzero"] = int(((p0h == 0) & (eng.params.cpu() != 0)).sum())
            xs, xh = int(eng.x_u8.long().sum()), int(x.long().sum())
            dma["x_u8_h2d"] = {"device": xs, "host": xh, "equal": xs == xh}
            first_bad = {"step": step, "epoch": epoch, "cur": cur, "errs": errs, "dma": dma,
                         "g_finite": bool(torch.isfinite(g).all()), "p0_finite": bool(torch.isfinite(p0).all()),
                         "g_nonfinite_idx": (~torch.isfinite(g)).nonzero().flatten()[:8].tolist(),
                         "hand": eng.hand[:20].tolist(), "counters_after": eng.counters[:11].tolist(),
                         "session": _session_facts(eng)}
            ne, nc = eng.epoch, eng.step_in_epoch
            nidx = shard_indices(x.size(0), world, 0, ne, eng.seed, True)[nc * B:(nc + 1) * B]
            first_bad["post_state_for_next_step"] = _pre_step_check(_snapshot(eng), x, y, nidx, L1, L2, B, nc, ne)
            if make is not None:
                for label, one in (("fresh_one_launch", True), ("fresh_two_launch", False)):
                    f = make()
                    if not one and f.dp_ctx is not None:
                        continue  # the loopback exchange exists only in the one-launch step
                    f.one_launch = f.one_launch and one
                    fb1 = f.betas[0]
                    for _ in range(step):
                        f.step()
                    fp0, fm0 = f.params.clone(), f.exp_avg.clone()
                    f.step()
                    torch.cuda.synchronize()
                    first_bad[label] = {
                        "errs": _per_tensor_rel((f.exp_avg - fb1 * fm0) / (1 - fb1),
                                                _fp32_ref_grads(fp0, x[idx], y[idx], L1, L2), L1, L2),
                        "pre_step_params_equal": bool(torch.equal(fp0, p0)),
                        "pre_step_params_words": _word_diff(p0, fp0),
                        "pre_step_exp_avg_words": _word_diff(m0, fm0),
                        "order_words": _word_diff(eng.order, f.order),
                        "x_u8_equal": bool(torch.equal(eng.x_u8, f.x_u8)),
                        "diff_vs_failing": _diff_summary(f, eng)}
    return worst, worst_ac, first_bad


@gpu
@pytest.mark.parametrize("L1,L2", [(32, 64), (128, 256)])
def test_mlp3_one_launch_grads_vs_fp32_autograd(L1, L2):
    """The production kernel (one-launch Step1) against fp32 PyTorch autograd, every
    step of 2+ epochs on the (non-trivial) synthetic task, held to the absolute bounds
    and to 1.5x stock bf16 autocast's own error on the same batches (+0.01)."""
    import json

    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    B, nb = 32, 24
    x, y = synthetic_mnist(B * nb + 7, seed=11)
    def make():
        e = FusedMLPEngine(L1, L2, B, lr=1e-3, device=_dev(), seed=1)
        e.set_data(x, y)
        return e

    eng = make()
    assert eng.one_launch
    worst, worst_ac, first_bad = _fidelity_run(eng, x, y, L1, L2, B, 2 * nb + 5, autocast=True, make=make)
    eng.check()
    _fidelity_log(f"one_launch_grads_{L1}_{L2}", {"steps": 2 * nb + 5, "max_rel_err": worst,
                                                  "stock_bf16_autocast_max_rel_err": worst_ac})
    if first_bad is not None:
        print("FIRST_BAD " + json.dumps(first_bad, default=str), flush=True)
    for k in _NAMES:
        assert worst[k] < GRAD_BOUND[k], (k, worst, first_bad)
        assert worst[k] < 1.5 * worst_ac[k] + 0.01, (k, worst, worst_ac)


@gpu
@pytest.mark.parametrize("proto", ["packed", "owner"])
def test_mlp3_dp_loopback_grads_vs_fp32_autograd(proto):
    """Step1DP (loopback world 4: every in-kernel path of the 4-rank exchange) against
    fp32 autograd, every step over 2+ epochs: the exchanged-and-averaged gradient
    (4 identical contributions) is the rank's own fp32 gradient up to bf16 compute and
    the protocol's wire rounding."""
    import json

    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    L1, L2, B, nb = 32, 64, 32, 20
    x, y = synthetic_mnist(B * nb + 3, seed=12)
    comms = []

    def make():
        cc, cx = _loopback_ctx(4)
        comms.append(cc)  # alive as long as its engine
        e = FusedMLPEngine(L1, L2, B, lr=1e-3, device=_dev(), seed=2, dp_context=cx, dp_proto=proto, dp_loop=True)
        e.set_data(x, y)
        return e

    eng = make()
    c = comms[0]
    assert eng.one_launch_dp
    worst, _, first_bad = _fidelity_run(eng, x, y, L1, L2, B, 2 * nb + 3, make=make)
    assert c.error_state() == 0
    eng.check()
    _fidelity_log(f"dp_loopback4_{proto}_grads", {"steps": 2 * nb + 3, "max_rel_err": worst})
    if first_bad is not None:
        print("FIRST_BAD " + json.dumps(first_bad, default=str), flush=True)
    for k in _NAMES:
        assert worst[k] < GRAD_BOUND[k], (k, worst, first_bad)


@gpu
def test_mlp3_300_step_trajectory_vs_fp32_torch_adam():
    """300 optimizer steps of the production step (hipGraph replays) against an fp32
    nn.Linear model + torch.optim.Adam fed the same batches from the same init: the
    parameter distance stays a small fraction of the distance travelled."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    L1, L2, B, n = 32, 64, 32, 300
    x, y = synthetic_mnist(B * 150, seed=13)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-3, device=_dev(), seed=3)
    eng.set_data(x, y)
    p_init = eng.params.clone()
    ref = {k: v.clone().requires_grad_(True) for k, v in
           zip(_NAMES, fused_mlp.mlp_unpack(p_init.cpu(), L1, L2).values())}
    opt = torch.optim.Adam(list(ref.values()), lr=1e-3)
    # the stock bf16 path (autocast, fp32 master weights + torch Adam) from the same init:
    # its own drift from fp32 calibrates what bf16 compute does to a trajectory
    dev = _dev()
    ac = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in ref.items()}
    opt_ac = torch.optim.Adam(list(ac.values()), lr=1e-3)
    nb = eng.n_batches
    losses_ref = []
    for s in range(n):
        epoch, cur = divmod(s, nb)
        idx = shard_indices(x.size(0), 1, 0, epoch, eng.seed, True)[cur * B:(cur + 1) * B]
        xb = x[idx].float() / 255.0
        h = torch.relu(F.linear(xb, ref["W1"], ref["b1"]))
        h = torch.relu(F.linear(h, ref["W2"], ref["b2"]))
        loss = F.nll_loss(torch.log_softmax(F.linear(h, ref["W3"], ref["b3"]), 1), y[idx])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses_ref.append(loss.item())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = torch.relu(F.linear(xb.to(dev), ac["W1"], ac["b1"]))
            h = torch.relu(F.linear(h, ac["W2"], ac["b2"]))
            z = F.linear(h, ac["W3"], ac["b3"])
        loss_ac = F.nll_loss(torch.log_softmax(z.float(), 1), y[idx].to(dev))
        opt_ac.zero_grad()
        loss_ac.backward()
        opt_ac.step()
    assert eng.capture(10)
    eng.run(n - 1)
    torch.cuda.synchronize()
    p_ref = torch.cat([ref[k].detach().reshape(-1) for k in _NAMES])
    p_k = eng.params.cpu()
    moved = (p_ref - p_init.cpu()).norm().item()
    drift = (p_k - p_ref).norm().item() / moved
    loss_k = eng.recent_stats(50)[:, 0].mean().item()
    loss_r = sum(losses_ref[-50:]) / 50
    per = {k: (a - b).norm().item() / max((b - c).norm().item(), 1e-12) for k, a, b, c in zip(
        _NAMES, fused_mlp.mlp_unpack(p_k, L1, L2).values(), fused_mlp.mlp_unpack(p_ref, L1, L2).values(),
        fused_mlp.mlp_unpack(p_init.cpu(), L1, L2).values())}
    p_ac = torch.cat([ac[k].detach().reshape(-1) for k in _NAMES]).cpu()
    drift_ac = (p_ac - p_ref).norm().item() / moved
    _fidelity_log("trajectory_300", {"drift_rel_to_travel": drift, "per_tensor": per,
                                     "stock_bf16_autocast_drift_rel_to_travel": drift_ac,
                                     "loss_kernel_last50": loss_k, "loss_fp32_last50": loss_r})
    # bf16 trajectories separate from fp32 chaotically (a flipped bf16 rounding
    # perturbs every later step): the kernel must stay within 1.5x of what the stock
    # bf16 path does from the same init and batches, and well inside the travel
    assert drift < 1.5 * drift_ac + 0.02 and drift < 0.3, (drift, drift_ac, per)
    assert abs(loss_k - loss_r) < 0.05 * loss_r + 0.02, (loss_k, loss_r)


@gpu
def test_dp_packed_wire_keeps_non_finite_and_max_finite():
    """the packed exchange's 2-bit tag rides in v0's low mantissa bits.
    Inf must stay Inf, NaN stay NaN (not become Inf), FLT_MAX stay finite (no carry
    into the exponent), every finite value within 2 ulp of fp32 (truncation near
    the top of a binade: 3 ulp) and the second value of a pair bit-exact."""
    from ray_lightning_accelerators_amd import ops

    C = ops.require()
    fmax = torch.finfo(torch.float32).max
    special = [float("inf"), -float("inf"), float("nan"), fmax, -fmax, 0.0, -0.0, 1e-45, 1.0,
               torch.nextafter(torch.tensor(2.0), torch.tensor(0.0)).item()]
    nan_low = torch.tensor([0x7F800001, 0x7F800003, 0xFF800002 - (1 << 32)], dtype=torch.int32).view(torch.float32)
    x = torch.cat([torch.tensor(special), nan_low, torch.randn(4096) * 1e3]).cuda()
    for tag in range(4):
        # every value in the encoded (even) position, then in the plain (odd) one
        even = torch.stack([x, torch.zeros_like(x)], 1).reshape(-1).contiguous()
        y = C.dp_pack_roundtrip(even, tag)[0::2]
        assert not torch.isnan(y[~torch.isnan(x)]).any(), "a tag mismatch or a finite value became NaN"
        assert torch.isnan(y[torch.isnan(x)]).all(), "a NaN lost its NaN-ness"
        inf = torch.isinf(x)
        assert torch.equal(y[inf], x[inf])
        fin = torch.isfinite(x)
        assert torch.isfinite(y[fin]).all(), "a finite value carried into the exponent"
        ulp = (torch.nextafter(x[fin].abs(), torch.tensor(float("inf"), device=x.device)) - x[fin].abs())
        assert ((y[fin] - x[fin]).abs() <= 3 * ulp).all()
        odd = torch.stack([torch.zeros_like(x), x], 1).reshape(-1).contiguous()
        y1 = C.dp_pack_roundtrip(odd, tag)[1::2]
        assert torch.equal(y1.view(torch.int32), x.view(torch.int32))
