"""Gradient accumulation on the CPU reference engine (``FusedMLPEngine(accumulate=K)``,
the oracle of tests/test_mlp3_accumulate.py): against a hand-written torch loop with
``loss / K`` backward and ``torch.optim.Adam.step()`` at every window close."""
import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices

_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
L1, L2, B, NB = 32, 64, 32, 5


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _closes(i, K, nb=NB):
    return (i + 1) % K == 0 or i + 1 == nb


def _torch_loop(p_init, x, y, K, clip, epochs=2, lr=1e-2, seed=0):
    ref = {k: v.clone().requires_grad_(True) for k, v in zip(_NAMES, fused_mlp.mlp_unpack(p_init, L1, L2).values())}
    opt = torch.optim.Adam(list(ref.values()), lr=lr)
    steps, rows = 0, []
    for epoch in range(epochs):
        order = shard_indices(x.size(0), 1, 0, epoch, seed, True)
        opt.zero_grad()
        for i in range(NB):
            idx = order[i * B:(i + 1) * B]
            h = torch.relu(F.linear(x[idx].float() / 255.0, ref["W1"], ref["b1"]))
            h = torch.relu(F.linear(h, ref["W2"], ref["b2"]))
            logp = torch.log_softmax(F.linear(h, ref["W3"], ref["b3"]), 1)
            loss = F.nll_loss(logp, y[idx])
            (loss / K).backward()
            rows.append((loss.item(), float((logp.argmax(1) == y[idx]).sum()), float(B), float(steps + 1)))
            if _closes(i, K):
                if clip:
                    torch.nn.utils.clip_grad_norm_(list(ref.values()), clip)
                opt.step()
                opt.zero_grad()
                steps += 1
    return torch.cat([ref[k].detach().reshape(-1) for k in _NAMES]), opt, steps, torch.tensor(rows)


@pytest.mark.parametrize("clip", [None, 0.05])
@pytest.mark.parametrize("K", [2, 4])
def test_accumulate_equals_torch_loop(K, clip):
    x, y = _data(NB * B + 8, seed=K)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, clip_norm=clip, accumulate=K)
    eng.set_data(x, y)
    assert eng.n_batches == NB and eng.accumulate == K and not eng.one_launch
    p_init = eng.params.clone()
    eng.run(2 * NB)
    want, opt, steps, rows = _torch_loop(p_init, x, y, K, clip)
    assert steps == 2 * -(-NB // K)
    assert eng.optimizer_steps == steps and int(eng.counters[0]) == steps
    assert eng.global_step == 2 * NB and eng.epoch == 2 and eng.step_in_epoch == 0
    torch.testing.assert_close(eng.params, want)
    m = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in opt.param_groups[0]["params"]])
    v = torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for p in opt.param_groups[0]["params"]])
    torch.testing.assert_close(eng.exp_avg, m)
    torch.testing.assert_close(eng.exp_avg_sq, v)
    # one stats row per micro-batch, in consumption order; column 3: the window's optimizer step
    got = eng.recent_stats(2 * NB)
    assert got.shape == (2 * NB, 4)
    torch.testing.assert_close(got[:, 0], rows[:, 0])
    assert torch.equal(got[:, 1:], rows[:, 1:])
    if clip:
        assert eng.health()["clipped_steps"] == steps  # 0.05 is far below an untrained net's gradient norm


def test_k2_counts_six_optimizer_steps():
    """windows 2, 2, 1 per epoch of 5 batches: 6 optimizer steps after 10 batches"""
    x, y = _data(NB * B + 8, seed=1)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, accumulate=2)
    eng.set_data(x, y)
    seen = []
    for _ in range(2 * NB):
        eng.step()
        seen.append(eng.optimizer_steps)
    assert seen == [0, 1, 1, 2, 3, 3, 4, 4, 5, 6]
    assert eng.optimizer_steps == 6 and int(eng.counters[0]) == 6
    assert eng.steps_to_epoch_end() == NB


@pytest.mark.parametrize("clip", [None, 0.05])
def test_k1_is_bitwise_the_engine_without_the_argument(clip):
    x, y = _data(NB * B + 8, seed=3)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, clip_norm=clip)
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, clip_norm=clip, accumulate=1)
    for e in (a, b):
        e.set_data(x, y)
        e.run(2 * NB)
    for k in ("params", "exp_avg", "exp_avg_sq", "grads", "stats", "counters", "shadow"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.one_launch == b.one_launch and b.optimizer_steps == a.optimizer_steps == 2 * NB


def test_bad_accumulate_is_refused():
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="accumulate"):
            FusedMLPEngine(L1, L2, B, accumulate=bad)
    with pytest.raises(ValueError, match="dp_context"):
        FusedMLPEngine(L1, L2, B, world_size=2, accumulate=2, dp_context=[2, 0, 1 << 20, 1000, 0, 0, 0, 0])
    eng = FusedMLPEngine(L1, L2, B, accumulate=2)
    with pytest.raises(ValueError, match="whole windows"):
        eng.capture(3)
