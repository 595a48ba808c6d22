"""Per-step learning-rate schedules read from a device ring (GPU).

Every route of the fused MNIST step in ring mode (``FusedMLPEngine(lr_ring=8)`` driven by
``set_lr_schedule``) against the engine without a ring that is given ``set_lr(rate)`` before
every step: parameters, optimizer state, bf16 shadow, counters and stats rows ``torch.equal``.
The engine without a ring runs the instances that existed before the ring (the one-launch
kernel's are instruction-identical), so this holds the schedule instances to fp64-tested code.
Then: graph replays with schedules written behind them without a host sync, the zero-rate
step that pins the index rule, the refusal of the one-launch exchange, the loopback exchange
on the two-launch route, and ``Trainer.fit`` with ``OneCycleLR`` at step interval."""
import math

import pytest
import torch

import ray_lightning_accelerators_amd.lightning as pl
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

gpu = pytest.mark.gpu
RING = 8
DISPATCHES = (8, 5, 1) * 4  # 56 batches: 7 wraps of the ring (accumulate=2: 32 steps, 4 wraps)
_STATE = ("params", "exp_avg", "exp_avg_sq", "shadow", "stats", "counters")
MNIST_NORM = (0.1307, 0.3081)

# route -> (L1, L2, B, engine kwargs, set_data kwargs, RLA_MLP_ONE_LAUNCH, runs as one launch)
ROUTES = {
    "one_launch_row_chain_32_64": (32, 64, 32, {}, {}, None, True),
    "one_launch_parent_form_32_128": (32, 128, 32, {}, {}, None, True),
    "one_launch_normalize_32_64": (32, 64, 32, {}, {"normalize": MNIST_NORM}, None, True),
    "two_launches_b64": (32, 64, 64, {}, {}, None, False),
    "one_launch_off_b32": (32, 64, 32, {}, {}, "0", False),
    "clipped_three_launches": (32, 64, 32, {"clip_norm": 0.05}, {}, None, False),
    "sgd": (32, 64, 32, {"optimizer": "sgd", "momentum": 0.9, "weight_decay": 5e-4}, {}, None, False),
    "adamw_one_launch": (32, 64, 32, {"optimizer": "adamw", "weight_decay": 1e-2}, {}, None, True),
    "accumulate2": (32, 64, 32, {"accumulate": 2}, {}, None, False),
}


def _dev():
    return torch.device("cuda", 0)


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def rate(t: int) -> float:
    """The rate of optimizer step ``t`` (1-based): pairwise distinct."""
    return 1e-3 * (1.0 + 0.37 * math.sin(0.9 * t)) + 1e-6 * t


def _pair(L1, L2, B, kw, data_kw, nb=7):
    x, y = _data(nb * B + 5)
    out = []
    for ring in (RING, 0):
        eng = FusedMLPEngine(L1, L2, B, lr=1e-3, seed=3, device=_dev(), lr_ring=ring, **kw)
        eng.set_data(x, y, **data_kw)
        out.append(eng)
    return out


def _same_state(a, b, what=""):
    torch.cuda.synchronize()
    for k in _STATE:
        pa, pb = getattr(a, k), getattr(b, k)
        if pa is None and pb is None:
            continue
        assert torch.equal(pa, pb), (what, k, int((pa != pb).sum()))


def _scheduled(eng, n):
    eng.set_lr_schedule([rate(eng.optimizer_steps + 1 + i) for i in range(eng._opt_steps_in(n))])
    eng.run(n)


def _per_step(eng, n):
    for _ in range(n):
        eng.set_lr(rate(eng.optimizer_steps + 1))
        eng.step()


@gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_ring_route_equals_set_lr_per_step(route, monkeypatch):
    L1, L2, B, kw, data_kw, env, one = ROUTES[route]
    if env is not None:
        monkeypatch.setenv("RLA_MLP_ONE_LAUNCH", env)
    ring, ref = _pair(L1, L2, B, kw, data_kw)
    assert ring.one_launch == ref.one_launch == one
    assert ring.lr_mask == RING - 1 and ring.lr_tensor.numel() == RING and ref.lr_mask == 0
    p0 = ring.params.clone()
    for i, n in enumerate(DISPATCHES):
        _scheduled(ring, n)
        _per_step(ref, n)
        if i in (2, 7):
            _same_state(ring, ref, (route, i))
    assert ring.optimizer_steps == ref.optimizer_steps >= 3 * RING and ring.epoch >= 3
    _same_state(ring, ref, (route, "end"))
    assert not torch.equal(ring.params, p0)
    ring.check()


@gpu
def test_graph_replays_follow_schedules_written_behind_them():
    """``capture(4)``, then 50 dispatches of 3 or 7 steps, each behind a fresh 8-step schedule
    and with no host sync in between: the replayed graphs read each step's own rate.  A rate
    baked at capture, or a ring write that is not ordered with the launches (a staging buffer
    reused while an earlier copy is pending), separates the runs."""
    x, y = _data(40 * 32 + 5)
    ring = FusedMLPEngine(32, 64, 32, lr=1e-3, seed=3, device=_dev(), lr_ring=RING)
    ref = FusedMLPEngine(32, 64, 32, lr=1e-3, seed=3, device=_dev())
    for e in (ring, ref):
        e.set_data(x, y)
    ring.set_lr_schedule([rate(1)])
    assert ring.capture(4)  # one warm-up step, then the recording
    assert ring.optimizer_steps == 1 and ring._graph is not None and sorted(ring._tail_graphs) == [1, 2]
    for d in range(50):
        n = 4 * (d % 2) + 3
        t0 = ring.optimizer_steps
        ring.set_lr_schedule([rate(t0 + 1 + i) for i in range(RING)])
        ring.run(n)
    assert ring.optimizer_steps == 1 + 25 * 3 + 25 * 7
    _per_step(ref, ring.optimizer_steps)
    _same_state(ring, ref, "graph replay")
    assert ring._graph is not None
    ring.check()


def _zero_rate_snaps(eng, zero_at, n):
    t0 = eng.optimizer_steps
    eng.set_lr_schedule([0.0 if t0 + 1 + i == zero_at else 1e-3 for i in range(n)])
    snaps = [eng.params.clone()]
    for _ in range(n):
        eng.run(1)
        snaps.append(eng.params.clone())
    torch.cuda.synchronize()
    return snaps


@gpu
@pytest.mark.parametrize("B", [32, 64], ids=["one_launch", "two_launches"])
def test_zero_rate_step_sits_at_index_t_minus_1(B):
    """With weight_decay 0 a rate of 0.0 leaves the parameters bitwise alone at exactly that
    step; ``t & mask`` would move it by one, an ignored mask would lose it."""
    x, y = _data(7 * B + 5)
    eng = FusedMLPEngine(32, 64, B, lr=1e-3, seed=3, device=_dev(), lr_ring=RING, weight_decay=0.0)
    eng.set_data(x, y)
    assert eng.one_launch == (B == 32)
    snaps = _zero_rate_snaps(eng, zero_at=4, n=7)
    for t in range(1, 8):
        assert torch.equal(snaps[t - 1], snaps[t]) == (t == 4), t
    eng.set_step(20)  # the rates follow the new count: step 23 is entry (23 - 1) & 7
    snaps = _zero_rate_snaps(eng, zero_at=23, n=5)
    for i, t in enumerate(range(21, 26)):
        assert torch.equal(snaps[i], snaps[i + 1]) == (t == 23), t


@gpu
def test_one_launch_exchange_refuses_a_rate_ring_before_any_launch():
    from test_mlp3 import _loopback_ctx

    x, y = _data(7 * 32 + 5)
    c, ctx = _loopback_ctx(2)
    eng = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev(), dp_context=ctx, dp_proto="packed", dp_loop=True)
    eng.set_data(x, y)
    assert eng.one_launch_dp
    eng.prime()
    torch.cuda.synchronize()
    before = {k: getattr(eng, k).clone() for k in ("params", "exp_avg", "exp_avg_sq", "counters", "hand", "h1pre")}
    ring = torch.full((RING,), 1e-3, device=_dev())
    kw = {**eng._kw3(), "lr_tensor": ring, "lr_mask": RING - 1}
    with pytest.raises(ValueError, match="-16"):
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1_DP, stats=eng.stats, grad_scale=0.5, dp_ctx=eng.dp_ctx,
                              dp_proto=fused_mlp.DP_PROTOS["packed"], dp_loop=True, **kw)
    with pytest.raises(ValueError, match="lr_mask"):
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1, stats=eng.stats, **{**kw, "lr_mask": 5})
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k
    assert c.error_state() == 0, c.error_message()


@gpu
def test_loopback_exchange_takes_the_two_launch_route_in_ring_mode(caplog):
    """The in-process exchange (world 2, loopback) in ring mode: the one-launch exchange has no
    schedule instance, so the engine steps as head + tail with the exchange in the tail
    (``one_launch_dp`` false, one warning), and equals the same loopback engine given
    ``set_lr`` before every step.  (The same engine: the tail's loopback lives in its ring
    instances, and without a ring a loopback engine runs the one-launch exchange, whose packed
    wire form rounds to 4 ulp.  ``set_lr`` fills the whole ring, so a wrong index moves only
    the scheduled run.)"""
    import logging

    from test_mlp3 import _loopback_ctx

    x, y = _data(7 * 32 + 5)
    c, ctx = _loopback_ctx(2)
    kw = dict(lr=1e-3, seed=3, device=_dev(), dp_context=ctx, dp_proto="packed", dp_loop=True, lr_ring=RING)
    with caplog.at_level(logging.WARNING):
        ring = FusedMLPEngine(32, 64, 32, **kw)
    assert ring.one_launch and not ring.one_launch_dp and ring.dp_ctx[0] == 2
    assert len([r for r in caplog.records if "learning-rate ring" in r.getMessage()]) == 1
    ref = FusedMLPEngine(32, 64, 32, **kw)
    assert not ref.one_launch_dp
    for e in (ring, ref):
        e.set_data(x, y)
    p0 = ring.params.clone()
    for n in (8, 5, 1) * 3:
        _scheduled(ring, n)
        _per_step(ref, n)
    _same_state(ring, ref, "loopback")
    assert c.error_state() == 0, c.error_message()
    assert not torch.equal(ring.params, p0)


@gpu
def test_trainer_onecycle_step_interval_keeps_chunked_dispatch(tmpdir):
    """``Trainer.fit`` with Adam + ``OneCycleLR`` at step interval: 64-step chunks (a captured
    graph) train bit for bit what one dispatch per batch trains, and leave the scheduler where
    the per-batch loop leaves it."""
    from ray_lightning_accelerators_amd import ops
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    class OneCycle(LightningMNISTClassifier):
        def configure_optimizers(self):
            opt = torch.optim.Adam(self.parameters(), lr=1e-3)
            # (cycle_momentum would rewrite beta1 per step, which a captured graph bakes:
            # the Trainer dispatches such a scheduler per batch)
            sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-3, total_steps=260, cycle_momentum=False)
            return [opt], [{"scheduler": sch, "interval": "step"}]

    ops.require()
    res = {}
    for spd in (1, 64):
        pl.seed_everything(0)
        model = OneCycle({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": 32})
        tr = pl.Trainer(default_root_dir=str(tmpdir / f"s{spd}"), gpus=1, max_epochs=2, limit_train_batches=130,
                        limit_val_batches=2, checkpoint_callback=False, progress_bar_refresh_rate=0,
                        steps_per_dispatch=spd)
        assert tr.fit(model) == 1
        f = tr._fused
        assert f is not None and f.eng is not None and tr.global_step == 260
        assert f.lr_ring and f.eng.lr_mask == f.lr_ring - 1 and f.eng.lr_tensor is f.lr_tensor
        if spd > 1:
            assert f.eng._graph is not None and not f._capture_failed and f.eng._graph_steps == 64
        sch = tr.lr_schedulers[0]["scheduler"]
        res[spd] = ({k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                    float(tr.callback_metrics["ptl/train_loss"]), sch.last_epoch,
                    tr.optimizers[0].param_groups[0]["lr"], sch.state_dict())
    for k, v in res[1][0].items():
        assert torch.equal(v, res[64][0][k]), k
    assert res[1][1] == res[64][1]
    assert res[1][2] == res[64][2] == 260
    assert res[1][3] == res[64][3] and res[1][3] != 1e-3
    assert res[1][4] == res[64][4]
