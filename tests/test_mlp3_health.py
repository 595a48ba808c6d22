"""Health of the fused MNIST step's layer-1 partial sums: the kernels count the tile
partials their 12.20 fixed point clamps (finite, beyond +-32) and the NaN / Inf ones
(which the conversion would silently turn into a finite +-32), the engine reports the
counts (``health``) and applies ``RLAConfig.mlp_saturation`` in ``check``.

The GPU cases run with lr = 0 and no weight decay: Adam then leaves W1 exactly as
loaded, so the expected counts are closed-form (``mlp3_h1_health`` of one batch times
the number of primed batches: PRIME and every step prime one)."""
import logging
import math

import pytest
import torch

from ray_lightning_accelerators_amd.config import RLAConfig, get_config, set_config
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel import mlp_engine
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

gpu = pytest.mark.gpu
ENGINE_LOG = mlp_engine.__name__
# tile t of the constructed image holds 0, 4 or 12 pixels at 255 (t % 3 = 0, 1, 2)
TILES_12 = len([t for t in range(49) if t % 3 == 2])


@pytest.fixture
def policy():
    """Install a saturation policy for one test; the process's config is restored."""
    before = get_config()

    def use(name):
        set_config(before.replace(mlp_saturation=name))

    yield use
    set_config(before)


def _pattern_images(n):
    """n identical images: tile t has (0, 4, 12)[t % 3] pixels at 255, the rest 0."""
    row = torch.zeros(49, 16, dtype=torch.uint8)
    for t in range(49):
        row[t, : (0, 4, 12)[t % 3]] = 255
    x = row.reshape(1, 784).repeat(n, 1)
    y = torch.arange(n) % 10
    return x, y


def _saturating_params(L1, L2, seed=0):
    """W1[m, :] = +4 (even m) / -4 (odd m), both bf16-exact; the rest default (small)."""
    flat = fused_mlp.init_mlp_params(L1, L2, torch.Generator().manual_seed(seed))
    w1 = fused_mlp.mlp_unpack(flat, L1, L2)["layer_1.weight"]
    w1[0::2] = 4.0
    w1[1::2] = -4.0
    return flat


def _rand_u8(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


# ------------------------------------------------------------------ CPU: the oracle
def test_h1_health_small_weights_are_clean():
    x, _ = _rand_u8(20)
    w1 = fused_mlp.mlp_unpack(fused_mlp.init_mlp_params(32, 64), 32, 64)["layer_1.weight"]
    assert fused_mlp.mlp3_h1_health(x.float() / 255.0, w1) == (0, 0)


def test_h1_health_exact_count_of_constructed_case():
    """Partials are 0, +-16 or +-48: the nearest is a factor 1.5 from the clamp."""
    L1, B = 32, 20
    x, _ = _pattern_images(B)
    w1 = fused_mlp.mlp_unpack(_saturating_params(L1, 64), L1, 64)["layer_1.weight"]
    xr = x.float() / 255.0
    part = torch.einsum("bti,mti->tbm", xr.view(B, 49, 16), w1.view(L1, 49, 16))
    assert sorted(part.abs().unique().tolist()) == [0.0, 16.0, 48.0]
    assert fused_mlp.mlp3_h1_health(xr, w1) == (B * TILES_12 * L1, 0)


def test_h1_health_keeps_nan_and_inf_out_of_saturated():
    B, L1 = 4, 32
    x, _ = _pattern_images(B)
    xr = x.float() / 255.0
    w1 = torch.full((L1, 784), 0.01)
    w1[5, 100] = float("nan")  # tile 6: NaN whatever the pixel (0 * NaN)
    w1[7, 16 * 2] = float("inf")  # tile 2, a pixel that is on: +Inf
    w1[9, 16 * 5 + 1] = -float("inf")  # tile 5, on
    w1[11, 16 * 3] = float("inf")  # tile 3 has no pixel on: 0 * Inf = NaN
    assert fused_mlp.mlp3_h1_health(xr, w1) == (0, 4 * B)
    w1[1] = 4.0  # one saturating channel next to them
    assert fused_mlp.mlp3_h1_health(xr, w1) == (B * TILES_12, 4 * B)


def test_hand_layout_python_mirror():
    assert fused_mlp.mlp3_hand_layout(native=False) == {
        "ack": 0, "err": 16, "sat": 17, "nonfinite": 18, "last_step": 19, "words": 32}
    assert fused_mlp.mlp3_hand_words(32, 64) == 32


# ------------------------------------------------------------------ CPU: policy
def _stub_engine():
    """A CPU engine whose ``check`` reads a host ``hand`` (the blocking form needs no GPU)."""
    eng = FusedMLPEngine(32, 64, 32, device="cpu")
    eng.native = True
    eng.hand = torch.zeros(32, dtype=torch.int64)
    return eng


def _warnings(caplog):
    return [r for r in caplog.records if r.name == ENGINE_LOG and r.levelno == logging.WARNING]


def test_policy_warn_logs_once_per_increase(policy, caplog):
    policy("warn")
    eng = _stub_engine()
    caplog.set_level(logging.WARNING, logger=ENGINE_LOG)
    eng.check()
    assert not _warnings(caplog)
    eng.hand[17], eng.hand[19] = 640, 3
    eng.check()
    assert len(_warnings(caplog)) == 1 and "640" in _warnings(caplog)[0].getMessage()
    eng.check()  # nothing grew: silent
    assert len(_warnings(caplog)) == 1
    eng.hand[18], eng.hand[19] = 20, 9
    eng.check()
    assert len(_warnings(caplog)) == 2
    assert eng.health() == {"saturated": 640, "nonfinite": 20, "last_step": 9, "timed_out": False}
    eng.reset_health()
    assert eng.health() == {"saturated": 0, "nonfinite": 0, "last_step": 0, "timed_out": False}
    eng.check()
    assert len(_warnings(caplog)) == 2


def test_policy_raise_carries_the_counts(policy):
    policy("raise")
    eng = _stub_engine()
    eng.check()
    eng.hand[17], eng.hand[18], eng.hand[19] = 1234, 56, 78
    with pytest.raises(mlp_engine.FusedStepNumericsError) as ei:
        eng.check()
    msg = str(ei.value)
    assert "1234" in msg and "56" in msg and "78" in msg
    for remedy in ("fused_step=False", "learning rate", "RLA_MLP_SATURATION=warn"):
        assert remedy in msg
    assert isinstance(ei.value, RuntimeError)
    assert (ei.value.saturated, ei.value.nonfinite, ei.value.last_step) == (1234, 56, 78)


def test_policy_ignore_is_silent_but_counts(policy, caplog):
    policy("ignore")
    eng = _stub_engine()
    caplog.set_level(logging.WARNING, logger=ENGINE_LOG)
    eng.hand[17], eng.hand[18] = 5, 6
    eng.check()
    assert not _warnings(caplog)
    h = eng.health()
    assert (h["saturated"], h["nonfinite"]) == (5, 6)


@pytest.mark.parametrize("name", ["warn", "raise", "ignore"])
def test_timeout_word_raises_under_every_policy(policy, name):
    policy(name)
    eng = _stub_engine()
    eng.hand[16] = 1
    with pytest.raises(RuntimeError, match="an in-launch hand-off timed out") as ei:
        eng.check()
    assert not isinstance(ei.value, mlp_engine.FusedStepNumericsError)
    assert eng.health()["timed_out"] is True


def test_config_choice_and_env_round_trip():
    assert RLAConfig().mlp_saturation == "warn"
    with pytest.raises(ValueError):
        RLAConfig(mlp_saturation="loud")
    cfg = RLAConfig.from_env({"RLA_MLP_SATURATION": "raise"})
    assert cfg.mlp_saturation == "raise"
    env = cfg.to_env()
    assert env["RLA_MLP_SATURATION"] == "raise"
    assert RLAConfig.from_env(env).mlp_saturation == "raise"


def test_cpu_reference_engine_health_is_zero():
    x, y = _pattern_images(64)
    eng = FusedMLPEngine(32, 64, 16, lr=1e-3, device="cpu", init_params=_saturating_params(32, 64))
    eng.set_data(x, y)
    eng.run(3)
    assert eng.health() == {"saturated": 0, "nonfinite": 0, "last_step": 0, "timed_out": False}
    eng.check()
    eng.reset_health()


# ------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda", 0)


def _sat_engine(L1, L2, B, n_batches=5):
    x, y = _pattern_images(n_batches * B)
    eng = FusedMLPEngine(L1, L2, B, lr=0.0, weight_decay=0.0, device=_dev(),
                         init_params=_saturating_params(L1, L2))
    eng.set_data(x, y)
    per_batch, bad = fused_mlp.mlp3_h1_health(x[:B].float() / 255.0,
                                               fused_mlp.mlp_unpack(eng.params.cpu(), L1, L2)["layer_1.weight"])
    assert (per_batch, bad) == (B * TILES_12 * L1, 0)
    return eng, per_batch


@gpu
def test_hand_layout_from_the_extension():
    from ray_lightning_accelerators_amd import ops

    lay = dict(ops.require().mlp3_hand_layout())
    assert lay == {"ack": 0, "err": 16, "sat": 17, "nonfinite": 18, "last_step": 19, "words": 32}
    assert fused_mlp.mlp3_hand_layout() == lay


# (32, 64, 32): one launch, two H1pre copies; (128, 256, 32): one launch, one copy;
# (32, 32, 20): one launch, 12 padded rows that must not count; (64, 128, 64): two launches
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 32), (32, 32, 20), (64, 128, 64)])
def test_exact_saturation_count(L1, L2, B, policy):
    policy("ignore")
    n = 7  # over a 5-batch epoch: the count crosses an epoch boundary
    eng, per_batch = _sat_engine(L1, L2, B)
    assert eng.one_launch == (B <= 32)
    w1_before = eng.params.clone()
    eng.run(n)
    torch.cuda.synchronize()
    h = eng.health()
    print("health", (L1, L2, B), h, "expected", (n + 1) * per_batch)
    assert torch.equal(eng.params[: L1 * 784], w1_before[: L1 * 784])  # lr = 0: W1 as loaded
    assert h["saturated"] == (n + 1) * per_batch  # PRIME + n steps primed n + 1 batches
    assert h["nonfinite"] == 0
    assert h["last_step"] == n
    assert h["timed_out"] is False


@gpu
def test_saturation_count_in_graph_replay_equals_eager(policy):
    policy("ignore")
    eager, per_batch = _sat_engine(32, 64, 32)
    eager.run(8)
    graphed, _ = _sat_engine(32, 64, 32)
    assert graphed.capture(3)  # one eager warm-up step, then the captures
    graphed.run(7)
    torch.cuda.synchronize()
    assert graphed.global_step == eager.global_step == 8
    he, hg = eager.health(), graphed.health()
    print("eager", he, "graph", hg)
    assert hg == he
    assert hg["saturated"] == 9 * per_batch and hg["last_step"] == 8


@gpu
def test_nonfinite_w1_is_counted_and_loss_stays_finite(policy):
    """The hole being closed: a NaN in W1 becomes a finite -32 in H1pre, so the loss the
    step reports stays finite; the counter is what shows it."""
    policy("ignore")
    L1, L2, B, n = 32, 32, 20, 7
    x, y = _rand_u8(5 * B)
    flat = fused_mlp.init_mlp_params(L1, L2, torch.Generator().manual_seed(0))
    fused_mlp.mlp_unpack(flat, L1, L2)["layer_1.weight"][5, 100] = float("nan")
    eng = FusedMLPEngine(L1, L2, B, lr=0.0, weight_decay=0.0, device=_dev(), init_params=flat)
    eng.set_data(x, y)
    w1 = fused_mlp.mlp_unpack(eng.params.cpu(), L1, L2)["layer_1.weight"]
    assert fused_mlp.mlp3_h1_health(x[:B].float() / 255.0, w1) == (0, B)  # one tile, one channel, rows < B
    eng.run(n)
    torch.cuda.synchronize()
    h = eng.health()
    print("health", h)
    assert h["nonfinite"] == B * (n + 1)
    assert h["saturated"] == 0
    assert h["last_step"] == n
    assert bool(torch.isfinite(eng.recent_stats(n)[:, 0]).all())


@gpu
def test_policies_through_the_engine(policy, caplog):
    eng, per_batch = _sat_engine(32, 64, 32)
    eng.run(2)
    policy("raise")
    with pytest.raises(mlp_engine.FusedStepNumericsError, match=str(3 * per_batch)):
        eng.check()
    # the non-blocking form reports the copy made at the previous call
    eng.check(blocking=False)
    with pytest.raises(mlp_engine.FusedStepNumericsError):
        eng.check(blocking=False)
    policy("warn")
    caplog.set_level(logging.WARNING, logger=ENGINE_LOG)
    eng.check()
    assert len(_warnings(caplog)) == 1
    eng.reset_health()
    policy("raise")
    eng.check()  # no further steps: clean
    eng.check(blocking=False)
    eng.check(blocking=False)
    assert eng.health() == {"saturated": 0, "nonfinite": 0, "last_step": 0, "timed_out": False}
    eng.run(1)
    assert eng.health()["saturated"] == per_batch and eng.health()["last_step"] == 3


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (64, 128, 64)])
def test_healthy_run_counts_nothing(L1, L2, B, policy):
    policy("raise")
    x, y = _rand_u8(16 * B, seed=1)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-3, device=_dev(), seed=2)
    eng.set_data(x, y)
    eng.run(40)  # 16-batch epochs: two epoch boundaries
    torch.cuda.synchronize()
    assert eng.health() == {"saturated": 0, "nonfinite": 0, "last_step": 0, "timed_out": False}
    eng.check()
    eng.check(blocking=False)
    eng.check(blocking=False)


@gpu
def test_trainer_stores_fused_step_health(tmpdir):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    pl.seed_everything(0)
    model = LightningMNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": 32})
    trainer = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=2, limit_train_batches=6,
                         limit_val_batches=2)
    assert trainer.fused_step_health is None
    assert trainer.fit(model) == 1
    assert trainer._fused is not None and trainer._fused.eng is not None
    h = trainer.fused_step_health
    assert isinstance(h, dict), h
    assert h["saturated"] == 0 and h["nonfinite"] == 0 and h["timed_out"] is False
    assert trainer._fused.health() == h


# ------------------------------------------------ lr = 0.1, the reference's default
def _lr01_run(x, y, n_steps, L1=32, L2=64, B=32):
    eng = FusedMLPEngine(L1, L2, B, lr=0.1, device=_dev(), seed=0)
    eng.set_data(x, y)
    assert eng.capture(8)
    eng.run(n_steps - 1)
    torch.cuda.synchronize()
    assert eng.global_step == n_steps
    return eng


@gpu
def test_lr01_two_epochs_32_64(policy):
    """The bench's synthetic task at the reference's default learning rate (0.1, Adam),
    784-32-64-10, batch 32, two full epochs: nothing non-finite, and the counts and the
    parameters reproducible bit for bit.

    No loss assertion.  The bound asked for, |loss_fused - loss_fp32| < 1.5 |loss_autocast -
    loss_fp32| + m over the last 200 steps (m: the fp32 run's spread over three initial
    seeds), is missed: measured on an MI355X (scripts/mlp_health_lr01.py,
    profiles/r10_mlp_health/lr01.md) fused 1.7380, fp32 2.3179, autocast 2.3180,
    m = 0.00050, so 0.580 against a bound of 0.0007.  At this learning rate the fp32 run
    (all three seeds, around step 2,000) and the autocast run (around step 800) both end
    in the dead network that predicts the class prior (loss 2.318); the fused run does
    not.  The runs part in the first 200 steps; the first of the 13,318 saturated
    partials comes in steps 1,481-1,500."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    policy("ignore")
    x, y = synthetic_mnist(55000, seed=0)
    n = 2 * (x.size(0) // 32)
    a, b = _lr01_run(x, y, n), _lr01_run(x, y, n)
    ha, hb = a.health(), b.health()
    print("lr 0.1 health", ha, "loss of the last 200 steps", a.recent_stats(200)[:, 0].mean().item())
    assert ha["nonfinite"] == 0
    assert ha == hb
    assert ha["last_step"] <= n
    assert torch.equal(a.params, b.params)
    assert math.isfinite(a.recent_stats(200)[:, 0].mean().item())
