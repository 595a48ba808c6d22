"""Per-step learning-rate schedules read from a device ring (CPU).

Engine: a ring-mode ``FusedMLPEngine`` driven by ``set_lr_schedule`` equals, bit for bit, the
engine without a ring that is given ``set_lr(rate)`` before every step -- Adam, AdamW, SGD with
momentum, ``accumulate=2`` and ``clip_norm``; the index rule ``(t - 1) & mask`` is held
independently of ``set_lr`` by a zero-rate step.  Trainer: with a fused step that declares
``schedules_lr`` a step-interval scheduler no longer forces one dispatch per batch; the rates
handed to the step, the scheduler's state and what ``LearningRateMonitor("step")`` logs are
those of the per-batch loop."""
import math

import pytest
import torch
from torch.utils.data import DataLoader

import ray_lightning_accelerators_amd.lightning as pl
from ray_lightning_accelerators_amd.lightning import Callback, LightningModule
from ray_lightning_accelerators_amd.lightning.callbacks import LearningRateMonitor
from ray_lightning_accelerators_amd.models.data import RandomDataset
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

RING = 8
B = 32
N_DATA = 7 * B + 5  # 7 batches an epoch: every run below wraps the epoch several times
DISPATCHES = (8, 5, 1, 8, 5, 1, 8, 5, 1)  # 42 batches: >= 5 wraps of a ring of 8 (accumulate=2: ~3)
CONFIGS = {
    "adam": dict(weight_decay=1e-3),
    "adamw": dict(optimizer="adamw", weight_decay=1e-2),
    "sgd_momentum": dict(optimizer="sgd", momentum=0.9, weight_decay=5e-4),
    "accumulate2": dict(accumulate=2),
    "clip": dict(clip_norm=0.05),
}


def _data(n=N_DATA, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _engine(ring, **kw):
    x, y = _data()
    eng = FusedMLPEngine(32, 64, B, lr=1e-3, seed=3, lr_ring=ring, **kw)
    eng.set_data(x, y, shuffle=True)
    return eng


def rate(t: int) -> float:
    """The rate of optimizer step ``t`` (1-based): pairwise distinct, none a neighbour's."""
    return 1e-3 * (1.0 + 0.37 * math.sin(0.9 * t)) + 1e-6 * t


def _state(eng):
    out = [eng.params.clone(), eng.exp_avg.clone(), eng.counters[:5].clone()]
    if eng.exp_avg_sq is not None:
        out.append(eng.exp_avg_sq.clone())
    return out


def _assert_same(a, b, what):
    for i, (u, v) in enumerate(zip(_state(a), _state(b))):
        assert torch.equal(u, v), (what, i)


def drive_scheduled(eng, n_batches: int):
    """``n_batches`` batches with a schedule for exactly the optimizer steps among them."""
    n_opt = eng._opt_steps_in(n_batches)
    eng.set_lr_schedule([rate(eng.optimizer_steps + 1 + i) for i in range(n_opt)])
    eng.run(n_batches)


def drive_per_step(eng, n_batches: int):
    for _ in range(n_batches):
        eng.set_lr(rate(eng.optimizer_steps + 1))
        eng.step()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_scheduled_ring_equals_set_lr_per_step(name):
    ring, ref = _engine(RING, **CONFIGS[name]), _engine(0, **CONFIGS[name])
    assert ring.lr_tensor.numel() == RING and ref.lr_tensor.numel() == 1
    assert len({rate(t) for t in range(1, 60)}) == 59
    for i, n in enumerate(DISPATCHES):
        drive_scheduled(ring, n)
        drive_per_step(ref, n)
        assert ring.optimizer_steps == ref.optimizer_steps and ring.global_step == ref.global_step
        if i in (2, 5):  # two intermediate points
            _assert_same(ring, ref, (name, i))
    assert ring.optimizer_steps >= 3 * RING and ring.epoch >= 3
    _assert_same(ring, ref, (name, "end"))
    assert not torch.equal(ring.params, _engine(0, **CONFIGS[name]).params)


def test_steps_past_the_schedule_run_at_the_engine_rate():
    """``set_lr`` / ``step`` / ``run`` keep working in ring mode: entries of unscheduled steps
    are rewritten with ``lr`` before they are dispatched, stale scheduled rates included."""
    ring, ref = _engine(RING), _engine(0)
    ring.set_lr_schedule([rate(t) for t in range(1, 4)])
    ring.run(11)  # 3 scheduled, 8 at lr: the whole ring is walked once past the schedule
    drive_per_step(ref, 3)
    ref.set_lr(1e-3)
    ref.run(8)
    _assert_same(ring, ref, "past the schedule")
    for e in (ring, ref):
        e.set_lr(2e-3)
        e.run(9)
    _assert_same(ring, ref, "set_lr in ring mode")
    ring.set_lr_schedule([rate(t) for t in range(1, 6)])
    ring.set_lr(5e-4)  # forgets the schedule
    ref.set_lr(5e-4)
    ring.run(6)
    ref.run(6)
    _assert_same(ring, ref, "set_lr forgets a schedule")


def _zero_rate_run(eng, zero_at: int, n: int):
    """Parameters after each of ``n`` steps under a schedule whose step ``zero_at`` has rate 0."""
    t0 = eng.optimizer_steps
    eng.set_lr_schedule([0.0 if t0 + 1 + i == zero_at else 1e-3 for i in range(n)])
    snaps = [eng.params.clone()]
    for _ in range(n):
        eng.run(1)
        snaps.append(eng.params.clone())
    return snaps


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_zero_rate_step_sits_at_index_t_minus_1(optimizer):
    """Independent of the ``set_lr`` route: with weight_decay 0 a rate of 0.0 leaves the
    parameters bitwise alone at exactly that step -- ``t & mask`` would move it by one."""
    eng = _engine(RING, optimizer=optimizer, weight_decay=0.0)
    snaps = _zero_rate_run(eng, zero_at=4, n=7)
    for t in range(1, 8):
        assert torch.equal(snaps[t - 1], snaps[t]) == (t == 4), t
    # after set_step the rates follow the new count: step 21 is entry (21 - 1) & 7 = 4
    eng.set_step(20)
    assert eng.optimizer_steps == 20
    snaps = _zero_rate_run(eng, zero_at=23, n=5)
    for i, t in enumerate(range(21, 26)):
        assert torch.equal(snaps[i], snaps[i + 1]) == (t == 23), t


def test_argument_checks():
    for bad in (1, 3, 6, 12, -2, True):
        with pytest.raises(ValueError, match="lr_ring"):
            FusedMLPEngine(32, 64, B, lr_ring=bad)
    eng = _engine(RING)
    eng.set_lr_schedule([1e-3] * RING)
    with pytest.raises(ValueError, match="do not fit"):
        eng.set_lr_schedule([1e-3] * (RING + 1))
    with pytest.raises(RuntimeError, match="ring mode"):
        _engine(0).set_lr_schedule([1e-3])
    with pytest.raises(ValueError, match="learning-rate ring"):
        eng.capture(2 * RING)


# ----------------------------------------------------------------------------- Trainer
class _RecordingFused:
    """A fused step that records what the Trainer hands it (no device work)."""
    max_chunk = 64
    schedules_lr = True

    def __init__(self, trainer):
        self.trainer = trainer
        self.chunks = []      # steps per train_chunk
        self.rates = []       # the rate each step ran with
        self.per_batch = 0
        self._B = 4
        self._pending = None

    def make_epoch_batches(self, dl, n):
        return [("__rla_resident__", i) for i in range(n)]

    def set_lr_schedule(self, rates):
        self._pending = list(rates)

    def train_batch(self, batch, batch_idx):
        self.per_batch += 1
        self.rates.append(self.trainer.optimizers[0].param_groups[0]["lr"])
        return {"loss": torch.tensor(1.0)}

    def train_chunk(self, k):
        assert self._pending is not None and len(self._pending) == k, (self._pending, k)
        self.rates.extend(self._pending)
        self._pending = None
        self.chunks.append(k)
        return [{"loss": torch.tensor(1.0)} for _ in range(k)]

    def on_lr_change(self):
        pass

    def sync_params_to_module(self):
        pass

    def load_params_from_module(self):
        pass


class _Model(LightningModule):
    fused_cls = _RecordingFused

    def __init__(self, kind="steplr"):
        super().__init__()
        self.layer = torch.nn.Linear(32, 2)
        self.kind = kind

    def forward(self, x):
        return self.layer(x)

    def training_step(self, batch, batch_idx):
        return self(batch).sum()

    def configure_optimizers(self):
        opt = torch.optim.SGD(self.layer.parameters(), lr=0.1, momentum=0.9)
        if self.kind == "steplr":
            return [opt], [{"scheduler": torch.optim.lr_scheduler.StepLR(opt, 10), "interval": "step"}]
        if self.kind == "lambda3":
            sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1.0 + e))
            return [opt], [{"scheduler": sch, "interval": "step", "frequency": 3}]
        if self.kind == "onecycle_momentum":  # cycle_momentum defaults to True: it moves the momentum too
            sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.5, total_steps=90)
            return [opt], [{"scheduler": sch, "interval": "step"}]
        if self.kind == "plateau":
            sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt)
            return [opt], [{"scheduler": sch, "interval": "step", "reduce_on_plateau": True, "monitor": "loss"}]
        return opt

    def train_dataloader(self):
        return DataLoader(RandomDataset(32, 4 * 45), batch_size=4)

    def configure_fused_step(self, trainer):
        self.fake = self.fused_cls(trainer)
        return self.fake


class _BatchRates(Callback):
    """The per-batch loop's own record: the group's rate when each batch starts."""

    def __init__(self):
        self.rates = []

    def on_train_batch_start(self, trainer, pl_module, batch, batch_idx, dataloader_idx):
        self.rates.append(trainer.optimizers[0].param_groups[0]["lr"])


def _fit(tmpdir, kind, spd, callbacks=(), **kw):
    model = _Model(kind)
    tr = pl.Trainer(default_root_dir=str(tmpdir / f"{kind}_{spd}_{len(callbacks)}"), max_epochs=2,
                    num_sanity_val_steps=0, progress_bar_refresh_rate=0, steps_per_dispatch=spd,
                    callbacks=list(callbacks), log_every_n_steps=7, **kw)
    assert tr.fit(model) == 1
    return tr, model


@pytest.mark.parametrize("kind", ["steplr", "lambda3"])
def test_trainer_chunks_carry_the_per_batch_rates(tmpdir, kind):
    hook = _BatchRates()
    tr1, m1 = _fit(tmpdir, kind, 1, callbacks=[hook], checkpoint_callback=False)
    assert m1.fake.chunks == [] and m1.fake.per_batch == 90 and len(hook.rates) == 90
    assert len(set(hook.rates)) > 3  # the scheduler did move the rate
    tr64, m64 = _fit(tmpdir, kind, 16, checkpoint_callback=False)
    assert m64.fake.per_batch == 0 and max(m64.fake.chunks) > 1 and sum(m64.fake.chunks) == 90
    assert m64.fake.rates == hook.rates == m1.fake.rates
    s1, s64 = tr1.lr_schedulers[0]["scheduler"], tr64.lr_schedulers[0]["scheduler"]
    assert s1.last_epoch == s64.last_epoch == (90 if kind == "steplr" else 30)
    assert tr1.optimizers[0].param_groups[0]["lr"] == tr64.optimizers[0].param_groups[0]["lr"]
    d1, d64 = s1.state_dict(), s64.state_dict()
    d1.pop("lr_lambdas", None), d64.pop("lr_lambdas", None)
    assert d1 == d64


def test_trainer_checkpoint_holds_the_per_batch_scheduler_state(tmpdir):
    cks = []
    for spd in (1, 16):
        tr, _ = _fit(tmpdir, "steplr", spd)
        cks.append(tr.checkpoint_connector.dump_checkpoint())
    assert cks[0]["lr_schedulers"] == cks[1]["lr_schedulers"] and cks[0]["lr_schedulers"][0]["last_epoch"] == 90
    assert cks[0]["global_step"] == cks[1]["global_step"] == 91  # the checkpoint counts from 1


def test_plateau_scheduler_and_steps_without_schedules_lr_stay_per_batch(tmpdir):
    for kind in ("plateau", "onecycle_momentum"):  # (the second rewrites the momentum per step)
        _, m = _fit(tmpdir, kind, 16, checkpoint_callback=False)
        assert m.fake.chunks == [] and m.fake.per_batch == 90, kind

    class NoSched(_RecordingFused):
        schedules_lr = False

    class M(_Model):
        fused_cls = NoSched

    model = M("steplr")
    tr = pl.Trainer(default_root_dir=str(tmpdir / "nosched"), max_epochs=1, num_sanity_val_steps=0,
                    checkpoint_callback=False, progress_bar_refresh_rate=0, steps_per_dispatch=16)
    assert tr.fit(model) == 1
    assert model.fake.chunks == [] and model.fake.per_batch == 45


def test_learning_rate_monitor_step_logs_the_rate_each_log_point_ran_with(tmpdir):
    logs = []
    for spd in (1, 16):
        mon = LearningRateMonitor(logging_interval="step")
        tr, m = _fit(tmpdir, "steplr", spd, callbacks=[mon], checkpoint_callback=False)
        assert (m.fake.per_batch == 0) == (spd == 16)
        logs.append(list(mon.history))
        # log_every_n_steps=7: the rate step 7, 14, ... ran with
        assert [s for s, _ in mon.history] == list(range(7, 91, 7))
        assert all(lr == m.fake.rates[s - 1] for s, lr in mon.history)
    assert logs[0] == logs[1]
    # the default stays what it was: one value per epoch start, no step entries
    mon = LearningRateMonitor()
    _fit(tmpdir, "steplr", 16, callbacks=[mon], checkpoint_callback=False)
    assert mon.history == []
