"""The short last batch of a ``drop_last=False`` loader on the fused MNIST step's HIP path
(GPU): ``last_rows`` of the two-launch kernels and PRIME (csrc/mlp_step3.hip), the engine's
routing around it (``FusedMLPEngine.begin_epoch(..., last_rows=r)``), graphs, accumulation,
health counts, the refusals, and ``MNISTClassifier`` under the Trainer.
CPU semantics: tests/test_mlp3_short_batch_reference.py.

The key oracle is the kernels themselves: a short batch of ``r`` rows in an engine of batch
``B`` is the computation an engine of batch ``r`` performs -- the same zero padding, the same
fixed reduction orders -- so the two must agree under ``==`` (``-0 == +0`` where the larger
engine sums extra all-zero head blocks / batch columns)."""
import logging

import pytest
import torch
from torch.utils.data import DataLoader, Subset

from ray_lightning_accelerators_amd.ops import fused_mlp, require
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

gpu = pytest.mark.gpu
NORM = (0.1307, 0.3081)
_STATE = ("params", "exp_avg", "exp_avg_sq", "shadow", "stats", "h1pre", "xring", "yring", "grads")


def _dev():
    return torch.device("cuda", 0)


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _order(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _engine(L1, L2, B, x, y, one_launch=None, normalize=None, **kw):
    kw.setdefault("lr", 1e-2)
    eng = FusedMLPEngine(L1, L2, B, device=_dev(), stats_ring=64, **kw)
    if one_launch is not None:
        eng.one_launch = one_launch and eng.one_launch
    eng.attach_dataset(x, y, normalize=normalize)
    return eng


ROUTES = {
    "default": dict(),
    "two_launch": dict(one_launch=False),
    "clip": dict(clip_norm=0.05),
    "sgd": dict(optimizer="sgd", momentum=0.9),
}
CASES = [(32, 64, 32, 1), (32, 64, 32, 17), (128, 256, 32, 31), (64, 128, 64, 33), (64, 128, 64, 7), (32, 32, 24, 5)]
_PAIRS = [(c, r, None) for c in CASES for r in ROUTES] + [((32, 64, 32, 17), "default", NORM)]


# ------------------------------------------------------------------ 3: short step == step of a B = r engine
@gpu
@pytest.mark.parametrize("case,route,norm", _PAIRS,
                         ids=["%d-%d-B%d-r%d-%s%s" % (*c, r, "-norm" if n else "") for c, r, n in _PAIRS])
def test_short_step_equals_the_step_of_an_engine_of_that_batch(case, route, norm):
    L1, L2, B, r = case
    kw = ROUTES[route]
    x, y = _data(2 * B + r + 5, seed=L1 + B + r)
    order = _order(x.size(0), 1)[: 2 * B + r]
    a = _engine(L1, L2, B, x, y, normalize=norm, **kw)
    a.begin_epoch(order, 3, last_rows=r)
    a.run(2)
    torch.cuda.synchronize()
    step = int(a.counters[0])
    assert step == 2 and a.last_rows == r
    c = _engine(L1, L2, r, x, y, normalize=norm, init_params=a.params, **kw)
    c.exp_avg.copy_(a.exp_avg)
    if a.exp_avg_sq is not None:
        c.exp_avg_sq.copy_(a.exp_avg_sq)
    c.set_step(step)
    c.begin_epoch(order[2 * B:], 1)
    a.run(1)
    c.run(1)
    torch.cuda.synchronize()
    a.check()
    c.check()
    assert int(a.counters[0]) == int(c.counters[0]) == 3
    for k in ("params", "exp_avg", "exp_avg_sq"):
        pa, pc = getattr(a, k), getattr(c, k)
        if pa is None:
            assert pc is None
            continue
        assert bool((pa == pc).all()), (k, int((pa != pc).sum()), (pa - pc).abs().max().item())
        if (r + 31) // 32 == (B + 31) // 32:   # the same head blocks and batch columns: the same bits
            assert torch.equal(pa.view(torch.int32), pc.view(torch.int32)), k
    ra, rc = a.stats[step % 64].cpu(), c.stats[step % 64].cpu()
    assert bool((ra == rc).all()) and ra[2] == r and ra[3] == 3, (ra, rc)
    if route == "clip":
        assert torch.equal(a.clip_out[:2], c.clip_out[:2])
    # the order's padding slots hold a valid index and the staged batch is masked past r
    assert a.order.size(1) == 3 * B and int(a.order.max()) < x.size(0)
    h = a.health()
    assert h["saturated"] == 0 and h["nonfinite"] == 0


# ------------------------------------------------------------------ 4 + 9: across the epoch boundary, health
def _same_state(a, b, keys=_STATE):
    torch.cuda.synchronize()
    assert torch.equal(a.counters[:10].cpu(), b.counters[:10].cpu()), (a.counters, b.counters)
    for k in keys:
        pa, pb = getattr(a, k), getattr(b, k)
        bits = (lambda u: u.view(torch.int16)) if pa.dtype == torch.bfloat16 else (lambda u: u)
        assert torch.equal(bits(pa), bits(pb)), (k, int((pa != pb).sum()))


@gpu
@pytest.mark.parametrize("L1,L2,B,r,norm", [(32, 64, 32, 17, None), (128, 256, 20, 3, NORM)])
def test_short_batch_one_launch_route_equals_two_launch_across_epochs(L1, L2, B, r, norm):
    """2 epochs + 1 step of [B, B, r]: one launch around the two head + tail steps against head +
    tail throughout, every state tensor bit for bit (the re-prime after the short batch, a
    second short batch); then the health words."""
    x, y = _data(2 * B + r, seed=7)
    a = _engine(L1, L2, B, x, y, normalize=norm)
    b = _engine(L1, L2, B, x, y, one_launch=False, normalize=norm)
    assert a.one_launch and not b.one_launch
    seq = []
    for ep, n in ((0, 3), (1, 3), (2, 1)):
        order = _order(x.size(0), 10 + ep)
        for e in (a, b):
            e.begin_epoch(order, 3, last_rows=r)
        for _ in range(n):
            seq.append(a._short_pos(a.step_in_epoch))
            a.step()
            b.step()
    assert seq == [False, True, True] * 2 + [False]
    keys = tuple(k for k in _STATE if k != "grads")   # the one-launch step keeps its gradient in registers
    _same_state(a, b, keys)
    assert int(a.counters[10]) == 3 and int(b.counters[10]) == 0   # one-launch steps: positions 0 only
    assert a.recent_stats(7)[:, 2].tolist() == [B, B, r, B, B, r, B]
    for e in (a, b):
        e.check()
        h = e.health()
        assert h["saturated"] == 0 and h["nonfinite"] == 0 and not h["timed_out"], h


@gpu
def test_prime_gathers_a_short_only_batch_masked():
    """A one-batch epoch: PRIME gathers the short batch itself -- r labels, -1 and true zero
    pixels past them -- and the masked rows raise no health count."""
    L1, L2, B, r = 32, 64, 32, 5
    x, y = _data(64, seed=2)
    x[:] = 255   # every real pixel is non-zero: a masked row is told from a real one
    eng = _engine(L1, L2, B, x, y)
    eng.begin_epoch(_order(64, 3)[:r], 1, last_rows=r)
    eng.prime()
    torch.cuda.synchronize()
    h = eng.health()
    assert h["saturated"] == 0 and h["nonfinite"] == 0
    bp = 32
    yr = eng.yring.view(2, bp)[int(eng.counters[3])]
    assert bool((yr[r:] == -1).all()) and bool((yr[:r] >= 0).all())
    xr = eng.xring.view(2, 49, bp, 16)[int(eng.counters[3])]
    assert bool((xr[:, r:].view(torch.int16) == 0).all())   # true zeros past the short batch
    assert bool((xr[:, :r].float() == 1.0).all())


# ------------------------------------------------------------------ 5: graph replay == eager
@gpu
@pytest.mark.parametrize("K,gsteps", [(1, 3), (2, 2)], ids=["plain", "accumulate2"])
def test_short_batch_graph_replay_matches_eager(K, gsteps):
    nb, B, r = 5, 32, 9
    x, y = _data(4 * B + r + 1, seed=5)
    longer = _order(x.size(0), 6)
    order = longer[: 4 * B + r]
    a = _engine(32, 64, B, x, y, lr=1e-3, accumulate=K)
    b = _engine(32, 64, B, x, y, lr=1e-3, accumulate=K)
    for e in (a, b):
        e.begin_epoch(order, nb, last_rows=r)
    assert b.capture(gsteps)
    a.run(K)   # capture() ran K real batches
    a.run(24 - K)
    replays = 0
    for n in (6, 1, 9, 7 if K == 1 else 8 - K):
        done = 0
        while done < n:   # run(), counting the replays
            g, k = b._pick_graph(n - done)
            if g is not None:
                assert b.step_in_epoch + k <= nb - (2 if K == 1 else 1)   # never across the short batch
                g.replay()
                replays += 1
            else:
                b._device_step()
            b._advance_host(k)
            done += k
    torch.cuda.synchronize()
    assert replays > 0 and a.global_step == b.global_step == 24
    assert a.optimizer_steps == b.optimizer_steps == int(a.counters[0])
    assert torch.equal(a.counters.cpu(), b.counters.cpu())
    _same_state(a, b, ("params", "exp_avg", "exp_avg_sq", "stats", "h1pre"))
    assert a.recent_stats(24)[:, 2].tolist() == ([B] * 4 + [r]) * 4 + [B] * 4
    b.begin_epoch(order, nb, last_rows=r)
    assert b._graph is not None    # the same shape keeps the graphs ...
    b.begin_epoch(longer, nb, last_rows=r + 1)
    assert b._graph is None        # ... another last_rows drops them


# ------------------------------------------------------------------ 6: accumulation
@gpu
@pytest.mark.parametrize("L1,L2,B,r", [(32, 64, 32, 17), (64, 128, 64, 7)])
def test_short_window_accumulates_the_exact_fp32_sum(L1, L2, B, r):
    """K = 2 over [B, B, r], lr = 0 (the method of test_accumulated_grads_are_the_exact_fp32_sum):
    a split-route twin's ``grads`` are the single gradients; the short batch is the epoch's
    short last window and overwrites."""
    K = 2
    x, y = _data(2 * B + r, seed=L1 + r)
    a = _engine(L1, L2, B, x, y, lr=0.0, accumulate=K)
    b = _engine(L1, L2, B, x, y, lr=0.0, world_size=2, allreduce=lambda g: None)
    run = None
    for ep in range(2):
        order = _order(x.size(0), 20 + ep)
        for e in (a, b):
            e.begin_epoch(order, 3, last_rows=r)
        for pos in range(3):
            a.step()
            b.step()
            run = b.grads.clone() if pos % K == 0 else run + b.grads
            torch.cuda.synchronize()
            assert torch.equal(a.grads, run), (ep, pos, int((a.grads != run).sum()))
    assert a.optimizer_steps == 4 == int(a.counters[0])
    assert a.recent_stats(6)[:, 2].tolist() == [B, B, r] * 2
    assert a.recent_stats(6)[:, 3].tolist() == [1, 1, 2, 3, 3, 4]


# ------------------------------------------------------------------ 7: against fp32 autograd
@gpu
@pytest.mark.parametrize("L1,L2", [(32, 64), (128, 256)])
def test_short_step_grads_vs_fp32_autograd(L1, L2):
    """The short step's gradient (B = 32, r = 17) against fp32 autograd on its 17 rows, under
    the per-tensor bounds tests/test_mlp3.py::test_mlp3_one_launch_grads_vs_fp32_autograd
    applies to a full batch: GRAD_BOUND, and 1.5x stock bf16 autocast's own error + 0.01."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist
    from test_mlp3 import GRAD_BOUND, _NAMES, _autocast_grads, _fp32_ref_grads, _per_tensor_rel

    B, r = 32, 17
    x, y = synthetic_mnist(2 * B + r, seed=11)
    order = _order(x.size(0), 4)
    eng = _engine(L1, L2, B, x, y, lr=1e-3, world_size=2, allreduce=lambda g: None)   # grads stay readable
    eng.begin_epoch(order, 3, last_rows=r)
    eng.run(2)
    torch.cuda.synchronize()
    p = eng.params.cpu().clone()
    eng.run(1)
    torch.cuda.synchronize()
    idx = order[2 * B:]
    got = _per_tensor_rel(eng.grads, _fp32_ref_grads(p, x[idx], y[idx], L1, L2), L1, L2)
    ac = _per_tensor_rel(_autocast_grads(p, x[idx], y[idx], L1, L2, _dev()), _fp32_ref_grads(p, x[idx], y[idx], L1, L2),
                         L1, L2)
    print(f"short step {L1}/{L2}: rel err {got}, autocast {ac}")
    for k in _NAMES:
        assert got[k] < GRAD_BOUND[k], (k, got)
        assert got[k] < 1.5 * ac[k] + 0.01, (k, got, ac)


# ------------------------------------------------------------------ 8: refusals
def _raw_mlp3(kind, kw, stats, dp_ctx=(), dp_proto=-1, **extra):
    """``_C.mlp3`` without ops.fused_mlp.mlp3_launch's own argument checks."""
    b = kw["betas"]
    args = [int(kind), kw["x_u8"], kw["labels"], kw["order"], kw["counters"], kw["n_batches"], kw["B"], kw["L1"],
            kw["L2"], kw["params"], kw["grads"], kw["exp_avg"], kw["exp_avg_sq"], kw["shadow"], kw["dh1t"],
            kw["xring"], kw["h1pre"], kw["act"], kw["yring"], stats, True, kw["lr"], b[0], b[1], kw["eps"],
            kw["weight_decay"], 1.0, kw["lr_tensor"], False, None, list(dp_ctx), kw["head_part"], kw["hand"], dp_proto,
            False, 1]
    require().mlp3(*args, **extra)


@gpu
def test_bad_last_rows_is_refused_before_any_launch():
    x, y = _data(96, seed=1)
    eng = _engine(32, 64, 32, x, y)
    eng.begin_epoch(_order(96, 1), 3)
    eng.run(2)
    torch.cuda.synchronize()
    names = _STATE + ("hand", "dh1t", "act", "counters")
    before = {k: getattr(eng, k).clone() for k in names}
    kw = {k: v for k, v in eng._kw3().items() if k != "last_rows"}
    kinds = (fused_mlp.MLP3_STEP, fused_mlp.MLP3_HEAD, fused_mlp.MLP3_TAIL_GRAD, fused_mlp.MLP3_TAIL_ADAM,
             fused_mlp.MLP3_PRIME, fused_mlp.MLP3_STEP1, fused_mlp.MLP3_TAIL_ACC)
    for bad in (0, 33, -1):
        for kind in kinds:
            with pytest.raises(ValueError, match="last_rows"):   # the Python wrapper
                fused_mlp.mlp3_launch(kind, stats=eng.stats, last_rows=bad, **kw)
            with pytest.raises(ValueError, match=r"code -15, nothing was launched"):   # launch_mlp3, via the binding
                _raw_mlp3(kind, kw, eng.stats, last_rows=bad)
    # a short batch on the kinds that have none
    ctx = [2, 0, 1 << 20, 1000, 0, 0, 0, 0]
    for kind, extra in ((fused_mlp.MLP3_STEP1, {}), (fused_mlp.MLP3_STEP1_DP, dict(dp_ctx=ctx, dp_proto=1)),
                        (fused_mlp.MLP3_STEP_DP, dict(dp_ctx=ctx))):
        with pytest.raises(ValueError, match="last_rows"):
            fused_mlp.mlp3_launch(kind, stats=eng.stats, last_rows=31, **extra, **kw)
        with pytest.raises(ValueError, match=r"code -15, nothing was launched"):
            _raw_mlp3(kind, kw, eng.stats, last_rows=31, **extra)
    torch.cuda.synchronize()
    for k, v in before.items():
        t = getattr(eng, k)
        bits = (lambda u: u.view(torch.int16)) if t.dtype == torch.bfloat16 else (lambda u: u)
        assert torch.equal(bits(t), bits(v)), k
    _raw_mlp3(fused_mlp.MLP3_STEP1, kw, eng.stats, last_rows=32)   # == B: the step as ever
    torch.cuda.synchronize()
    assert int(eng.counters[0]) == 3


# ------------------------------------------------------------------ 10: Trainer
def _classifier(drop_last):
    from ray_lightning_accelerators_amd.models.data import SyntheticMNIST
    from ray_lightning_accelerators_amd.models.mnist import MNISTClassifier

    class Upstream(MNISTClassifier):
        """Loaders as the upstream module builds them: PyTorch's default ``drop_last``."""

        def prepare_data(self):
            if not hasattr(self, "_train_set"):
                full = SyntheticMNIST(256, seed=0)
                self._train_set = Subset(full, list(range(113)))
                self._val_set = Subset(full, list(range(120, 192)))

        def train_dataloader(self):
            self.prepare_data()
            return DataLoader(self._train_set, batch_size=32, drop_last=drop_last)

        def val_dataloader(self):
            self.prepare_data()
            return DataLoader(self._val_set, batch_size=32, drop_last=drop_last)

    return Upstream({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": 32})


@gpu
@pytest.mark.parametrize("drop_last", [False, True], ids=["upstream", "drop_last"])
def test_trainer_trains_and_validates_the_short_batch_on_the_hip_path(tmpdir, caplog, drop_last):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    require()
    pl.seed_everything(0)
    model = _classifier(drop_last)
    calls = []
    orig = FusedMNISTStep.eval_epoch

    def counting(self, dl, n):
        res = orig(self, dl, n)
        calls.append(res is not None)
        return res

    FusedMNISTStep.eval_epoch = counting
    try:
        with caplog.at_level(logging.INFO):
            tr = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=2, checkpoint_callback=False,
                            progress_bar_refresh_rate=0, num_sanity_val_steps=0)
            assert tr.fit(model) == 1
    finally:
        FusedMNISTStep.eval_epoch = orig
    f = tr._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    assert not [r for r in caplog.records if "fused step unavailable" in r.getMessage()], caplog.text   # no fallback
    assert calls == [True, True]   # both validation passes ran fused
    torch.cuda.synchronize()
    if drop_last:
        assert tr.global_step == 6 and f.eng.n_batches == 3 and getattr(f.eng, "last_rows", 32) == 32
        assert f.eng.recent_stats(6)[:, 2].tolist() == [32.0] * 6
        return
    assert tr.global_step == 8 == f.eng.global_step == int(f.eng.counters[0])
    assert f.eng.n_batches == 4 and f.eng.last_rows == 17
    assert f.eng.recent_stats(8)[:, 2].tolist() == [32.0, 32.0, 32.0, 17.0] * 2
    f.check()
    # validation: 72 samples = 2 full batches + 8 rows, the mean of the three per-batch means
    fused = tr.run_evaluation()[0]
    f.eval_epoch = lambda dl, n: None
    eager = tr.run_evaluation()[0]
    assert abs(fused["ptl/val_loss"] - eager["ptl/val_loss"]) < 2e-2 * max(1.0, eager["ptl/val_loss"]), (fused, eager)
    assert abs(fused["ptl/val_accuracy"] - eager["ptl/val_accuracy"]) < 5e-3, (fused, eager)


# ------------------------------------------------------------------ 11: the exchange keeps today's behaviour
@gpu
def test_exchange_drops_the_short_batch_with_one_warning(caplog):
    from test_mlp3 import _loopback_ctx

    B, r = 32, 17
    x, y = _data(3 * B + r, seed=8)
    c, ctx = _loopback_ctx(2)
    kw = dict(lr=1e-3, dp_context=ctx, dp_proto="packed", dp_loop=True)
    a = _engine(32, 64, B, x, y, **kw)
    b = _engine(32, 64, B, x, y, **kw)
    assert a.one_launch_dp and b.one_launch_dp
    with caplog.at_level(logging.WARNING):
        for ep in range(2):
            order = _order(x.size(0), 30 + ep)
            a.begin_epoch(order, 4, last_rows=r)       # the drop_last=False loader
            b.begin_epoch(order[: 3 * B], 3)           # the drop_last=True loader
            assert a.n_batches == 3 and a.last_rows == B
            a.run(3)
            b.run(3)
    torch.cuda.synchronize()
    assert c.error_state() == 0, c.error_message()
    warned = [r_ for r_ in caplog.records if "short batch" in r_.getMessage()]
    assert len(warned) == 1 and "dropped" in warned[0].getMessage()
    _same_state(a, b, ("params", "exp_avg", "exp_avg_sq", "stats", "h1pre", "xring", "yring"))
    assert a.global_step == b.global_step == 6
