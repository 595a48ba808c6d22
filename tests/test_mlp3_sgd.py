"""SGD inside the fused MNIST step's tail kernel (GPU): the update against the float64
reference of tests/optim_reference.py, the first-step rule, the engine's routes (two-launch,
split, clipped, accumulating, graph-replayed), misuse, a 300-step trajectory against torch
twins, and the Trainer with a ``torch.optim.SGD`` from ``configure_optimizers``."""
import pytest
import torch
import torch.nn.functional as F

import optim_reference as O
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices

gpu = pytest.mark.gpu
_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
_STATE = ("params", "momentum_buffer", "shadow", "stats", "h1pre", "xring", "yring")
SHAPES = [(32, 32, 20), (32, 64, 32), (64, 128, 48), (128, 256, 100), (64, 128, 1)]
CONFIGS = {
    "plain": dict(),
    "momentum": dict(momentum=0.9),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "dampening": dict(momentum=0.9, dampening=0.1),
    "weight_decay": dict(momentum=0.9, weight_decay=5e-4),
}
LR = 0.05
SENTINEL = -7.25


def _dev():
    return torch.device("cuda", 0)


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _same_state(a, b, extra=()):
    torch.cuda.synchronize()
    assert torch.equal(a.counters[:10].cpu(), b.counters[:10].cpu()), (a.counters, b.counters)
    for k in _STATE + tuple(extra):
        pa, pb = getattr(a, k), getattr(b, k)
        assert torch.equal(pa, pb), (k, int((pa != pb).sum()), (pa.float() - pb.float()).abs().max().item())


def _engine(L1, L2, B, cfg, world2=False, **kw):
    """``world2``: the split route head -> tail(grad) -> allreduce -> tail(sgd) on one GPU
    (two identical ranks: the SUM doubles ``grads``, grad_scale 1/2 undoes it, both exact)."""
    if world2:
        kw["allreduce"] = lambda g: g.mul_(2)
    return FusedMLPEngine(L1, L2, B, lr=LR, device=_dev(), optimizer="sgd", **cfg, **kw)


def _ref_cfg(name, cfg, **kw):
    return O.sgd_cfg(name, lr=LR, momentum=cfg.get("momentum", 0.0), dampening=cfg.get("dampening", 0.0),
                     wd=cfg.get("weight_decay", 0.0), nesterov=cfg.get("nesterov", False), **kw)


def _snapshot(eng):
    torch.cuda.synchronize()
    return {"p": eng.params.cpu().clone(), "buf": eng.momentum_buffer.cpu().clone()}


def _check_shadows(eng):
    fresh = torch.zeros_like(eng.shadow)
    fused_mlp.mlp_refresh_shadow(eng.params, fresh, eng.L1, eng.L2)
    torch.cuda.synchronize()
    assert torch.equal(eng.shadow, fresh)   # row-major, W2^T and W3^T alike


# ------------------------------------------------------------------ 1. the update
_UPDATE_CASES = [(n, 32, 64, 32) for n in CONFIGS] + [("momentum",) + s for s in SHAPES if s != (32, 64, 32)]


@gpu
@pytest.mark.parametrize("name,L1,L2,B", _UPDATE_CASES)
def test_sgd_update_vs_fp64(name, L1, L2, B):
    cfg = CONFIGS[name]
    x, y = _data(6 * B + 3, seed=L1 + L2 + B)
    eng = _engine(L1, L2, B, cfg, world2=True)
    eng.set_data(x, y)
    eng.world_size = 2   # after set_data: same shard, split optimizer path
    assert not eng.one_launch and eng.exp_avg_sq is None
    if not cfg.get("momentum"):
        eng.momentum_buffer.fill_(SENTINEL)
    eng.run(2)
    st = _snapshot(eng)
    eng.step()
    torch.cuda.synchronize()
    st["g"] = eng.grads.cpu().clone()   # the doubled gradient of step 3
    assert int(eng.counters[0]) == 3
    ref = O.ref_sgd(st, _ref_cfg(name, cfg, grad_scale=0.5, t=3))
    got = _snapshot(eng)
    cmp = O.check_sgd(got, ref)
    print(f"{name} {L1}/{L2}/{B}: {cmp.detail}")
    assert cmp.ok, cmp.detail
    if not cfg.get("momentum"):
        assert bool((got["buf"] == SENTINEL).all())   # no optimizer state is touched
    else:
        assert not torch.equal(got["buf"], st["buf"])
    _check_shadows(eng)
    h = eng.health()
    assert h["saturated"] == 0 and h["nonfinite"] == 0


# ------------------------------------------------------------------ 2. the first step
_ROUTES = {
    "two_launch": dict(),                 # head -> tail (MLP3_STEP)
    "split": dict(clip_norm=1e30),        # head -> tail(grad) -> norm partials -> tail(sgd), coef = 1: grads = gradient
    "world2": dict(world2=True),          # ... with the allreduce: grads is the doubled gradient
}


@gpu
@pytest.mark.parametrize("name", ["momentum", "nesterov", "dampening", "plain"])
@pytest.mark.parametrize("route", list(_ROUTES))
def test_sgd_first_step(name, route):
    """Step 1 overwrites the velocity with the gradient (no dampening, whatever it held);
    without momentum the buffer is never written."""
    cfg = CONFIGS[name]
    x, y = _data(4 * 32, seed=8)
    eng = _engine(32, 64, 32, cfg, **_ROUTES[route])
    eng.set_data(x, y)
    if route == "world2":
        eng.world_size = 2
    eng.momentum_buffer.fill_(SENTINEL)
    p0 = eng.params.clone()
    eng.step()
    torch.cuda.synchronize()
    assert int(eng.counters[0]) == 1
    if not cfg.get("momentum"):
        assert bool((eng.momentum_buffer == SENTINEL).all())
        return
    if route == "split":
        assert float(eng.clip_out[1]) == 1.0
        assert torch.equal(eng.momentum_buffer, eng.grads)
    elif route == "world2":
        assert torch.equal(eng.momentum_buffer, eng.grads * 0.5)   # x 2 and x 1/2 are exact
    g = eng.momentum_buffer   # (the two-launch route leaves no gradient arena behind)
    assert not bool((g == SENTINEL).any()) and bool(g.abs().max() > 0)
    # p1 = p0 - lr * d with d = g (or g + momentum g under Nesterov): a few roundings
    d = g.double() * (1.9 if cfg.get("nesterov") else 1.0)
    want = p0.double() - LR * d
    err = (eng.params.double() - want).abs()
    bound = 4 * O.U * (p0.double().abs() + (LR * d).abs()) + O.TINY
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------ 3. routes agree
@gpu
@pytest.mark.parametrize("name", ["momentum", "plain", "weight_decay"])
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (64, 128, 48)])
def test_two_launch_route_is_bitwise_the_split_route(L1, L2, B, name):
    cfg = CONFIGS[name]
    x, y = _data(8 * B, seed=7)
    a = _engine(L1, L2, B, cfg)
    b = _engine(L1, L2, B, cfg, world2=True)
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2
    for _ in range(6):
        a.step()
        b.step()
    _same_state(a, b)
    assert a.health() == b.health()


# ------------------------------------------------------------------ 4. clipping, accumulation
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 100)])
def test_clipped_sgd_update_vs_fp64(L1, L2, B):
    cfg = CONFIGS["momentum"]
    x, y = _data(6 * B, seed=9)
    eng = _engine(L1, L2, B, cfg, clip_norm=0.05)
    eng.set_data(x, y)
    eng.run(2)
    st = _snapshot(eng)
    eng.step()
    torch.cuda.synchronize()
    st["g"] = eng.grads.cpu().clone()
    coef = float(eng.clip_out[1])
    assert coef < 1.0, coef   # the bound is far below the norm of an untrained net's gradient
    assert int(eng.counters[0]) == 3
    ref = O.ref_sgd(st, _ref_cfg("clipped", cfg, grad_scale=coef, t=3))
    cmp = O.check_sgd(_snapshot(eng), ref)
    print(f"clipped {L1}/{L2}/{B}: coef {coef:.6f} {cmp.detail}")
    assert cmp.ok, cmp.detail
    _check_shadows(eng)


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (64, 128, 48)])
def test_accumulating_sgd_update_vs_fp64(L1, L2, B):
    """accumulate=2: the step that closes window 3 applies SGD to (g1 + g2) / 2."""
    cfg = CONFIGS["momentum"]
    x, y = _data(8 * B, seed=10)
    eng = _engine(L1, L2, B, cfg, accumulate=2)
    eng.set_data(x, y)
    eng.run(5)   # two windows and the first micro-batch of the third
    assert eng.optimizer_steps == 2
    st = _snapshot(eng)
    eng.step()
    torch.cuda.synchronize()
    st["g"] = eng.grads.cpu().clone()   # the window's sum
    assert int(eng.counters[0]) == 3 and eng.optimizer_steps == 3
    ref = O.ref_sgd(st, _ref_cfg("accumulated", cfg, grad_scale=0.5, t=3))
    cmp = O.check_sgd(_snapshot(eng), ref)
    print(f"accumulate {L1}/{L2}/{B}: {cmp.detail}")
    assert cmp.ok, cmp.detail
    _check_shadows(eng)


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 100)])
def test_clipped_sgd_world2_equals_world1(L1, L2, B):
    cfg = CONFIGS["momentum"]
    x, y = _data(8 * B, seed=11)
    a = _engine(L1, L2, B, cfg, clip_norm=0.05)
    b = _engine(L1, L2, B, cfg, clip_norm=0.05, world2=True)
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2
    for _ in range(6):
        a.step()
        b.step()
    _same_state(a, b, extra=("clip_out",))
    assert int(a.clip_out[2]) == 6   # every step clipped


# ------------------------------------------------------------------ 5. graph replay
@gpu
@pytest.mark.parametrize("nb", [5, 7])
@pytest.mark.parametrize("clip", [None, 0.5])
def test_sgd_graph_replay_matches_eager(nb, clip):
    """clip None: head -> tail(sgd); clip 0.5: head -> tail(grad) -> norm partials -> tail(sgd)."""
    x, y = _data(32 * nb + 8, seed=5)
    a = _engine(32, 64, 32, CONFIGS["momentum"], clip_norm=clip)
    b = _engine(32, 64, 32, CONFIGS["momentum"], clip_norm=clip)
    a.set_data(x, y)
    b.set_data(x, y)
    assert b.capture(3, remainders=True)
    assert sorted(b._tail_graphs) == [1, 2]
    a.run(24)
    for n in (6, 1, 9, 7):   # dispatches that are not multiples of 3; epochs of nb batches end inside them
        b.run(n)
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 24
    _same_state(a, b, extra=("clip_out",) if clip else ())
    assert a.health() == b.health()


# ------------------------------------------------------------------ 6. misuse
@gpu
def test_sgd_misuse_is_refused_before_any_launch():
    dev = _dev()
    x, y = _data(4 * 32, seed=2)
    eng = _engine(32, 64, 32, CONFIGS["momentum"])
    eng.set_data(x, y)
    eng.run(1)
    torch.cuda.synchronize()
    before = {k: getattr(eng, k).clone() for k in _STATE + ("counters", "grads")}
    kw = eng._kw3()
    assert kw["exp_avg_sq"] is None
    for kind in (fused_mlp.MLP3_HEAD, fused_mlp.MLP3_TAIL_GRAD, fused_mlp.MLP3_PRIME, fused_mlp.MLP3_STEP_DP,
                 fused_mlp.MLP3_STEP1, fused_mlp.MLP3_STEP1_DP, fused_mlp.MLP3_TAIL_ACC):
        with pytest.raises(ValueError, match="MLP3_STEP / MLP3_TAIL_ADAM"):
            fused_mlp.mlp3_launch(kind, stats=eng.stats, sgd_momentum=0.9, **kw)
        with pytest.raises(ValueError, match="MLP3_STEP / MLP3_TAIL_ADAM"):
            fused_mlp.mlp3_launch(kind, stats=eng.stats, sgd_momentum=0.0, **kw)
    for kind in (fused_mlp.MLP3_STEP, fused_mlp.MLP3_TAIL_ADAM):
        with pytest.raises(ValueError, match="velocity"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.9, **{**kw, "exp_avg": None})
        with pytest.raises(ValueError, match="Nesterov"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.9, sgd_dampening=0.1, sgd_nesterov=True, **kw)
        with pytest.raises(ValueError):
            fused_mlp.mlp3_launch(kind, sgd_momentum=-0.1, **kw)
        # a velocity off the 16-byte boundary never reaches the kernel's float4 accesses
        off = torch.zeros(eng.params.numel() + 1, device=dev)[1:]
        with pytest.raises(RuntimeError, match="aligned"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.9, **{**kw, "exp_avg": off})
        # Adam's launches still need both moments
        with pytest.raises(RuntimeError, match="exp_avg_sq"):
            fused_mlp.mlp3_launch(kind, **kw)
    with pytest.raises(ValueError, match="dp_context"):
        FusedMLPEngine(32, 64, 32, device=dev, world_size=2, optimizer="sgd",
                       dp_context=[2, 0, 1 << 20, 1000, 0, 0, 0, 0])
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k   # nothing ran


# ------------------------------------------------------------------ 7. trajectory
TRAJ_LR = 0.05


@gpu
def test_sgd_300_step_trajectory_vs_fp32_torch():
    """test_clipped_300_step_trajectory_vs_fp32_torch's construction with
    torch.optim.SGD(lr=0.05, momentum=0.9) in both torch twins and in the engine.

    The fp32 twin on this batch order (measured on the CPU): mean loss 1.4126 over the first
    50 steps, 0.3206 over the last 50, no step above 2.34; largest 16-pixel sum of |W1| 1.71,
    far from the +-32 clamp of the layer-1 fixed point.  The learning rate stays 0.05."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    L1, L2, B, n = 32, 64, 32, 300
    x, y = synthetic_mnist(B * 150, seed=13)
    eng = FusedMLPEngine(L1, L2, B, lr=TRAJ_LR, device=_dev(), seed=3, optimizer="sgd", momentum=0.9)
    eng.set_data(x, y)
    p_init = eng.params.clone()
    ref = {k: v.clone().requires_grad_(True) for k, v in
           zip(_NAMES, fused_mlp.mlp_unpack(p_init.cpu(), L1, L2).values())}
    opt = torch.optim.SGD(list(ref.values()), lr=TRAJ_LR, momentum=0.9)
    dev = _dev()
    ac = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in ref.items()}
    opt_ac = torch.optim.SGD(list(ac.values()), lr=TRAJ_LR, momentum=0.9)
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
    first, loss_r = sum(losses_ref[:50]) / 50, sum(losses_ref[-50:]) / 50
    assert loss_r < 0.5 * first, (first, loss_r)   # the reference trains: a stable learning rate
    assert eng.capture(10)
    eng.run(n - 1)
    torch.cuda.synchronize()
    p_ref = torch.cat([ref[k].detach().reshape(-1) for k in _NAMES])
    p_k = eng.params.cpu()
    moved = (p_ref - p_init.cpu()).norm().item()
    drift = (p_k - p_ref).norm().item() / moved
    loss_k = eng.recent_stats(50)[:, 0].mean().item()
    p_ac = torch.cat([ac[k].detach().reshape(-1) for k in _NAMES]).cpu()
    drift_ac = (p_ac - p_ref).norm().item() / moved
    h = eng.health()
    print(f"sgd trajectory: drift {drift:.4f} autocast drift {drift_ac:.4f} loss {loss_k:.4f} vs {loss_r:.4f} "
          f"(first 50: {first:.4f}); health {h}")
    assert h["saturated"] == 0 and h["nonfinite"] == 0
    assert drift < 1.5 * drift_ac + 0.02 and drift < 0.3, (drift, drift_ac)
    assert abs(loss_k - loss_r) < 0.05 * loss_r + 0.02, (loss_k, loss_r)


# ------------------------------------------------------------------ 8. Trainer
def _sgd_model(scheduler=False):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    class SGDClassifier(LightningMNISTClassifier):
        def configure_optimizers(self):
            opt = torch.optim.SGD(self.parameters(), lr=LR, momentum=0.9)
            if scheduler:
                return [opt], [torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)]
            return opt

    pl.seed_everything(0)
    return SGDClassifier({"layer_1": 32, "layer_2": 64, "lr": LR, "batch_size": 32})


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


@gpu
def test_trainer_with_sgd_stays_on_the_fused_step(tmpdir):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    steps = 40
    model = _sgd_model()
    p0 = _flat(model).clone()
    trainer = pl.Trainer(default_root_dir=str(tmpdir.join("fit")), gpus=1, max_epochs=1, limit_train_batches=steps,
                         limit_val_batches=2)
    assert trainer.fit(model) == 1
    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    eng = f.eng
    assert eng.sgd and eng.one_launch is False and eng.dp_ctx is None and eng.momentum == 0.9
    assert int(eng.counters[0]) == steps and f.gs.step == steps
    # the same 40 batches through an engine of its own, from the same init
    order = eng.order[0].cpu()
    assert order.numel() == steps * 32
    direct = FusedMLPEngine(32, 64, 32, lr=LR, device=_dev(), init_params=p0, optimizer="sgd", momentum=0.9)
    direct.attach_dataset(f._u8.cpu(), f._labels.cpu())
    direct.begin_epoch(order, steps)
    direct.run(steps)
    torch.cuda.synchronize()
    assert torch.equal(_flat(model), direct.params)
    assert torch.equal(eng.momentum_buffer, direct.momentum_buffer)
    assert trainer.fused_step_health["saturated"] == 0
    # the optimizer's state is torch's: a stock SGD loads it
    opt = trainer.optimizers[0]
    sd = opt.state_dict()
    stock = torch.optim.SGD([torch.zeros_like(p) for p in model.parameters()], lr=1.0)
    stock.load_state_dict(sd)
    bufs = torch.cat([stock.state[p]["momentum_buffer"].reshape(-1) for p in stock.param_groups[0]["params"]])
    assert torch.equal(bufs.to(_dev()), eng.momentum_buffer)
    assert stock.param_groups[0]["momentum"] == 0.9 and stock.param_groups[0]["lr"] == LR
    # ... and a fit resumed from the checkpoint goes on from that velocity
    path = str(tmpdir.join("sgd.ckpt"))
    trainer.save_checkpoint(path)
    p1, buf1 = _flat(model).clone(), eng.momentum_buffer.clone()
    model2 = _sgd_model()
    # (the checkpoint written after the fit names epoch 2 as the next one)
    t2 = pl.Trainer(default_root_dir=str(tmpdir.join("resume")), gpus=1, max_epochs=3, limit_train_batches=steps,
                    limit_val_batches=2, resume_from_checkpoint=path)
    assert t2.fit(model2) == 1
    f2 = t2._fused
    assert isinstance(f2, FusedMNISTStep) and f2.eng is not None and f2.eng.sgd
    # torch's SGD state has no step: the group restarts at 1 and the device counter follows it
    assert f2.gs.step == 1 + steps and int(f2.eng.counters[0]) == 1 + steps
    assert f2.eng.optimizer_steps == f2.gs.step
    again = FusedMLPEngine(32, 64, 32, lr=LR, device=_dev(), init_params=p1, optimizer="sgd", momentum=0.9)
    again.momentum_buffer.copy_(buf1)
    again.set_step(1)   # not a first step: the velocity blends
    again.attach_dataset(f2._u8.cpu(), f2._labels.cpu())
    again.begin_epoch(f2.eng.order[0].cpu(), steps)
    again.run(steps)
    torch.cuda.synchronize()
    assert torch.equal(_flat(model2), again.params)
    assert torch.equal(f2.eng.momentum_buffer, again.momentum_buffer)
    # the stats-ring slot follows the same count
    ring = f2.eng.stats.size(0)
    assert torch.equal(f2.eng.stats[(f2.gs.step - 1) % ring], again.stats[(again.optimizer_steps - 1) % ring])
    assert float(f2.eng.stats[(f2.gs.step - 1) % ring, 3]) == f2.gs.step
    # a velocity re-initialised at the resume would have given other weights
    fresh = FusedMLPEngine(32, 64, 32, lr=LR, device=_dev(), init_params=p1, optimizer="sgd", momentum=0.9)
    fresh.momentum_buffer.copy_(buf1)
    fresh.attach_dataset(f2._u8.cpu(), f2._labels.cpu())
    fresh.begin_epoch(f2.eng.order[0].cpu(), steps)
    fresh.run(steps)
    torch.cuda.synchronize()
    assert not torch.equal(fresh.params, again.params)


@gpu
def test_trainer_sgd_scheduler_moves_the_device_learning_rate(tmpdir):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    model = _sgd_model(scheduler=True)
    trainer = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=2, limit_train_batches=4,
                         limit_val_batches=2)
    assert trainer.fit(model) == 1
    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None and f.eng.sgd
    lr = trainer.optimizers[0].param_groups[0]["lr"]
    assert lr == LR * 0.25   # two epochs, gamma 0.5
    assert f.eng.lr_tensor is f.lr_tensor
    f.on_lr_change()
    assert float(f.lr_tensor) == pytest.approx(lr, rel=1e-7)
    # the second epoch ran at LR / 2: four more steps from the first epoch's state, on the device rate
    assert f.gs.step == 8 and int(f.eng.counters[0]) == 8


@gpu
def test_loader_fed_batch_takes_the_sgd_step(tmpdir):
    """A batch the resident path cannot serve (fp32 pixels from a loader): gradients from the
    fp32-input kernel, then the arena SGD with the same first-step rule."""
    import ray_lightning_accelerators_amd.lightning as pl

    B = 32
    model = _sgd_model()
    trainer = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=1, limit_train_batches=2,
                         limit_val_batches=2)
    assert trainer.fit(model) == 1
    f = trainer._fused
    g = torch.Generator().manual_seed(4)
    xb, yb = torch.rand(B, 1, 28, 28, generator=g), torch.randint(0, 10, (B,), generator=g)
    n = f.np
    st = {"p": f.arena.data[:n].cpu().clone(), "buf": f.gs.buf[:n].cpu().clone()}
    f.train_batch((xb, yb), 0)
    torch.cuda.synchronize()
    st["g"] = f.arena.grad[:n].cpu().clone()
    assert f.gs.step == 3
    ref = O.ref_sgd(st, O.sgd_cfg("loader", lr=LR, momentum=0.9, t=3))
    got = {"p": f.arena.data[:n].cpu(), "buf": f.gs.buf[:n].cpu()}
    cmp = O.check_sgd(got, ref)
    assert cmp.ok, cmp.detail
    # the next resident step starts from these weights, at the count the loader batch left
    f._sync_engine()
    assert f.eng.optimizer_steps == 3 and int(f.eng.counters[0]) == 3
