"""Gradient clipping on the fused MNIST step's HIP path (GPU): the fixed-order norm
partials (csrc/optim_kernels.hip), the coefficient the ADAM tail derives on the device
(csrc/mlp_step3.hip), the engine's clipped route, its graph capture, and the Trainer's
``gradient_clip_val``.  Bounds: tests/clip_reference.py and tests/optim_reference.py."""
import pytest
import torch
import torch.nn.functional as F

import clip_reference as R
import optim_reference as O
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.ops.optim import clip_partials
from ray_lightning_accelerators_amd.parallel.mlp_engine import CLIP_NBLK, FusedMLPEngine, shard_indices

gpu = pytest.mark.gpu
_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
_STATE = ("params", "exp_avg", "exp_avg_sq", "shadow", "stats", "h1pre", "xring", "yring")


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


# ------------------------------------------------------------------ the norm kernel
@gpu
@pytest.mark.parametrize("nblk", R.NBLKS)
@pytest.mark.parametrize("n", R.SIZES)
def test_clip_partials_kernel_vs_fp64(n, nblk):
    x = R.make_input(n)
    xd = x.to(_dev())
    part = clip_partials(xd, nblk)
    again = clip_partials(xd, nblk)
    out = torch.full((nblk,), 7.0, device=_dev())
    assert clip_partials(xd, nblk, out=out) is out
    torch.cuda.synchronize()
    assert part.shape == (nblk,) and part.dtype == torch.float32
    ref_part, s, bound = R.ref_partials(x, nblk)
    err = abs(float(part.double().sum()) - s)
    print(f"clip_partials n={n} nblk={nblk}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)
    assert bool(((part.double().cpu() - ref_part).abs() <= bound).all())
    for b, (lo, hi) in enumerate(R.slices(n, nblk)):
        assert hi > lo or float(part[b]) == 0.0   # an empty slice stores 0
    assert torch.equal(part, again) and torch.equal(part, out)


@gpu
def test_clip_partials_refuses_bad_operands():
    dev = _dev()
    base = torch.ones(1024 + 1, device=dev)
    with pytest.raises(RuntimeError, match="aligned"):
        clip_partials(base[1:], 4)   # 4 bytes past a 16-byte boundary
    with pytest.raises(ValueError):
        clip_partials(base[:1024], 65)
    with pytest.raises(RuntimeError):
        clip_partials(base[:1024].double(), 4)
    with pytest.raises(ValueError):
        clip_partials(base[:1024], 4, out=torch.zeros(4))   # out on the CPU


# ------------------------------------------------------------------ norm, coefficient
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (32, 32, 20), (64, 128, 64), (128, 256, 100), (64, 128, 1)])
def test_clip_norm_and_coefficient(L1, L2, B):
    """After each step: the reported norm against the float64 norm of the gradient arena,
    the coefficient against min(1, c / (norm + 1e-6)) in fp32 from the reported norm."""
    c = 0.5
    n = fused_mlp.mlp_param_count(L1, L2)
    x, y = _data(3 * B + B // 2 + 2, seed=L1 + L2 + B)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), clip_norm=c)
    eng.set_data(x, y)
    assert not eng.one_launch and eng.clip_part.numel() == CLIP_NBLK
    clipped = 0
    for s in range(4):
        eng.step()
        torch.cuda.synchronize()
        norm64 = float(eng.grads.double().cpu().norm())
        out = eng.clip_out.cpu()
        norm32, coef = float(out[0]), float(out[1])
        bound = R.norm_bound(n, CLIP_NBLK, norm64)
        want = float(R.coef_f32(c, norm32))
        print(f"{L1}/{L2}/{B} step {s}: norm {norm32:.6f} err {abs(norm32 - norm64):.3e} bound {bound:.3e} "
              f"coef {coef:.6f} ulps {R.ulps(coef, want)}")
        assert abs(norm32 - norm64) <= bound, (s, norm32, norm64, bound)
        assert R.ulps(coef, want) <= 1, (s, coef, want)
        clipped += coef < 1.0
        assert int(out[2]) == clipped and int(out[3]) == 0
    h = eng.health()
    assert h["clipped_steps"] == clipped and h["nonfinite_norm_steps"] == 0
    assert h["clip_norm_last"] == norm32 and h["clip_coef_last"] == coef
    assert {k: h[k] for k in ("saturated", "nonfinite", "timed_out")} == {"saturated": 0, "nonfinite": 0,
                                                                          "timed_out": False}


# ------------------------------------------------------------------ the update
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 100)])
def test_clipped_update_vs_fp64_adam(L1, L2, B):
    """One clipped step from a mid-training state: params / m / v against the float64
    Adam step of tests/optim_reference.py applied to coef * grads (coef: the kernel's own,
    checked above), within that module's fp32 bound; the shadows follow the params."""
    c, lr = 0.05, 1e-2
    x, y = _data(6 * B, seed=9)
    eng = FusedMLPEngine(L1, L2, B, lr=lr, device=_dev(), clip_norm=c)
    eng.set_data(x, y)
    eng.run(2)   # m, v away from zero
    torch.cuda.synchronize()
    st = {"p": eng.params.cpu().clone(), "m": eng.exp_avg.cpu().clone(), "v": eng.exp_avg_sq.cpu().clone()}
    eng.step()
    torch.cuda.synchronize()
    st["g"] = eng.grads.cpu().clone()
    coef = float(eng.clip_out[1])
    assert coef < 1.0, coef   # c is far below the norm of an untrained net's gradient
    t = int(eng.counters[0])
    assert t == 3
    ref = O.ref_adam(st, O.adam_cfg("clipped", lr=lr, grad_scale=coef, t=t))
    got = {"p": eng.params.cpu(), "m": eng.exp_avg.cpu(), "v": eng.exp_avg_sq.cpu()}
    cmp = O.cmp_state(got, ref, (("p", "bp"), ("m", "bm"), ("v", "bv")))
    print(f"{L1}/{L2}/{B}: coef {coef:.6f} {cmp.detail}")
    assert cmp.ok, cmp.detail
    fresh = torch.zeros_like(eng.shadow)
    fused_mlp.mlp_refresh_shadow(eng.params, fresh, L1, L2)
    torch.cuda.synchronize()
    lay = fused_mlp.mlp_shadow_layout(L1, L2)
    assert torch.equal(eng.shadow[: lay["np"]], fresh[: lay["np"]])
    assert torch.equal(eng.shadow[lay["w2t"]:], fresh[lay["w2t"]:])


# ------------------------------------------------------------------ inactive clip, world 2
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (64, 128, 48)])
def test_inactive_clip_is_bitwise_noop(L1, L2, B):
    """clip_norm = 1e30 (coef = 1 every step): bitwise the un-clipped split route -- head,
    tail(grad), tail(adam) with no clip arguments, driven as
    test_mlp3_fused_matches_split drives it (two identical ranks: x2, then grad_scale 1/2,
    both exact)."""
    x, y = _data(8 * B, seed=7)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), clip_norm=1e30)
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), allreduce=lambda g: g.mul_(2))
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2  # after set_data: same shard, split optimizer path (6 steps < 2 epochs)
    assert b.clip_out is None
    for _ in range(6):
        a.step()
        b.step()
    _same_state(a, b)
    out = a.clip_out.cpu()
    assert float(out[1]) == 1.0 and int(out[2]) == 0 and int(out[3]) == 0 and float(out[0]) > 0.0


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 100)])
def test_clipped_world2_equals_world1(L1, L2, B):
    """SUM of two identical ranks then grad_scale 1/2: every partial is 4x (exact), the
    root 2x (exact), the norm, the coefficient and the update the world-1 engine's bits."""
    c = 0.05
    x, y = _data(8 * B, seed=11)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), clip_norm=c)
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), clip_norm=c, allreduce=lambda g: g.mul_(2))
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2
    for _ in range(6):
        a.step()
        b.step()
    _same_state(a, b, extra=("clip_out",))
    assert int(a.clip_out[2]) == 6   # every step clipped


# ------------------------------------------------------------------ graph replay
@gpu
@pytest.mark.parametrize("nb,gsteps,remainders", [(5, 3, False), (5, 3, True), (7, 5, True)])
def test_clipped_graph_replay_matches_eager(nb, gsteps, remainders):
    x, y = _data(32 * nb + 8, seed=5)
    a = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev(), clip_norm=0.5)
    b = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev(), clip_norm=0.5)
    a.set_data(x, y)
    b.set_data(x, y)
    assert b.capture(gsteps, remainders=remainders)
    assert sorted(b._tail_graphs) == ([k for k in (1, 2, 4) if k < gsteps] if remainders else [])
    a.run(24)
    for n in (6, 1, 9, 7):  # dispatches that are not multiples of gsteps
        b.run(n)
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 24
    _same_state(a, b, extra=("clip_out",))
    print(f"clipped steps {int(a.clip_out[2])} of 24")
    assert a.health() == b.health()


@gpu
def test_clipped_capture_7_steps_matches_eager():
    """capture(3, remainders=True) + run(7) against 7 eager steps."""
    x, y = _data(32 * 5 + 8, seed=6)
    a = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev(), clip_norm=0.5)
    b = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev(), clip_norm=0.5)
    a.set_data(x, y)
    b.set_data(x, y)
    for _ in range(8):
        a.step()
    assert b.capture(3, remainders=True)   # one real step
    b.run(7)
    _same_state(a, b, extra=("clip_out",))


# ------------------------------------------------------------------ misuse
@gpu
def test_clip_misuse_is_refused_before_any_launch():
    dev = _dev()
    x, y = _data(4 * 32, seed=2)
    eng = FusedMLPEngine(32, 64, 32, lr=1e-3, device=dev, clip_norm=1.0)
    eng.set_data(x, y)
    eng.run(1)
    torch.cuda.synchronize()
    before = {k: getattr(eng, k).clone() for k in _STATE + ("counters", "clip_out", "grads")}
    kw = eng._kw3()
    part = torch.ones(CLIP_NBLK, device=dev)
    for kind in (fused_mlp.MLP3_STEP, fused_mlp.MLP3_HEAD, fused_mlp.MLP3_TAIL_GRAD, fused_mlp.MLP3_PRIME,
                 fused_mlp.MLP3_STEP_DP, fused_mlp.MLP3_STEP1, fused_mlp.MLP3_STEP1_DP):
        with pytest.raises(ValueError, match="MLP3_TAIL_ADAM"):
            fused_mlp.mlp3_launch(kind, stats=eng.stats, clip_part=part, clip_max_norm=1.0, **kw)
        with pytest.raises(ValueError, match="MLP3_TAIL_ADAM"):
            fused_mlp.mlp3_launch(kind, stats=eng.stats, clip_out=eng.clip_out, **kw)
    adam = fused_mlp.MLP3_TAIL_ADAM
    bad = [
        dict(clip_part=torch.ones(8, device=dev), clip_nblk=CLIP_NBLK),      # shorter than nblk
        dict(clip_part=torch.ones(CLIP_NBLK)),                                 # on the CPU
        dict(clip_part=torch.ones(CLIP_NBLK, device=dev, dtype=torch.float64)),
        dict(clip_part=torch.ones(65, device=dev)),                            # more partials than a launch writes
        dict(clip_part=part, clip_out=torch.zeros(3, device=dev)),
        dict(clip_part=part, clip_out=torch.zeros(4)),
    ]
    for extra in bad:
        with pytest.raises(RuntimeError):
            fused_mlp.mlp3_launch(adam, grad_scale=1.0, clip_max_norm=1.0, **extra, **kw)
    with pytest.raises(ValueError):
        fused_mlp.mlp3_launch(adam, clip_part=part, clip_max_norm=0.0, **kw)
    with pytest.raises(ValueError):
        fused_mlp.mlp3_launch(adam, clip_max_norm=1.0, **kw)   # a bound without partials
    with pytest.raises(ValueError, match="dp_context"):
        FusedMLPEngine(32, 64, 32, device=dev, world_size=2, clip_norm=1.0,
                       dp_context=[2, 0, 1 << 20, 1000, 0, 0, 0, 0])
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k   # nothing ran


# ------------------------------------------------------------------ trajectory
TRAJ_CLIP = 1.0   # the fp32 reference below clips 155 of its 300 steps (0.517), measured on the CPU


@gpu
def test_clipped_300_step_trajectory_vs_fp32_torch():
    """test_mlp3_300_step_trajectory_vs_fp32_torch_adam with clip_grad_norm_(params, 1.0)
    before every optimizer step of both torch twins and clip_norm=1.0 in the engine."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    L1, L2, B, n = 32, 64, 32, 300
    x, y = synthetic_mnist(B * 150, seed=13)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-3, device=_dev(), seed=3, clip_norm=TRAJ_CLIP)
    eng.set_data(x, y)
    p_init = eng.params.clone()
    ref = {k: v.clone().requires_grad_(True) for k, v in
           zip(_NAMES, fused_mlp.mlp_unpack(p_init.cpu(), L1, L2).values())}
    opt = torch.optim.Adam(list(ref.values()), lr=1e-3)
    dev = _dev()
    ac = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in ref.items()}
    opt_ac = torch.optim.Adam(list(ac.values()), lr=1e-3)
    nb = eng.n_batches
    losses_ref, norms_ref = [], []
    for s in range(n):
        epoch, cur = divmod(s, nb)
        idx = shard_indices(x.size(0), 1, 0, epoch, eng.seed, True)[cur * B:(cur + 1) * B]
        xb = x[idx].float() / 255.0
        h = torch.relu(F.linear(xb, ref["W1"], ref["b1"]))
        h = torch.relu(F.linear(h, ref["W2"], ref["b2"]))
        loss = F.nll_loss(torch.log_softmax(F.linear(h, ref["W3"], ref["b3"]), 1), y[idx])
        opt.zero_grad()
        loss.backward()
        norms_ref.append(float(torch.nn.utils.clip_grad_norm_(list(ref.values()), TRAJ_CLIP)))
        opt.step()
        losses_ref.append(loss.item())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = torch.relu(F.linear(xb.to(dev), ac["W1"], ac["b1"]))
            h = torch.relu(F.linear(h, ac["W2"], ac["b2"]))
            z = F.linear(h, ac["W3"], ac["b3"])
        loss_ac = F.nll_loss(torch.log_softmax(z.float(), 1), y[idx].to(dev))
        opt_ac.zero_grad()
        loss_ac.backward()
        torch.nn.utils.clip_grad_norm_(list(ac.values()), TRAJ_CLIP)
        opt_ac.step()
    frac = sum(v > TRAJ_CLIP for v in norms_ref) / n
    assert 0.2 <= frac <= 0.8, frac
    assert eng.capture(10)
    eng.run(n - 1)
    torch.cuda.synchronize()
    p_ref = torch.cat([ref[k].detach().reshape(-1) for k in _NAMES])
    p_k = eng.params.cpu()
    moved = (p_ref - p_init.cpu()).norm().item()
    drift = (p_k - p_ref).norm().item() / moved
    loss_k = eng.recent_stats(50)[:, 0].mean().item()
    loss_r = sum(losses_ref[-50:]) / 50
    p_ac = torch.cat([ac[k].detach().reshape(-1) for k in _NAMES]).cpu()
    drift_ac = (p_ac - p_ref).norm().item() / moved
    h = eng.health()
    print(f"clipped trajectory: drift {drift:.4f} autocast drift {drift_ac:.4f} loss {loss_k:.4f} vs {loss_r:.4f}; "
          f"clipped fp32 {frac:.3f} kernel {h['clipped_steps'] / n:.3f}")
    assert h["nonfinite_norm_steps"] == 0 and 0.2 <= h["clipped_steps"] / n <= 0.8
    assert drift < 1.5 * drift_ac + 0.02 and drift < 0.3, (drift, drift_ac)
    assert abs(loss_k - loss_r) < 0.05 * loss_r + 0.02, (loss_k, loss_r)


# ------------------------------------------------------------------ Trainer
def _fit(tmpdir, clip, name):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    pl.seed_everything(0)
    model = LightningMNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": 32})
    p0 = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
    trainer = pl.Trainer(default_root_dir=str(tmpdir.join(name)), gpus=1, max_epochs=1, limit_train_batches=40,
                         limit_val_batches=2, gradient_clip_val=clip)
    assert trainer.fit(model) == 1
    return trainer, model, p0


@gpu
def test_trainer_gradient_clip_val_stays_on_the_fused_step(tmpdir):
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    clip, steps = 0.5, 40
    trainer, model, p0 = _fit(tmpdir, clip, "clip")
    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    eng = f.eng
    assert eng.clip_norm == clip and not eng.one_launch and eng.dp_ctx is None
    assert int(eng.counters[0]) == steps
    # the same 40 batches through an engine of its own, from the same init
    order = eng.order[0].cpu()
    assert order.numel() == steps * 32
    direct = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev(), init_params=p0, clip_norm=clip)
    direct.attach_dataset(f._u8.cpu(), f._labels.cpu())
    direct.begin_epoch(order, steps)
    unclipped = 0
    for _ in range(steps):
        direct.step()
        unclipped += float(direct.clip_out[1]) == 1.0
    torch.cuda.synchronize()
    h = trainer.fused_step_health
    print(f"trainer clip: clipped {h['clipped_steps']} of {steps}, last norm {h['clip_norm_last']}")
    assert h["clipped_steps"] + unclipped == steps and h["nonfinite_norm_steps"] == 0
    assert h["clipped_steps"] == direct.health()["clipped_steps"]
    assert h["clip_norm_last"] == direct.health()["clip_norm_last"]
    got = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert torch.equal(got, direct.params)


@gpu
def test_loader_fed_batch_is_clipped_too(tmpdir):
    """A batch the resident path cannot serve (fp32 pixels from a loader): gradients from
    the one-launch fp32-input kernel, scaled in place to the bound, then the arena Adam."""
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    c, B = 0.05, 32
    pl.seed_everything(0)
    model = LightningMNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": B})
    trainer = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=1, limit_train_batches=2,
                         limit_val_batches=2, gradient_clip_val=c)
    assert trainer.fit(model) == 1
    f = trainer._fused
    g = torch.Generator().manual_seed(4)
    xb, yb = torch.rand(B, 1, 28, 28, generator=g), torch.randint(0, 10, (B,), generator=g)
    n = f.np
    st = {"p": f.arena.data[:n].cpu().clone(), "m": f.gs.m[:n].cpu().clone(), "v": f.gs.v[:n].cpu().clone()}
    f.train_batch((xb, yb), 0)
    torch.cuda.synchronize()
    st["g"] = f.arena.grad[:n].cpu().clone()   # already scaled by the coefficient
    # an untrained net's gradient norm (> 0.25) is several times the bound, so the scaled norm is
    # c * norm / (norm + 1e-6): below c by less than 4e-6 relative, plus a few fp32 roundings
    norm = float(st["g"].double().norm())
    assert abs(norm - c) <= 1e-4 * c, norm
    assert f.gs.step == 3
    ref = O.ref_adam(st, O.adam_cfg("loader", lr=1e-3, t=3))
    got = {"p": f.arena.data[:n].cpu(), "m": f.gs.m[:n].cpu(), "v": f.gs.v[:n].cpu()}
    cmp = O.cmp_state(got, ref, (("p", "bp"), ("m", "bm"), ("v", "bv")))
    assert cmp.ok, cmp.detail


@gpu
def test_trainer_without_clip_keeps_the_one_launch_step(tmpdir):
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    trainer, _, _ = _fit(tmpdir, 0, "noclip")
    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    assert f.eng.one_launch and f.eng.clip_norm is None and f.eng.clip_part is None and f.eng.clip_out is None
    assert "clipped_steps" not in trainer.fused_step_health
