"""Gradient accumulation on the fused MNIST step's HIP path (GPU): the adding GRAD tail and
the ACC tail (csrc/mlp_step3.hip), the engine's ``accumulate=K`` route, its graph capture,
the per-micro-batch stats rows and the Trainer's ``accumulate_grad_batches``.
Bounds: tests/optim_reference.py; the CPU semantics: tests/test_mlp3_accumulate_reference.py.

Shapes: (32, 64) has two H1pre copies, (128, 256) one copy and eight tail waves; B = 32 is
one head chunk, 5 pads rows inside one chunk, 48 is a multi-chunk head (stats from the
tail, Bp = 64).  n_batches = 5: K = 2 gives windows 2, 2, 1 and K = 4 gives 4, 1."""
import math

import pytest
import torch
import torch.nn.functional as F

import optim_reference as O
from ray_lightning_accelerators_amd.ops import fused_mlp, require
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices

gpu = pytest.mark.gpu
_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
_STATE = ("params", "exp_avg", "exp_avg_sq", "shadow", "stats", "h1pre", "xring", "yring", "grads")
SHAPES = [(L1, L2, B) for (L1, L2) in ((32, 64), (128, 256)) for B in (32, 5, 48)]
NB = 5


def _dev():
    return torch.device("cuda", 0)


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _n(B, nb=NB):
    """rows of a dataset that gives exactly ``nb`` batches of B, with rows to spare"""
    return nb * B + min(8, B - 1)


def _engine(L1, L2, B, x, y, **kw):
    kw.setdefault("lr", 1e-2)
    eng = FusedMLPEngine(L1, L2, B, device=_dev(), **kw)
    eng.set_data(x, y)
    assert eng.n_batches == (x.size(0) // B)
    return eng


def _world2(eng):
    """World size 2 faked after set_data (as test_inactive_clip_is_bitwise_noop): the same
    shard on the split route.  Later epochs keep the world-1 shard the buffers were sized for."""
    eng.world_size = 2
    fill = eng._fill_order

    def fill_world1(epoch):
        eng.world_size = 1
        try:
            fill(epoch)
        finally:
            eng.world_size = 2

    eng._fill_order = fill_world1
    return eng


def _same_state(a, b, extra=()):
    torch.cuda.synchronize()
    assert torch.equal(a.counters.cpu(), b.counters.cpu()), (a.counters, b.counters)
    for k in _STATE + tuple(extra):
        pa, pb = getattr(a, k), getattr(b, k)
        assert torch.equal(pa, pb), (k, int((pa != pb).sum()), (pa.float() - pb.float()).abs().max().item())


# ------------------------------------------------------------------ 1: the adding tails
@gpu
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_accumulated_grads_are_the_exact_fp32_sum(L1, L2, B, K):
    """lr = 0: the weights never move, so a split-route twin's ``grads`` after each step are
    the single gradients g_j, and the accumulating engine must hold ((g_0 + g_1) + g_2) ...
    bitwise after every micro-batch (the ACC tail's add) and at every close (the GRAD tail's)."""
    x, y = _data(_n(B), seed=L1 + B)
    a = _engine(L1, L2, B, x, y, lr=0.0, accumulate=K)
    b = _engine(L1, L2, B, x, y, lr=0.0, allreduce=lambda g: None)
    _world2(b)  # split route: head / tail(grad) / tail(adam)
    assert not a.one_launch
    p0 = a.params.clone()
    run = None
    for i in range(2 * NB):
        a.step()
        b.step()
        pos = i % NB
        run = b.grads.clone() if pos % K == 0 else run + b.grads
        torch.cuda.synchronize()
        assert torch.equal(a.grads, run), (i, int((a.grads != run).sum()))
        assert a.optimizer_steps == int(a.counters[0]), i
    assert torch.equal(a.params, p0) and torch.equal(b.params, p0)
    assert a.optimizer_steps == 2 * math.ceil(NB / K)


# ------------------------------------------------------------------ 2: the ACC tail
@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_tail_acc_leaves_the_optimizer_alone_and_primes(L1, L2, B):
    x, y = _data(_n(B), seed=L1 + B + 1)
    a = _engine(L1, L2, B, x, y, accumulate=2)
    t = _engine(L1, L2, B, x, y, accumulate=2)
    plain = _engine(L1, L2, B, x, y, allreduce=lambda g: None)
    _world2(plain)
    for e in (a, t):
        e.run(2)  # one window: m, v away from zero
    plain.run(3)
    torch.cuda.synchronize()
    keep = {k: getattr(a, k).clone() for k in ("params", "exp_avg", "exp_avg_sq", "shadow")}
    step0 = int(a.counters[0])
    assert step0 == 1
    a.step()  # micro-batch 0 of the second window: HEAD + TAIL_ACC
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(getattr(a, k), v), k
    assert int(a.counters[0]) == step0 and a.optimizer_steps == step0
    assert torch.equal(a.counters[1:5], plain.counters[1:5]) and torch.equal(a.counters[6:10], plain.counters[6:10])
    bp = (B + 31) // 32 * 32
    per_slot = fused_mlp.mlp3_h1_copies(L1) * bp * L1
    slot = int(a.counters[3])
    assert int(a.h1pre.view(2, per_slot)[slot ^ 1].abs().max()) == 0  # the consumed slot
    assert int(a.h1pre.view(2, per_slot)[slot].abs().max()) > 0
    # the pending slot: prime() of a fresh engine with these weights at this cursor
    fresh = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), init_params=a.params)
    fresh.set_data(x, y)
    fresh.counters[0:5].copy_(a.counters[0:5])
    fresh._publish_counters()
    fresh.prime()
    torch.cuda.synchronize()
    assert torch.equal(fresh.shadow, a.shadow)
    assert torch.equal(fresh.h1pre, a.h1pre)
    # grads: a plain HEAD + TAIL_GRAD from the twin's identical state
    kw = t._kw3()
    fused_mlp.mlp3_launch(fused_mlp.MLP3_HEAD, stats=t._head_row, advance_step=False, **kw)
    fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_GRAD, stats=t.stats, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a.grads, t.grads)
    assert a.health()["saturated"] == 0 and a.health()["nonfinite"] == 0


# ------------------------------------------------------------------ 3: the update
@gpu
@pytest.mark.parametrize("clip", [None, 0.05])
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 48)])
def test_window_update_vs_fp64_adam(L1, L2, B, clip):
    """One closing window (K = 2) from a mid-training state: params / m / v against the
    float64 Adam of tests/optim_reference.py on the accumulated ``grads`` with grad_scale
    1 / K (coef / K when clipping; coef: the kernel's own), t = the optimizer step."""
    K, lr = 2, 1e-2
    x, y = _data(8 * B, seed=9)
    eng = _engine(L1, L2, B, x, y, lr=lr, accumulate=K, clip_norm=clip)
    eng.run(4)  # two windows
    torch.cuda.synchronize()
    st = {"p": eng.params.cpu().clone(), "m": eng.exp_avg.cpu().clone(), "v": eng.exp_avg_sq.cpu().clone()}
    eng.run(2)
    torch.cuda.synchronize()
    st["g"] = eng.grads.cpu().clone()
    t = int(eng.counters[0])
    assert t == 3 == eng.optimizer_steps
    coef = 1.0
    if clip:
        coef = float(eng.clip_out[1])
        assert coef < 1.0, coef
    ref = O.ref_adam(st, O.adam_cfg("window", lr=lr, grad_scale=coef / K, t=t))
    got = {"p": eng.params.cpu(), "m": eng.exp_avg.cpu(), "v": eng.exp_avg_sq.cpu()}
    cmp = O.cmp_state(got, ref, (("p", "bp"), ("m", "bm"), ("v", "bv")))
    print(f"{L1}/{L2}/{B} clip {clip}: coef {coef:.6f} {cmp.detail}")
    assert cmp.ok, cmp.detail
    fresh = torch.zeros_like(eng.shadow)
    fused_mlp.mlp_refresh_shadow(eng.params, fresh, L1, L2)
    torch.cuda.synchronize()
    lay = fused_mlp.mlp_shadow_layout(L1, L2)
    assert torch.equal(eng.shadow[: lay["np"]], fresh[: lay["np"]])
    assert torch.equal(eng.shadow[lay["w2t"]:], fresh[lay["w2t"]:])


# ------------------------------------------------------------------ 4: world 2
@gpu
@pytest.mark.parametrize("clip", [None, 0.05])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 48)])
def test_accumulating_world2_equals_world1(L1, L2, B, K, clip):
    """SUM of two identical ranks, then grad_scale 1 / (2 K): powers of two, exact.  The
    collective runs once per window."""
    x, y = _data(_n(B), seed=11)
    calls = []

    def allreduce(g):
        calls.append(1)
        g.mul_(2)

    a = _engine(L1, L2, B, x, y, accumulate=K, clip_norm=clip)
    b = _world2(_engine(L1, L2, B, x, y, accumulate=K, clip_norm=clip, allreduce=allreduce))
    a.run(2 * NB)
    b.run(2 * NB)
    torch.cuda.synchronize()
    windows = 2 * math.ceil(NB / K)
    assert len(calls) == windows == b.optimizer_steps == a.optimizer_steps
    # the allreduce doubled b's gradient arena in place
    assert torch.equal(b.grads, a.grads * 2)
    b.grads.copy_(a.grads)
    _same_state(a, b, extra=("clip_out",) if clip else ())
    if clip:
        assert int(a.clip_out[2]) == windows  # every window clipped


# ------------------------------------------------------------------ 5: graph replay
@gpu
@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("nb", [5, 7])
def test_accumulating_graph_replay_matches_eager(nb, clip):
    x, y = _data(32 * nb + 8, seed=5)
    a = _engine(32, 64, 32, x, y, lr=1e-3, accumulate=2, clip_norm=clip)
    b = _engine(32, 64, 32, x, y, lr=1e-3, accumulate=2, clip_norm=clip)
    with pytest.raises(ValueError, match="whole windows"):
        b.capture(3)
    assert b.global_step == 0
    assert b.capture(4)  # K real batches first
    assert b.global_step == 2 and sorted(b._tail_graphs) == [2]
    a.run(25)
    for n in (6, 1, 9, 7):  # dispatches that are neither multiples of the graph nor of K
        b.run(n)
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 25
    assert a.optimizer_steps == b.optimizer_steps == int(a.counters[0])
    _same_state(a, b, extra=("clip_out",) if clip else ())
    assert torch.equal(a.recent_stats(25), b.recent_stats(25))
    assert a.health() == b.health()


# ------------------------------------------------------------------ 6: reproducible
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 48)])
def test_accumulation_is_reproducible(L1, L2, B):
    x, y = _data(_n(B), seed=21)
    a = _engine(L1, L2, B, x, y, accumulate=2)
    b = _engine(L1, L2, B, x, y, accumulate=2)
    a.run(12)  # across the epoch boundary and its short last window
    b.run(12)
    _same_state(a, b)
    assert a.optimizer_steps == 7


# ------------------------------------------------------------------ 7: stats rows
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (32, 64, 5), (128, 256, 48)])
def test_one_stats_row_per_micro_batch(L1, L2, B):
    """Row i: loss / correct / count of batch i under the weights of its window (mlp_eval
    of the same batch: count and correct exact, loss within the bound tests/test_mlp3.py
    uses for stats against a forward pass), column 3 the window's optimizer step."""
    n_data = _n(B)
    x, y = _data(n_data, seed=31)
    eng = _engine(L1, L2, B, x, y, accumulate=2)
    want = []
    for i in range(2 * NB):
        epoch, cur = eng.epoch, eng.step_in_epoch
        idx = shard_indices(n_data, 1, 0, epoch, 0, True)[cur * B:(cur + 1) * B].to(_dev())
        out = torch.zeros(2, device=_dev())
        fused_mlp.mlp_eval(eng.params, L1=L1, L2=L2, B=B, labels=eng.labels, out=out, x_u8=eng.x_u8, index=idx)
        want.append((float(out[0]) / B, float(out[1])))
        eng.step()
    torch.cuda.synchronize()
    rows = eng.recent_stats(2 * NB)
    assert rows.shape == (2 * NB, 4)
    assert len({tuple(r.tolist()) for r in rows}) == 2 * NB
    assert rows[:, 3].tolist() == [1, 1, 2, 2, 3, 4, 4, 5, 5, 6]
    for i, (loss, correct) in enumerate(want):
        st = rows[i]
        print(f"{L1}/{L2}/{B} batch {i}: loss {float(st[0]):.5f} vs {loss:.5f}, correct {int(st[1])} vs {int(correct)}")
        assert int(st[2]) == B and int(st[1]) == int(correct), (i, st, correct)
        assert abs(float(st[0]) - loss) < 3e-2 * max(1.0, float(st[0])), (i, st, loss)


# ------------------------------------------------------------------ 8: misuse
def _raw_mlp3(kind, kw, stats, **extra):
    """``_C.mlp3`` without ops.fused_mlp.mlp3_launch's own argument checks."""
    b = kw["betas"]
    args = [int(kind), kw["x_u8"], kw["labels"], kw["order"], kw["counters"], kw["n_batches"], kw["B"], kw["L1"],
            kw["L2"], kw["params"], kw["grads"], kw["exp_avg"], kw["exp_avg_sq"], kw["shadow"], kw["dh1t"],
            kw["xring"], kw["h1pre"], kw["act"], kw["yring"], stats, True, kw["lr"], b[0], b[1], kw["eps"],
            kw["weight_decay"], 1.0, kw["lr_tensor"], False, None, [], kw["head_part"], kw["hand"], -1, False, 1]
    require().mlp3(*args, **extra)


@gpu
def test_accumulation_misuse_is_refused_before_any_launch():
    dev = _dev()
    x, y = _data(4 * 32, seed=2)
    eng = FusedMLPEngine(32, 64, 32, lr=1e-3, device=dev, accumulate=2, clip_norm=1.0)
    eng.set_data(x, y)
    eng.run(3)
    torch.cuda.synchronize()
    before = {k: getattr(eng, k).clone() for k in _STATE + ("counters", "clip_out", "_head_row")}
    kw = eng._kw3()
    others = (fused_mlp.MLP3_STEP, fused_mlp.MLP3_HEAD, fused_mlp.MLP3_TAIL_ADAM, fused_mlp.MLP3_PRIME,
              fused_mlp.MLP3_STEP_DP, fused_mlp.MLP3_STEP1, fused_mlp.MLP3_STEP1_DP)
    for kind in others:
        for flags in (dict(acc_add=True), dict(acc_rows=True, acc_head_row=eng._head_row),
                      dict(acc_head_row=eng._head_row)):
            with pytest.raises(ValueError, match=f"MLP3_TAIL_GRAD.*kind {kind}"):
                fused_mlp.mlp3_launch(kind, stats=eng.stats, **flags, **kw)
    # the launcher's own refusal (launch_mlp3: a negative code before any launch)
    for kind in (fused_mlp.MLP3_STEP, fused_mlp.MLP3_HEAD, fused_mlp.MLP3_TAIL_ADAM, fused_mlp.MLP3_PRIME,
                 fused_mlp.MLP3_STEP1):
        with pytest.raises(RuntimeError, match="code -10"):
            _raw_mlp3(kind, kw, eng.stats, acc_add=True)
    acc = fused_mlp.MLP3_TAIL_ACC
    part = torch.ones(32, device=dev)
    with pytest.raises(ValueError, match="MLP3_TAIL_ACC"):
        fused_mlp.mlp3_launch(acc, stats=eng.stats, clip_part=part, clip_max_norm=1.0, **kw)
    with pytest.raises(ValueError, match="MLP3_TAIL_ACC"):
        fused_mlp.mlp3_launch(acc, stats=eng.stats, clip_out=eng.clip_out, **kw)
    with pytest.raises(RuntimeError):
        _raw_mlp3(acc, kw, eng.stats, clip_part=part, clip_max_norm=1.0)
    with pytest.raises(ValueError, match="acc_rows"):
        fused_mlp.mlp3_launch(acc, stats=eng.stats, acc_rows=True, **kw)  # B <= 32: no row source
    with pytest.raises(RuntimeError, match="code -10"):
        _raw_mlp3(acc, kw, eng.stats, acc_rows=True)
    with pytest.raises(RuntimeError):
        fused_mlp.mlp3_launch(acc, stats=eng.stats, acc_rows=True, acc_head_row=torch.zeros(4), **kw)  # on the CPU
    with pytest.raises(ValueError, match="accumulate"):
        FusedMLPEngine(32, 64, 32, device=dev, accumulate=0)
    with pytest.raises(ValueError, match="dp_context"):
        FusedMLPEngine(32, 64, 32, device=dev, world_size=2, accumulate=2,
                       dp_context=[2, 0, 1 << 20, 1000, 0, 0, 0, 0])
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), k  # nothing ran


# ------------------------------------------------------------------ 9: Trainer
def _fit(tmpdir, name, **trainer_kw):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    pl.seed_everything(0)
    model = LightningMNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": 32})
    p0 = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
    trainer = pl.Trainer(default_root_dir=str(tmpdir.join(name)), gpus=1, max_epochs=1, limit_train_batches=10,
                         limit_val_batches=2, **trainer_kw)
    assert trainer.fit(model) == 1
    return trainer, model, p0


@gpu
@pytest.mark.parametrize("K,clip", [(4, 0), (2, 0.5)])
def test_trainer_accumulate_grad_batches_stays_on_the_fused_step(tmpdir, K, clip):
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    batches = 10
    trainer, model, p0 = _fit(tmpdir, f"acc{K}", accumulate_grad_batches=K, gradient_clip_val=clip)
    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    eng = f.eng
    assert eng.accumulate == K and not eng.one_launch and eng.dp_ctx is None
    assert eng.clip_norm == (clip or None)
    steps = math.ceil(batches / K)
    assert trainer.global_step == steps == int(eng.counters[0]) == eng.optimizer_steps == f.gs.step
    assert eng.global_step == batches
    order = eng.order[0].cpu()
    assert order.numel() == batches * 32
    direct = FusedMLPEngine(32, 64, 32, lr=1e-3, device=_dev(), init_params=p0, accumulate=K, clip_norm=clip or None)
    direct.attach_dataset(f._u8.cpu(), f._labels.cpu())
    direct.begin_epoch(order, batches)
    direct.run(batches)
    torch.cuda.synchronize()
    got = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert torch.equal(got, direct.params)
    assert torch.equal(eng.recent_stats(batches), direct.recent_stats(batches))


@gpu
def test_trainer_without_accumulation_keeps_the_one_launch_step(tmpdir):
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    trainer, _, _ = _fit(tmpdir, "noacc")
    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    assert f.eng.one_launch and f.eng.accumulate == 1 and not f.counts_steps
    assert trainer.global_step == 10


# ------------------------------------------------------------------ 10: loader-fed batches
@gpu
def test_loader_fed_batches_accumulate_too(tmpdir):
    """Two batches the resident path cannot serve (fp32 pixels from a loader) at K = 2: the
    first leaves the parameters alone, the second applies Adam to the summed gradient / 2."""
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    B = 32
    pl.seed_everything(0)
    model = LightningMNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": B})
    trainer = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=1, limit_train_batches=2,
                         limit_val_batches=2, accumulate_grad_batches=2)
    assert trainer.fit(model) == 1
    f = trainer._fused
    assert f.gs.step == 1 == trainer.global_step
    g = torch.Generator().manual_seed(4)
    xs = [torch.rand(B, 1, 28, 28, generator=g) for _ in range(2)]
    ys = [torch.randint(0, 10, (B,), generator=g) for _ in range(2)]
    n = f.np
    st = {"p": f.arena.data[:n].cpu().clone(), "m": f.gs.m[:n].cpu().clone(), "v": f.gs.v[:n].cpu().clone()}
    out0 = f.train_batch((xs[0], ys[0]), 0)
    torch.cuda.synchronize()
    g0 = f.arena.grad[:n].cpu().clone()
    assert torch.equal(f.arena.data[:n].cpu(), st["p"]) and torch.equal(f.gs.m[:n].cpu(), st["m"])
    assert f.gs.step == 1 == trainer.global_step
    out1 = f.train_batch((xs[1], ys[1]), 1)
    torch.cuda.synchronize()
    st["g"] = f.arena.grad[:n].cpu().clone()   # g0 + g1
    assert not torch.equal(st["g"], g0) and float(st["g"].abs().max()) > 0
    assert f.gs.step == 2 == trainer.global_step
    ref = O.ref_adam(st, O.adam_cfg("loader_acc", lr=1e-3, grad_scale=0.5, t=2))
    got = {"p": f.arena.data[:n].cpu(), "m": f.gs.m[:n].cpu(), "v": f.gs.v[:n].cpu()}
    cmp = O.cmp_state(got, ref, (("p", "bp"), ("m", "bm"), ("v", "bv")))
    assert cmp.ok, cmp.detail
    assert float(out0["loss"]) != float(out1["loss"])  # each batch keeps its own row


# ------------------------------------------------------------------ 11: trajectory
TRAJ_CLIP = 1.0


@gpu
def test_accumulating_300_batch_trajectory_vs_fp32_torch():
    """test_clipped_300_step_trajectory_vs_fp32_torch at K = 2: 300 batches, 150 optimizer
    steps, both torch twins running ``loss / 2`` backward over two batches and
    clip_grad_norm_(params, 1.0) before each optimizer step.  Same acceptance form and
    factors as that test (drift against the bf16-autocast twin's drift, loss band).
    Measured on an MI355X (profiles/r15_accumulate/README.md): engine drift 0.2906, autocast
    twin's drift 0.2492, loss 0.3439 against 0.3455."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    L1, L2, B, n, K = 32, 64, 32, 300, 2
    x, y = synthetic_mnist(B * 150, seed=13)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-3, device=_dev(), seed=3, clip_norm=TRAJ_CLIP, accumulate=K)
    eng.set_data(x, y)
    p_init = eng.params.clone()
    ref = {k: v.clone().requires_grad_(True) for k, v in
           zip(_NAMES, fused_mlp.mlp_unpack(p_init.cpu(), L1, L2).values())}
    opt = torch.optim.Adam(list(ref.values()), lr=1e-3)
    dev = _dev()
    ac = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in ref.items()}
    opt_ac = torch.optim.Adam(list(ac.values()), lr=1e-3)
    nb = eng.n_batches
    assert nb % K == 0
    losses_ref, norms_ref = [], []
    opt.zero_grad()
    opt_ac.zero_grad()
    for s in range(n):
        epoch, cur = divmod(s, nb)
        idx = shard_indices(x.size(0), 1, 0, epoch, eng.seed, True)[cur * B:(cur + 1) * B]
        xb = x[idx].float() / 255.0
        h = torch.relu(F.linear(xb, ref["W1"], ref["b1"]))
        h = torch.relu(F.linear(h, ref["W2"], ref["b2"]))
        loss = F.nll_loss(torch.log_softmax(F.linear(h, ref["W3"], ref["b3"]), 1), y[idx])
        (loss / K).backward()
        losses_ref.append(loss.item())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h = torch.relu(F.linear(xb.to(dev), ac["W1"], ac["b1"]))
            h = torch.relu(F.linear(h, ac["W2"], ac["b2"]))
            z = F.linear(h, ac["W3"], ac["b3"])
        loss_ac = F.nll_loss(torch.log_softmax(z.float(), 1), y[idx].to(dev))
        (loss_ac / K).backward()
        if (cur + 1) % K == 0:
            norms_ref.append(float(torch.nn.utils.clip_grad_norm_(list(ref.values()), TRAJ_CLIP)))
            opt.step()
            opt.zero_grad()
            torch.nn.utils.clip_grad_norm_(list(ac.values()), TRAJ_CLIP)
            opt_ac.step()
            opt_ac.zero_grad()
    frac = sum(v > TRAJ_CLIP for v in norms_ref) / len(norms_ref)
    assert eng.capture(10)
    eng.run(n - K)
    torch.cuda.synchronize()
    assert eng.optimizer_steps == n // K == int(eng.counters[0]) == len(norms_ref)
    p_ref = torch.cat([ref[k].detach().reshape(-1) for k in _NAMES])
    p_k = eng.params.cpu()
    moved = (p_ref - p_init.cpu()).norm().item()
    drift = (p_k - p_ref).norm().item() / moved
    loss_k = eng.recent_stats(50)[:, 0].mean().item()
    loss_r = sum(losses_ref[-50:]) / 50
    p_ac = torch.cat([ac[k].detach().reshape(-1) for k in _NAMES]).cpu()
    drift_ac = (p_ac - p_ref).norm().item() / moved
    h = eng.health()
    print(f"accumulating trajectory: drift {drift:.4f} autocast drift {drift_ac:.4f} loss {loss_k:.4f} vs "
          f"{loss_r:.4f}; clipped fp32 {frac:.3f} kernel {h['clipped_steps'] / (n // K):.3f}")
    assert h["nonfinite_norm_steps"] == 0
    assert drift < 1.5 * drift_ac + 0.02 and drift < 0.3, (drift, drift_ac)
    assert abs(loss_k - loss_r) < 0.05 * loss_r + 0.02, (loss_k, loss_r)
