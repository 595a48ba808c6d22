"""AdamW on the fused MNIST step (GPU): ``FusedMLPEngine(optimizer="adamw")`` passes the
decoupled weight decay every step kernel already carries (``adam1``) through each route --
split, two-launch, one-launch, the in-kernel exchange -- and the Trainer keeps a
``torch.optim.AdamW`` fit on the one-launch step."""
import pytest
import torch

import optim_reference as O
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

gpu = pytest.mark.gpu
_STATE = ("params", "exp_avg", "exp_avg_sq", "shadow", "stats", "h1pre", "xring", "yring")
LR, WD = 1e-2, 0.01


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


def _engine(L1, L2, B, optimizer="adamw", wd=WD, world2=False, **kw):
    if world2:
        kw["allreduce"] = lambda g: g.mul_(2)
    return FusedMLPEngine(L1, L2, B, lr=LR, weight_decay=wd, device=_dev(), optimizer=optimizer, **kw)


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (32, 32, 20), (64, 128, 48), (128, 256, 100), (64, 128, 1)])
def test_adamw_split_route_vs_fp64(L1, L2, B):
    x, y = _data(6 * B + 3, seed=L1 + L2 + B)
    eng = _engine(L1, L2, B, world2=True)
    eng.set_data(x, y)
    eng.world_size = 2   # after set_data: same shard, split optimizer path
    eng.run(2)
    torch.cuda.synchronize()
    st = {"p": eng.params.cpu().clone(), "m": eng.exp_avg.cpu().clone(), "v": eng.exp_avg_sq.cpu().clone()}
    eng.step()
    torch.cuda.synchronize()
    st["g"] = eng.grads.cpu().clone()   # the doubled gradient
    assert int(eng.counters[0]) == 3
    ref = O.ref_adam(st, O.adam_cfg("adamw", lr=LR, wd=WD, adamw=True, grad_scale=0.5, t=3))
    got = {"p": eng.params.cpu(), "m": eng.exp_avg.cpu(), "v": eng.exp_avg_sq.cpu()}
    cmp = O.cmp_state(got, ref, (("p", "bp"), ("m", "bm"), ("v", "bv")))
    print(f"adamw {L1}/{L2}/{B}: {cmp.detail}")
    assert cmp.ok, cmp.detail
    # decoupled: Adam's L2 reading of the same weight_decay is outside the bound somewhere
    l2 = O.ref_adam(st, O.adam_cfg("adam_l2", lr=LR, wd=WD, adamw=False, grad_scale=0.5, t=3))
    assert not O.cmp_state(got, l2, (("p", "bp"), ("m", "bm"))).ok
    fresh = torch.zeros_like(eng.shadow)
    fused_mlp.mlp_refresh_shadow(eng.params, fresh, L1, L2)
    torch.cuda.synchronize()
    assert torch.equal(eng.shadow, fresh)


@gpu
@pytest.mark.parametrize("B", [32, 20])
def test_adamw_one_launch_is_bitwise_the_split_route(B):
    x, y = _data(8 * B + 5, seed=7)
    a = _engine(32, 64, B)
    b = _engine(32, 64, B, world2=True)
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2
    assert a.one_launch and a.adamw and b.adamw
    for _ in range(6):
        a.step()
        b.step()
    _same_state(a, b)
    a.check()


@gpu
def test_adamw_two_launch_is_bitwise_the_split_route(monkeypatch):
    monkeypatch.setenv("RLA_MLP_ONE_LAUNCH", "0")
    x, y = _data(8 * 48, seed=7)
    a = _engine(64, 128, 48)
    b = _engine(64, 128, 48, world2=True)
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2
    assert not a.one_launch
    for _ in range(6):
        a.step()
        b.step()
    _same_state(a, b)


@gpu
def test_adamw_without_decay_is_bitwise_adam():
    x, y = _data(8 * 32, seed=3)
    a = _engine(32, 64, 32, optimizer="adamw", wd=0.0)
    b = _engine(32, 64, 32, optimizer="adam", wd=0.0)
    c = _engine(32, 64, 32, optimizer="adam", wd=WD)
    for e in (a, b, c):
        e.set_data(x, y)
        e.run(6)
    _same_state(a, b)
    d = _engine(32, 64, 32, optimizer="adamw", wd=WD)
    d.set_data(x, y)
    d.run(6)
    torch.cuda.synchronize()
    assert not torch.equal(c.params, d.params)   # with a decay the two optimizers part


@gpu
def test_adamw_loopback_exchange_tracks_the_one_launch_step():
    """The 2-rank loopback exchange (one process plays both ranks): two identical
    contributions average back to this rank's gradient, so after one step the weights are
    the plain one-launch AdamW step's up to the wire rounding."""
    from test_mlp3 import _loopback_ctx

    x, y = _data(8 * 32, seed=1)
    c, ctx = _loopback_ctx(2)
    kw = dict(lr=1e-3, weight_decay=0.1, device=_dev())
    lb = FusedMLPEngine(32, 64, 32, optimizer="adamw", dp_context=ctx, dp_proto="packed", dp_loop=True, **kw)
    ref = FusedMLPEngine(32, 64, 32, optimizer="adamw", **kw)
    plain = FusedMLPEngine(32, 64, 32, optimizer="adam", **kw)
    assert lb.one_launch_dp and lb.adamw and ref.one_launch
    for e in (lb, ref, plain):
        e.set_data(x, y)
        e.run(1)
    torch.cuda.synchronize()
    assert c.error_state() == 0, c.error_message()
    lb.check()
    # Adam's first update is ~lr * sign(g), blind to the 2^-22 wire rounding (the bound of
    # test_mlp3_dp_loopback_tracks_single_rank).  Against Adam with the same weight_decay the
    # exchange's step differs by at least the decay lr * wd * p of the largest weights (|p|
    # up to 1/8: 1.25e-5), and by 2 lr wherever the L2 term flips the sign of g
    d_same = (lb.params - ref.params).abs().max().item()
    d_adam = (lb.params - plain.params).abs().max().item()
    print(f"loopback adamw: vs one-launch adamw {d_same:.3e}, vs adam {d_adam:.3e}")
    assert d_same < 1e-6, d_same
    assert d_adam > 5e-6, d_adam


@gpu
def test_trainer_with_adamw_keeps_the_one_launch_step(tmpdir):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep, LightningMNISTClassifier

    class AdamWClassifier(LightningMNISTClassifier):
        def configure_optimizers(self):
            return torch.optim.AdamW(self.parameters(), lr=self.lr, weight_decay=WD)

    steps = 40
    pl.seed_everything(0)
    model = AdamWClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": 32})
    p0 = torch.cat([p.detach().reshape(-1).clone() for p in model.parameters()])
    trainer = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=1, limit_train_batches=steps,
                         limit_val_batches=2)
    assert trainer.fit(model) == 1
    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    eng = f.eng
    assert eng.one_launch is True and eng.adamw and eng.wd == WD and int(eng.counters[0]) == steps
    direct = FusedMLPEngine(32, 64, 32, lr=1e-3, weight_decay=WD, device=_dev(), init_params=p0, optimizer="adamw")
    direct.attach_dataset(f._u8.cpu(), f._labels.cpu())
    direct.begin_epoch(eng.order[0].cpu(), steps)
    direct.run(steps)
    torch.cuda.synchronize()
    got = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert torch.equal(got, direct.params)
    # torch's AdamW loads the optimizer's state
    stock = torch.optim.AdamW([torch.zeros_like(p) for p in model.parameters()], lr=1.0)
    stock.load_state_dict(trainer.optimizers[0].state_dict())
    m = torch.cat([stock.state[p]["exp_avg"].reshape(-1) for p in stock.param_groups[0]["params"]])
    assert torch.equal(m.to(_dev()), eng.exp_avg)
    assert float(stock.state[stock.param_groups[0]["params"][0]]["step"]) == steps
