"""SGD and AdamW on the CPU reference engine (``FusedMLPEngine(optimizer=...)``, the oracle
of tests/test_mlp3_sgd.py): against ``torch.optim.SGD`` / ``AdamW`` on fp32 autograd, and
every refusal of the SGD arguments (engine and ``mlp3_launch``)."""
import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices

_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
L1, L2, B, NB = 32, 64, 32, 5
SGD_CONFIGS = {
    "plain": dict(),
    "momentum": dict(momentum=0.9),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "dampening": dict(momentum=0.9, dampening=0.1),
    "weight_decay": dict(momentum=0.9, weight_decay=5e-4),
}


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _torch_loop(make_opt, p_init, x, y, n_batches, K=1, clip=None, seed=0):
    ref = {k: v.clone().requires_grad_(True) for k, v in zip(_NAMES, fused_mlp.mlp_unpack(p_init, L1, L2).values())}
    opt = make_opt(list(ref.values()))
    opt.zero_grad()
    for s in range(n_batches):
        epoch, i = divmod(s, NB)
        idx = shard_indices(x.size(0), 1, 0, epoch, seed, True)[i * B:(i + 1) * B]
        h = torch.relu(F.linear(x[idx].float() / 255.0, ref["W1"], ref["b1"]))
        h = torch.relu(F.linear(h, ref["W2"], ref["b2"]))
        loss = F.nll_loss(torch.log_softmax(F.linear(h, ref["W3"], ref["b3"]), 1), y[idx])
        (loss / K).backward()
        if (i + 1) % K == 0 or i + 1 == NB:
            if clip:
                torch.nn.utils.clip_grad_norm_(list(ref.values()), clip)
            opt.step()
            opt.zero_grad()
    return torch.cat([ref[k].detach().reshape(-1) for k in _NAMES]), opt


def _flat_state(opt, key):
    return torch.cat([opt.state[p][key].reshape(-1) for p in opt.param_groups[0]["params"]])


# every configuration alone; accumulate and clip_norm once each, with momentum
_CASES = [(n, {}) for n in SGD_CONFIGS] + [("momentum", dict(accumulate=2)), ("momentum", dict(clip_norm=0.05))]


@pytest.mark.parametrize("name,extra", _CASES, ids=[n + "".join("-" + k for k in e) for n, e in _CASES])
def test_sgd_engine_equals_torch_sgd(name, extra):
    cfg = SGD_CONFIGS[name]
    x, y = _data(NB * B + 8, seed=3)
    eng = FusedMLPEngine(L1, L2, B, lr=0.05, optimizer="sgd", **cfg, **extra)
    eng.set_data(x, y)
    assert eng.sgd and not eng.one_launch and eng.exp_avg_sq is None and eng.momentum_buffer is eng.exp_avg
    p_init = eng.params.clone()
    n = 5 * extra.get("accumulate", 1)   # 5 optimizer steps (the epoch's short last window included)
    steps = 0
    while steps < 5:
        eng.step()
        steps = eng.optimizer_steps
    assert int(eng.counters[0]) == 5
    want, opt = _torch_loop(lambda ps: torch.optim.SGD(ps, lr=0.05, **cfg), p_init, x, y, eng.global_step,
                            K=extra.get("accumulate", 1), clip=extra.get("clip_norm"))
    assert eng.global_step <= n
    torch.testing.assert_close(eng.params, want)
    if cfg.get("momentum"):
        torch.testing.assert_close(eng.momentum_buffer, _flat_state(opt, "momentum_buffer"))
        sd = eng.optimizer_state_dict()
        assert set(sd["state"][0]) == {"momentum_buffer"} and len(sd["state"]) == 6
    else:
        assert not eng.momentum_buffer.any()   # never written without momentum
        assert eng.optimizer_state_dict()["state"] == {}
    # torch's own SGD accepts the export
    ps = [torch.zeros_like(v) for v in fused_mlp.mlp_unpack(p_init, L1, L2).values()]
    stock = torch.optim.SGD(ps, lr=1.0, momentum=0.5)
    stock.load_state_dict(eng.optimizer_state_dict())
    g = stock.param_groups[0]
    assert g["lr"] == 0.05 and g["momentum"] == cfg.get("momentum", 0.0) and g["nesterov"] == cfg.get("nesterov", False)
    assert {"saturated": 0, "nonfinite": 0}.items() <= eng.health().items()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_engine_equals_torch_adamw(wd):
    x, y = _data(NB * B + 8, seed=4)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, weight_decay=wd, optimizer="adamw")
    eng.set_data(x, y)
    p_init = eng.params.clone()
    eng.run(5)
    want, opt = _torch_loop(lambda ps: torch.optim.AdamW(ps, lr=1e-2, weight_decay=wd), p_init, x, y, 5)
    torch.testing.assert_close(eng.params, want)
    torch.testing.assert_close(eng.exp_avg, _flat_state(opt, "exp_avg"))
    torch.testing.assert_close(eng.exp_avg_sq, _flat_state(opt, "exp_avg_sq"))
    if wd:   # decoupled decay is not Adam's L2 term
        adam = FusedMLPEngine(L1, L2, B, lr=1e-2, weight_decay=wd, init_params=p_init)
        adam.set_data(x, y)
        adam.run(5)
        assert not torch.equal(adam.params, eng.params)


def test_adam_is_bitwise_the_engine_without_the_argument():
    x, y = _data(NB * B + 8, seed=5)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, weight_decay=0.01)
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, weight_decay=0.01, optimizer="adam")
    for e in (a, b):
        e.set_data(x, y)
        e.run(2 * NB)
    for k in ("params", "exp_avg", "exp_avg_sq", "grads", "stats", "counters", "shadow"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert b.momentum_buffer is None and b.optimizer == "adam"


def test_engine_refuses_bad_optimizer_arguments():
    with pytest.raises(ValueError, match="optimizer"):
        FusedMLPEngine(L1, L2, B, optimizer="rmsprop")
    with pytest.raises(ValueError, match="dp_context"):
        FusedMLPEngine(L1, L2, B, world_size=2, optimizer="sgd", dp_context=[2, 0, 1 << 20, 1000, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="momentum"):
        FusedMLPEngine(L1, L2, B, optimizer="sgd", momentum=-0.1)
    with pytest.raises(ValueError, match="Nesterov"):
        FusedMLPEngine(L1, L2, B, optimizer="sgd", nesterov=True)
    with pytest.raises(ValueError, match="Nesterov"):
        FusedMLPEngine(L1, L2, B, optimizer="sgd", momentum=0.9, dampening=0.1, nesterov=True)
    for opt in ("adam", "adamw"):
        with pytest.raises(ValueError, match="optimizer='sgd'"):
            FusedMLPEngine(L1, L2, B, optimizer=opt, momentum=0.9)


def test_mlp3_launch_refuses_misplaced_sgd_arguments():
    """The Python-side checks run before the extension is touched: no GPU needed."""
    eng = FusedMLPEngine(L1, L2, B, optimizer="sgd", momentum=0.9)
    x, y = _data(NB * B, seed=6)
    eng.set_data(x, y)
    kw = eng._kw3()
    for kind in (fused_mlp.MLP3_HEAD, fused_mlp.MLP3_TAIL_GRAD, fused_mlp.MLP3_PRIME, fused_mlp.MLP3_STEP_DP,
                 fused_mlp.MLP3_STEP1, fused_mlp.MLP3_STEP1_DP, fused_mlp.MLP3_TAIL_ACC):
        with pytest.raises(ValueError, match="MLP3_STEP / MLP3_TAIL_ADAM"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.9, **kw)
        with pytest.raises(ValueError, match="MLP3_STEP / MLP3_TAIL_ADAM"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.0, **kw)
    for kind in (fused_mlp.MLP3_STEP, fused_mlp.MLP3_TAIL_ADAM):
        with pytest.raises(ValueError, match="velocity"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.9, **{**kw, "exp_avg": None})
        with pytest.raises(ValueError, match="Nesterov"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.0, sgd_nesterov=True, **kw)
        with pytest.raises(ValueError, match="Nesterov"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=0.9, sgd_dampening=0.1, sgd_nesterov=True, **kw)
        with pytest.raises(ValueError, match=">= 0"):
            fused_mlp.mlp3_launch(kind, sgd_momentum=-0.5, **kw)
        with pytest.raises(ValueError, match="need sgd_momentum"):
            fused_mlp.mlp3_launch(kind, sgd_dampening=0.1, **kw)
