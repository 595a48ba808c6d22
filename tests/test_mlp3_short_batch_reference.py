"""The short last batch of a ``drop_last=False`` loader on the CPU reference engine
(``FusedMLPEngine.begin_epoch(..., last_rows=r)``, the oracle of tests/test_mlp3_short_batch.py)
against plain torch: three ``nn.Linear`` in fp32, ``F.nll_loss`` and ``torch.optim`` fed batches
of sizes ``[B, ..., B, r]``.

Bound: ``torch.testing.assert_close`` with its fp32 defaults (rtol 1.3e-6, atol 1e-5), the one
tests/test_mlp3_sgd_reference.py and tests/test_mlp3_accumulate_reference.py apply to the same
comparison of the reference engine with a torch optimizer."""
import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

EPOCHS = 2


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _orders(n, seed):
    g = torch.Generator().manual_seed(100 + seed)
    return [torch.randperm(n, generator=g) for _ in range(EPOCHS)]


def _torch_loop(L1, L2, p_init, x, y, orders, sizes, make_opt, K=1):
    """Plain torch over the same batches; returns (flat params, optimizer, per-batch
    (loss, correct, count) rows, optimizer steps)."""
    net = torch.nn.Sequential(torch.nn.Linear(784, L1), torch.nn.ReLU(), torch.nn.Linear(L1, L2), torch.nn.ReLU(),
                              torch.nn.Linear(L2, 10))
    lin = [net[0], net[2], net[4]]
    with torch.no_grad():
        for m, (w, b) in zip(lin, zip(*[iter(fused_mlp.mlp_unpack(p_init, L1, L2).values())] * 2)):
            m.weight.copy_(w)
            m.bias.copy_(b)
    params = [t for m in lin for t in (m.weight, m.bias)]
    opt = make_opt(params)
    opt.zero_grad()
    rows, steps = [], 0
    for order in orders:
        at = 0
        for i, sz in enumerate(sizes):
            idx = order[at:at + sz]
            at += sz
            logp = torch.log_softmax(net(x[idx].float() / 255.0), 1)
            loss = F.nll_loss(logp, y[idx])
            (loss / K).backward()
            rows.append((float(loss.detach()), float((logp.argmax(1) == y[idx]).sum()), float(sz)))
            if (i + 1) % K == 0 or i + 1 == len(sizes):
                opt.step()
                opt.zero_grad()
                steps += 1
    return torch.cat([t.detach().reshape(-1) for t in params]), opt, rows, steps


def _flat_state(opt, key):
    return torch.cat([opt.state[p][key].reshape(-1) for p in opt.param_groups[0]["params"]])


def _run_engine(L1, L2, B, r, full, x, y, orders, **kw):
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, stats_ring=64, **kw)
    assert not eng.native
    eng.attach_dataset(x, y)
    p_init = eng.params.clone()
    nb = full + (1 if r else 0)
    for order in orders:
        eng.begin_epoch(order, nb, last_rows=r or None)
        assert eng.order.size(1) == nb * B and eng.last_rows == (r or B)
        eng.run(nb)
    return eng, p_init, nb


def _compare(L1, L2, B, r, full, extra, make_opt, state_keys):
    n = full * B + r
    x, y = _data(n, seed=B + r)
    orders = _orders(n, seed=r)
    eng, p_init, nb = _run_engine(L1, L2, B, r, full, x, y, orders, **extra)
    K = extra.get("accumulate", 1)
    sizes = [B] * full + ([r] if r else [])
    want, opt, rows, steps = _torch_loop(L1, L2, p_init, x, y, orders, sizes, make_opt, K=K)
    assert eng.global_step == EPOCHS * nb and eng.optimizer_steps == steps == int(eng.counters[0])
    torch.testing.assert_close(eng.params, want)
    for k in state_keys:
        torch.testing.assert_close(getattr(eng, "exp_avg" if k == "momentum_buffer" else k), _flat_state(opt, k))
    st = eng.recent_stats(EPOCHS * nb)
    assert st[:, 2].tolist() == [row[2] for row in rows]          # the short steps count r rows
    assert st[:, 1].tolist() == [row[1] for row in rows]
    torch.testing.assert_close(st[:, 0], torch.tensor([row[0] for row in rows]))
    return eng, steps


@pytest.mark.parametrize("L1,L2,B,r", [(32, 64, 32, 17), (32, 64, 8, 1), (64, 128, 48, 40), (32, 64, 32, 0)],
                         ids=["32-64-B32-r17", "32-64-B8-r1", "64-128-B48-r40", "control-r0"])
def test_short_batch_reference_equals_torch_adam(L1, L2, B, r):
    eng, steps = _compare(L1, L2, B, r, 3, {}, lambda ps: torch.optim.Adam(ps, lr=1e-2), ("exp_avg", "exp_avg_sq"))
    assert steps == (8 if r else 6)
    if r:
        assert eng.recent_stats(1)[0, 2] == r and eng.recent_stats(5)[0, 2] == r


def test_short_batch_reference_accumulate():
    # K = 2 over [B, B, B, r]: windows (B, B) and (B, r), every micro-batch weighted 1 / K
    _, steps = _compare(32, 64, 32, 17, 3, dict(accumulate=2), lambda ps: torch.optim.Adam(ps, lr=1e-2),
                        ("exp_avg", "exp_avg_sq"))
    assert steps == 4


def test_short_batch_reference_sgd_momentum():
    _, steps = _compare(32, 64, 32, 17, 3, dict(optimizer="sgd", momentum=0.9),
                        lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=0.9), ("momentum_buffer",))
    assert steps == 8


@pytest.mark.parametrize("full", [0, 1], ids=["nb1", "nb2"])
def test_short_batch_reference_one_and_two_batches(full):
    """A single short batch per epoch (PRIME gathers it) and a full one followed by it."""
    _, steps = _compare(32, 64, 32, 11, full, {}, lambda ps: torch.optim.Adam(ps, lr=1e-2), ("exp_avg", "exp_avg_sq"))
    assert steps == EPOCHS * (full + 1)


def test_short_batch_arguments_are_checked():
    x, y = _data(80)
    eng = FusedMLPEngine(32, 64, 32)
    eng.attach_dataset(x, y)
    order = torch.arange(80)
    for bad in (0, 33, -1, 1.5, True):
        with pytest.raises(ValueError, match="last_rows"):
            eng.begin_epoch(order, 3, last_rows=bad)
    with pytest.raises(AssertionError):
        eng.begin_epoch(order[:70], 3, last_rows=16)   # 2 * 32 + 16 indices are needed
    eng.begin_epoch(order, 3, last_rows=16)
    assert eng.order.size(1) == 96 and eng.order[0, 80:].tolist() == [0] * 16   # padded with a valid index
    assert eng._short_pos(1) and eng._short_pos(2) and not eng._short_pos(0)
    eng.begin_epoch(order[:64], 2)
    assert eng.last_rows == 32 and not eng._short_pos(1)
    # the launcher's own Python-side refusals run before the extension is touched
    kw = dict(x_u8=None, labels=None, order=None, counters=None, n_batches=3, B=32, L1=32, L2=64, params=None,
              grads=None, exp_avg=None, exp_avg_sq=None, shadow=None, dh1t=None, xring=None, h1pre=None, act=None,
              yring=None)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="last_rows"):
            fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP, last_rows=bad, **kw)
    for kind in (fused_mlp.MLP3_STEP1, fused_mlp.MLP3_STEP1_DP, fused_mlp.MLP3_STEP_DP):
        with pytest.raises(ValueError, match="last_rows"):
            fused_mlp.mlp3_launch(kind, last_rows=31, **kw)
