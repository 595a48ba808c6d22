"""Layer widths that are no multiples of 32 on the general-width step and forward (the ragged
instances of csrc/mlp_step_general.hip): tests/test_mlp_general.py's ``Case`` / ``checks`` with the
references and bounds of tests/mlp_reference.py at the TRUE widths.  The leak test plants ``-Inf`` in
``b2[0]``, the word behind W2's last row: +Inf would reach every logit and leave nothing to compare,
-Inf is relu'd to 0 in the kernel and in float64 alike and still makes an over-read pad 0 x Inf = NaN."""
import logging

import pytest
import torch

import optim_reference as OR
import test_mlp_general as G
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

pytestmark = pytest.mark.gpu
DEV, CFG = G.DEV, G.CFG
PAIRS, BS = ((33, 31), (1, 1), (65, 17), (300, 100), (511, 509), (96, 40)), (1, 33, 65)
LEAK = ((33, 31), (300, 100))


def pad32(w):
    return -(-w // 32) * 32


class Case(G.Case):
    def __init__(self, L1, L2, B, **kw):
        super().__init__(L1, L2, B, route="general", **kw)

    def obs(self):   # the workspace parks the layer widths rounded up to 32: the true rows of each operand
        lay = fused_mlp.mlp_general_layout(self.L1, self.L2, self.B)
        park, Bp, out = self.ws["park"].cpu().double(), lay["Bp"], {}
        for k, n in (("xt", 784), ("h1t", self.L1), ("h2t", self.L2), ("dh2t", self.L2), ("dzt", 16), ("dh1t", self.L1)):
            out[k[:-1]] = park[lay[k]:lay[k] + n * Bp].view(n, Bp).t().contiguous()
        return out


def guarded(t):   # ``t`` inside a larger buffer, four NaN words before and after it
    buf = torch.full((t.numel() + 8,), float("nan"), device=t.device)
    buf[4:-4] = t
    return buf, buf[4:-4]


@pytest.mark.parametrize("B,last", [(1, None), (33, None), (65, None), (33, 5)])   # 5 rows: the epoch's short last batch
@pytest.mark.parametrize("L1,L2", PAIRS)
def test_step_against_fp64(L1, L2, B, last):
    c = Case(L1, L2, B)
    c.counters[1] = cur = 0 if last is None else 1
    c.step(apply_adam=False, last_rows=last)
    c.checks(c.p, cur, last or B, 1, c.g, f"ragged grad {L1}/{L2} B={B} last_rows={last}")
    assert c.counters.tolist() == [1, 1 - cur]


@pytest.mark.parametrize("L1,L2", LEAK)
def test_nothing_crosses_the_edges(L1, L2):
    plain, c = Case(L1, L2, 65), Case(L1, L2, 65)
    plain.step(apply_adam=False)
    (pbuf, c.p), (gbuf, c.g) = guarded(c.p), guarded(c.g)
    c.step(apply_adam=False)
    assert torch.equal(c.g, plain.g) and torch.equal(c.stats, plain.stats)
    for buf in (pbuf, gbuf):
        assert bool(torch.isnan(buf[:4]).all() and torch.isnan(buf[-4:]).all())
    inf = Case(L1, L2, 65)
    fused_mlp.mlp_unpack(inf.p, L1, L2)["layer_2.bias"][0] = float("-inf")
    inf.step(apply_adam=False)
    inf.checks(inf.p, 0, 65, 1, inf.g, f"-Inf in b2[0] {L1}/{L2}")   # every element finite and within bound


@pytest.mark.parametrize("L1,L2", LEAK)
def test_padded_twin_is_bitwise_the_ragged_step(L1, L2):
    c, twin = Case(L1, L2, 65), Case(pad32(L1), pad32(L2), 65)
    twin.x, twin.y, twin.order, twin.dev = c.x, c.y, c.order, c.dev
    twin.p.zero_()
    small = fused_mlp.mlp_unpack(c.p, L1, L2)
    for k, t in fused_mlp.mlp_unpack(twin.p, twin.L1, twin.L2).items():
        t[tuple(slice(0, n) for n in small[k].shape)] = small[k]
    c.step(apply_adam=False)
    twin.step(apply_adam=False)
    assert torch.equal(c.stats, twin.stats)
    got = fused_mlp.mlp_unpack(c.g, L1, L2)
    for k, t in fused_mlp.mlp_unpack(twin.g.clone(), twin.L1, twin.L2).items():
        inside = tuple(slice(0, n) for n in got[k].shape)
        assert torch.equal(t[inside], got[k]), k
        t[inside] = 0
        assert not t.any(), f"{k}: the twin's gradient outside the true extents"


def test_arena_with_aligned_tensor_starts_is_bitwise_the_dense_one(L1=33, L2=31):
    dense, c = Case(L1, L2, 33), Case(L1, L2, 33)
    dense.step(apply_adam=False)
    wide = torch.zeros(fused_mlp.mlp_param_count(L1, L2, 4), device=DEV)
    for k, t in fused_mlp.mlp_unpack(wide, L1, L2, 4).items():
        t.copy_(fused_mlp.mlp_unpack(c.p, L1, L2)[k])
    c.p, c.g = wide, torch.full_like(wide, float("nan"))
    c.m, c.v = torch.zeros_like(wide), torch.zeros_like(wide)
    lay = fused_mlp.mlp_general_layout(L1, L2, 33)
    c.ws["part"][:lay["slices"] * lay["np_pad"]] = float("nan")   # slice partials of a workspace nobody zeroed
    c.step(apply_adam=False, arena_align=4)
    want = fused_mlp.mlp_unpack(dense.g, L1, L2)
    for k, t in fused_mlp.mlp_unpack(c.g, L1, L2, 4).items():
        assert torch.equal(t, want[k]), k
        t.zero_()
    assert torch.equal(c.stats, dense.stats) and not c.g.any()   # the words between the tensors: a zero gradient


def _engine(L1, L2, B=33, **kw):
    c = Case(L1, L2, B)
    eng = FusedMLPEngine(L1, L2, B, lr=CFG.lr, betas=CFG.betas, device=DEV, init_params=c.p.cpu(), stats_ring=8, **kw)
    eng.attach_dataset(c.x, c.y)
    eng.begin_epoch(c.order, 2)
    return eng


@pytest.mark.parametrize("kw", [dict(), dict(optimizer="adamw", weight_decay=0.1)], ids=["adam", "adamw"])
@pytest.mark.parametrize("L1,L2", LEAK)
def test_three_optimizer_steps_and_their_replay(L1, L2, kw):
    cfg = OR.adam_cfg("ragged", lr=CFG.lr, betas=CFG.betas, wd=kw.get("weight_decay", 0.0), adamw="optimizer" in kw)
    eng = _engine(L1, L2, **kw)
    for t in (1, 2, 3):
        eng.exp_avg.zero_()                               # beta1 = 0: m' is the gradient the kernel applied
        p0, v0 = eng.params.clone(), eng.exp_avg_sq.clone()
        eng.run(1)
        ref = OR.ref_adam({"p": p0.cpu(), "g": eng.exp_avg.cpu(), "m": torch.zeros_like(p0).cpu(), "v": v0.cpu()}, cfg, t=t)
        res = OR.check_adam({"p": eng.params.cpu(), "m": eng.exp_avg.cpu(), "v": eng.exp_avg_sq.cpu()}, ref)
        assert res.ok, res
    eager, graph = _engine(L1, L2, **kw), _engine(L1, L2, **kw)
    eager.run(3)
    assert graph.capture(1, remainders=False)             # one real warm-up step, then two replays
    graph.run(2)
    torch.cuda.synchronize()
    assert graph._graph is not None and G._same(eager, graph)


@pytest.mark.parametrize("n", BS)
@pytest.mark.parametrize("L1,L2", PAIRS)
def test_forward_against_fp64(L1, L2, n):
    G.test_forward_against_fp64(L1, L2, n)     # log-probs per row, chunk sums, both ``out`` forms


@pytest.mark.parametrize("L1,L2,kw", [(300, 100, {}), (33, 31, {}), (33, 31, dict(gradient_clip_val=0.05)),
                                      (33, 31, dict(accumulate_grad_batches=2))], ids=["classic", "align4", "clip", "acc"])
def test_trainer_fit_matches_its_autograd_twin(tmpdir, caplog, L1, L2, kw):
    """Six batches of 32 through ``Trainer.fit`` on the fused step (33/31: ParamArena's packing, arena_align 4;
    clipping and accumulation: the loader-fed ``mlp_train_step``) and through ``Trainer(fused_step=False)``, fp32
    autograd, from the same seed.  val_loss within 2e-2 max(1, loss), the tolerance tests/test_mlp3_short_batch.py
    gives the bf16-operand forward against the fp32 one on equal weights: the weights of the two fits differ only
    by what bf16 gradients change in six Adam steps, which is small beside it.  lr = 5e-3, so that the six steps
    move val_loss by more than the tolerance and a step that does nothing, or something else, is not inside it."""
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep, MNISTClassifier

    def fit(sub, **more):
        pl.seed_everything(0)
        model = MNISTClassifier({"layer_1": L1, "layer_2": L2, "lr": 5e-3, "batch_size": 32})
        tr = pl.Trainer(default_root_dir=str(tmpdir.join(sub)), gpus=1, max_epochs=1, limit_train_batches=6,
                        limit_val_batches=2, checkpoint_callback=False, progress_bar_refresh_rate=0,
                        num_sanity_val_steps=0, **kw, **more)
        assert tr.fit(model) == 1 and tr.global_step == 6 // kw.get("accumulate_grad_batches", 1)
        return tr, float(tr.callback_metrics["ptl/val_loss"]), torch.cat([p.detach().reshape(-1) for p in model.parameters()])

    with caplog.at_level(logging.INFO):
        tr, fused, p_fused = fit("fused")
    f = tr._fused
    assert isinstance(f, FusedMNISTStep) and f.arena_align == (4 if L1 % 4 else 1)
    assert (f.eng is not None and f.eng.general and f.eng.global_step == 6) is (not kw)   # else every batch loader-fed
    assert not [r for r in caplog.records if "fused step unavailable" in r.getMessage()], caplog.text
    twin, want, p_twin = fit("autograd", fused_step=False)
    print(f"{L1}/{L2} {kw}: val_loss fused {fused:.6f} autograd {want:.6f}, max |dp| {float((p_fused - p_twin).abs().max()):.3e}")
    assert twin._fused is None and abs(fused - want) < 2e-2 * max(1.0, want), (fused, want)
