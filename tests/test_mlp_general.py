"""The general-width step and forward (csrc/mlp_step_general.hip: L1, L2 multiples of 32 up to
512 outside the table, 1 <= B <= 4096) against float64, stage by stage, with the ``Case`` /
``checks`` scheme, references and bounds of tests/test_mlp_wide.py and tests/mlp_reference.py
unchanged: the general workspace parks the wide step's six operands at the same offsets, so every
stage is judged from the kernel's OWN parked output of the stage before.

Widths: (96, 32) one partial column block, L1 not a power of two; (160, 96) a full plus a partial
block in both layers; (512, 512) the LDS plan's limit and the most column blocks.  Batches: 1 (63
padded rows), 64 (one slab), 65 (a second slab of one row), 257 on (160, 96) (uneven slices).
The ``nozero`` family is compared with ``cmp_equal`` wherever ``exact_certificate`` holds, by the
bound where it does not; evaluated on the CPU from float64 H1 / H2, it holds for all three GEMMs
of every case listed here, the forward's included."""
import pytest
import torch

import mlp_reference as R
import optim_reference as OR
from test_mlp_wide import CFG, DEV, Case as WideCase
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

pytestmark = pytest.mark.gpu
WIDTHS, BS = ((96, 32), (160, 96), (512, 512)), (1, 64, 65)
SHAPES = [(L1, L2, B) for L1, L2 in WIDTHS for B in BS] + [(160, 96, 257)]


class Case(WideCase):
    """``test_mlp_wide.Case`` on the general workspace (``route``: "general" on a table pair)."""

    def __init__(self, L1, L2, B, family="random", n_batches=2, route="auto"):
        super().__init__(L1, L2, B, family, n_batches)
        self.ws, self.route = fused_mlp.mlp_general_buffers(L1, L2, B, DEV), route

    def step(self, **kw):
        super().step(route=self.route, **kw)


@pytest.mark.parametrize("family", ["random", "nozero"])
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_gradients_against_fp64(L1, L2, B, family):
    c = Case(L1, L2, B, family)
    c.step(apply_adam=False)
    c.checks(c.p, 0, B, 1, c.g, f"grad {L1}/{L2} B={B} {family}")
    assert c.counters.tolist() == [1, 1]


@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_three_fused_adam_steps(L1, L2, B):
    c = Case(L1, L2, B)
    for t in (1, 2, 3):
        c.m.zero_()
        p0, v0 = c.p.clone(), c.v.clone()
        c.step(apply_adam=True)
        c.checks(p0, (t - 1) % 2, B, t, c.m, f"adam {L1}/{L2} B={B} t={t}")   # m' = the applied gradient
        ref = OR.ref_adam({"p": p0.cpu(), "g": c.m.cpu(), "m": torch.zeros_like(p0).cpu(), "v": v0.cpu()}, CFG, t=t)
        res = OR.check_adam({"p": c.p.cpu(), "m": c.m.cpu(), "v": c.v.cpu()}, ref)
        assert res.ok, res
        assert c.counters.tolist() == [t, t % 2]


def test_table_pair_on_the_general_route():
    c = Case(64, 128, 320, route="general")   # full column blocks only
    c.step(apply_adam=False)
    c.checks(c.p, 0, 320, 1, c.g, "route=general 64/128 B=320")


def _adam_case(**kw):
    """One fused step of (160, 96) at B = 65 under ``kw``, checked as an Adam step of CFG + kw."""
    ring = kw.pop("lr_ring", 0)
    cfg = OR.adam_cfg("general", lr=CFG.lr, betas=CFG.betas, **kw)
    c = Case(160, 96, 65)
    p0 = c.p.clone()
    step = dict(weight_decay=cfg.wd, adamw=cfg.adamw)
    if ring:   # optimizer step 1 reads entry 0 of a ring of four
        step.update(lr=123.0, lr_tensor=torch.tensor([cfg.lr, 7.0, 7.0, 7.0], device=DEV), lr_mask=3)
    else:
        step.update(lr=cfg.lr)
    c.step(apply_adam=True, **step)
    c.checks(p0, 0, 65, 1, c.m, f"adam {kw} ring={ring}")
    ref = OR.ref_adam({"p": p0.cpu(), "g": c.m.cpu(), "m": torch.zeros_like(p0).cpu(), "v": torch.zeros_like(p0).cpu()},
                      cfg, t=1)
    res = OR.check_adam({"p": c.p.cpu(), "m": c.m.cpu(), "v": c.v.cpu()}, ref)
    assert res.ok, res


@pytest.mark.parametrize("kw", [dict(wd=0.1, adamw=True), dict(lr_ring=4)], ids=["adamw", "lr_ring"])
def test_adamw_and_the_lr_ring(kw):
    _adam_case(**kw)


def test_accumulate_short_batch_and_f32_mode():
    a, b = Case(160, 96, 65), Case(160, 96, 65)
    plant = torch.randn(a.g.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    a.step(apply_adam=False)
    b.g.copy_(plant)
    b.step(apply_adam=False, accumulate_grad=True)
    assert torch.equal(b.g, a.g + plant)
    idx = a.order[:65]                              # the same pixels as fp32 rows: bitwise the u8 step
    f = Case(160, 96, 65)
    f.step(x_f32=fused_mlp.u8_to_input(a.x[idx]).to(DEV), labels=a.y[idx].to(DEV), apply_adam=False)
    assert torch.equal(f.g, a.g) and torch.equal(f.stats[0], a.stats[0])
    s = Case(160, 96, 65)                           # five rows at the epoch's last cursor
    s.counters[1] = 1
    s.step(apply_adam=False, last_rows=5)
    s.checks(s.p, 1, 5, 1, s.g, "last_rows=5")
    assert s.counters.tolist() == [1, 0]


@pytest.mark.parametrize("L1,L2", WIDTHS)
@pytest.mark.parametrize("n", [97, 32])
def test_forward_against_fp64(L1, L2, n):
    """``mlp_eval`` on +-1 pixels (a Normalize map) and dyadic weights, tests/test_mlp3_stages_fp64.py's
    scheme: layers 1 and 2 certified exact, layer 3 by its certificate's verdict; each log-prob within
    2 max ez + 2^-16 (|z| + |lse|); every 32-row chunk's (sum NLL, #correct) against the kernel's own
    log-probs (32 U24 sum |lp|), the count between ``row_nll``'s certain and certain + ambiguous rows;
    both ``out`` forms; rows past n untouched."""
    seed = 11 * L1 + 5 * L2 + n
    params, (x, y), aff = R.exact_params(L1, L2, seed), R.exact_data(n + 9, seed), fused_mlp.input_affine(R.NORM_PM1)
    idx = torch.randperm(n + 9, generator=torch.Generator().manual_seed(seed))[:n]
    X, yb = R.ref_gather(x, y, idx, n, *aff)
    W1, b1, W2, b2, W3, b3 = fused_mlp.mlp_unpack(params.double(), L1, L2).values()
    assert R.exact_certificate(X, W1, b1).ok
    H1 = torch.relu(X @ W1.t() + b1).to(torch.bfloat16).double()
    assert R.exact_certificate(H1, W2, b2).ok
    H2 = torch.relu(H1 @ W2.t() + b2).to(torch.bfloat16).double()
    Z, ez = R.ref_logits(H2, W3, b3)
    if R.exact_certificate(H2, W3, b3).ok:
        ez = torch.zeros_like(ez)
    emax, m = ez.max(1, keepdim=True).values, Z.max(1, keepdim=True).values
    lse = m + torch.log(torch.exp(Z - m).sum(1, keepdim=True))
    nch = (n + 31) // 32
    kw = dict(L1=L1, L2=L2, B=n, x_u8=x.to(DEV), index=idx.to(DEV), labels=y.to(DEV), x_scale=aff[0], x_shift=aff[1])
    logits, out = torch.full((nch * 32 + 32, 10), -7777.0, device=DEV), torch.full((nch, 2), -5.0, device=DEV)
    fused_mlp.mlp_eval(params.to(DEV), out=out, logits=logits, **kw)
    acc = torch.tensor([3.0, 4.0], device=DEV)
    fused_mlp.mlp_eval(params.to(DEV), out=acc, **kw)
    lp, o, a = logits.cpu().double(), out.cpu().double(), acc.cpu().double()
    res = [("logp", R.cmp_bound(lp[:n], Z - lse, 2.0 * emax + R.SOFT * (Z.abs() + lse.abs()))),
           ("untouched", R.cmp_equal(lp[n:], torch.full_like(lp[n:], -7777.0)))]
    nll, sure, amb = (torch.zeros(nch * 32, dtype=torch.float64) for _ in range(3))
    nll[:n] = -lp[:n].gather(1, yb.view(-1, 1)).squeeze(1)
    _, _, right, maybe = R.row_nll(Z, ez, yb)
    sure[:n], amb[:n] = right.double(), maybe.double()
    per, lo, hi = nll.view(nch, 32), sure.view(nch, 32).sum(1), (sure + amb).view(nch, 32).sum(1)
    res += [("chunk_nll", R.cmp_bound(o[:, 0], per.sum(1), 32 * R.U24 * per.abs().sum(1))),
            ("acc_nll", R.cmp_bound(a[0:1] - 3.0, nll.sum().view(1), (nch * 32 * R.U24 * (nll.abs().sum() + 3.0)).view(1)))]
    assert bool(((o[:, 1] >= lo) & (o[:, 1] <= hi)).all()) and lo.sum() <= a[1] - 4.0 <= hi.sum(), (o[:, 1], lo, hi, a)
    assert not R.report(f"forward {L1}/{L2} n={n}", res), R.report(f"forward {L1}/{L2} n={n}", res)


def _engine(L1=96, L2=160, B=65):
    c = Case(L1, L2, B)
    eng = FusedMLPEngine(L1, L2, B, lr=CFG.lr, device=DEV, init_params=c.p.cpu(), stats_ring=8)
    eng.attach_dataset(c.x, c.y)
    eng.begin_epoch(c.order, 2)
    return c, eng


def _same(e, f):
    return all(torch.equal(getattr(e, k), getattr(f, k)) for k in ("params", "exp_avg", "exp_avg_sq", "stats"))


def test_engine_equals_the_op_and_replays_bitwise():
    c, eng = _engine()
    eng.run(4)
    for _ in range(4):
        c.step(apply_adam=True, betas=(0.9, 0.999))
    assert eng.general and torch.equal(eng.params, c.p) and torch.equal(eng.stats, c.stats)
    assert eng.counters[:2].tolist() == [4, 0]
    _, twin = _engine()
    twin.run(4)
    assert _same(eng, twin)                       # two runs from one state
    _, graph = _engine()
    assert graph.capture(1, remainders=False)     # one real warm-up step, then four replays
    graph.run(4)
    eng.run(1)
    torch.cuda.synchronize()
    assert graph._graph is not None and _same(eng, graph)


@pytest.mark.parametrize("L1,L2", [(48, 64), (544, 64), (0, 64), (64, 48)])
def test_widths_without_a_kernel_are_refused(L1, L2):
    p = torch.zeros(max(fused_mlp.mlp_param_count(L1, L2), 1), device=DEV)
    with pytest.raises(ValueError, match="no fused MLP kernel"):
        fused_mlp.mlp_train_step(p, torch.zeros_like(p), L1=L1, L2=L2, B=8, labels=torch.zeros(8, dtype=torch.long, device=DEV),
                                 x_f32=torch.zeros(8, 784, device=DEV), route="general")


@pytest.mark.parametrize("short", ["park", "part"])
def test_a_short_workspace_is_refused(short):
    c = Case(96, 32, 8)
    before = c.p.clone()
    c.ws[short] = c.ws[short][:-1]
    with pytest.raises(ValueError, match="workspace too small"):
        c.step(apply_adam=True)
    assert torch.equal(c.p, before) and c.counters.tolist() == [0, 0]


def test_trainer_fits_general_widths_on_the_fused_step(tmpdir):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep, MNISTClassifier

    def fit(sub):
        pl.seed_everything(0)
        model = MNISTClassifier({"layer_1": 96, "layer_2": 160, "lr": 1e-3, "batch_size": 32})
        tr = pl.Trainer(default_root_dir=str(tmpdir.join(sub)), gpus=1, max_epochs=1, limit_train_batches=6,
                        limit_val_batches=2, checkpoint_callback=False, progress_bar_refresh_rate=0,
                        num_sanity_val_steps=0)
        assert tr.fit(model) == 1
        assert isinstance(tr._fused, FusedMNISTStep) and tr._fused.eng is not None and tr._fused.eng.general
        assert tr._fused.eng.global_step == 6 and tr.global_step == 6
        assert torch.isfinite(tr.callback_metrics["loss"]).all() and "ptl/val_loss" in tr.callback_metrics
        return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), tr.callback_metrics["ptl/val_loss"].cpu()

    (p1, v1), (p2, v2) = fit("a"), fit("b")
    assert torch.equal(p1, p2) and torch.equal(v1, v2)
