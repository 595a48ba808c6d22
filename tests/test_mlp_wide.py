"""The wide-batch step (csrc/mlp_step_wide.hip, 256 < B <= 4096) against float64, stage by
stage, with the references and bounds of tests/mlp_reference.py.  Each stage is judged from the
kernel's OWN parked output of the stage before (``mlp_wide_layout``: XT, H1T, H2T, dH2T, dZT,
dH1T, ``[feature][Bp]`` bf16), the weights being bf16(fp32 master), the biases fp32:

  gather  == bf16(u8_to_input(x[idx])); rows past the batch zero
  H1 H2   ``ref_h2``'s form, U8 |ref| + 2 (K + 1) U24 amp with K = 784 / L1 (layer 1 is a plain
          fp32 MFMA sum here: no fixed point); dyadic operands under the certificate: equal
  dZ dH2 dH1   ``ref_dz`` / ``ref_dh2`` / ``ref_dh1`` unchanged
  loss    ``ref_stats``' bound + (Bp + 2) U24 loss: the Bp-term fp32 sum of the rows' NLL in any
          order (sum of absolute values = rows x loss) and the product with 1 / rows
  dW db   ``grad_checks``: 2 Bp U24 amp, Bp = every summed row, whatever the slice split
  Adam    tests/optim_reference.py ``ref_adam`` / ``check_adam`` from the kernel's own previous
          state; beta1 = 0 and a zeroed ``exp_avg`` make m' the applied gradient bit for bit

B = 257: one row past the old limit, a last slab of one row; 320: whole slabs; 513: uneven K
slices.  Worst error / bound per case: profiles/r23_wide_batch/test_ratios.log."""
import pytest
import torch

import mlp_reference as R
import optim_reference as OR
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BS, WIDTHS, N = (257, 320, 513), ((32, 32), (64, 128), (128, 256)), 2048
CFG = OR.adam_cfg("wide", lr=1e-2, betas=(0.0, 0.999))


class Case:
    def __init__(self, L1, L2, B, family="random", n_batches=2):
        seed = 9000 + 7 * L1 + 3 * L2 + B
        if family == "random":
            (self.x, self.y), p, norm = R.random_data(N, seed), R.random_params(L1, L2, seed), None
        else:
            (self.x, self.y), p, norm = R.exact_data(N, seed), R.exact_params(L1, L2, seed), R.NORM_PM1
        self.L1, self.L2, self.B, self.nb, self.exact = L1, L2, B, n_batches, family != "random"
        self.affine = fused_mlp.input_affine(norm)
        self.order = torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:n_batches * B]
        z = lambda: torch.zeros(p.numel(), device=DEV)
        self.p, self.g, self.m, self.v = p.to(DEV), z(), z(), z()
        self.stats, self.counters = torch.zeros(8, 4, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
        self.ws = fused_mlp.mlp_wide_buffers(L1, L2, B, DEV)
        self.dev = [t.to(DEV) for t in (self.x, self.y, self.order)]

    def step(self, x_f32=None, labels=None, **kw):
        xd, yd, od = self.dev
        kw = {"lr": CFG.lr, "betas": CFG.betas, "eps": CFG.eps, **kw}
        data = dict(x_u8=xd, labels=yd, order=od, x_scale=self.affine[0], x_shift=self.affine[1]) \
            if x_f32 is None else dict(x_f32=x_f32, labels=labels)
        fused_mlp.mlp_train_step(self.p, self.g, L1=self.L1, L2=self.L2, B=self.B, counters=self.counters,
                                 n_batches=self.nb, exp_avg=self.m, exp_avg_sq=self.v, stats=self.stats,
                                 workspace=self.ws, **data, **kw)

    def obs(self):
        lay = fused_mlp.mlp_wide_layout(self.L1, self.L2, self.B)
        park, Bp = self.ws["park"].cpu().double(), lay["Bp"]
        rows = {"xt": 784, "h1t": self.L1, "h2t": self.L2, "dh2t": self.L2, "dzt": 16, "dh1t": self.L1}
        return {k[:-1]: park[lay[k]:lay[k] + n * Bp].view(n, Bp).t().contiguous() for k, n in rows.items()}

    def checks(self, p_before, cursor, rows, t, grad, tag):
        """Every stage of the step just run, then the flat gradient ``grad``; asserts."""
        o = self.obs()
        W = [w.to(torch.bfloat16).double() if i % 2 == 0 else w.double()
             for i, w in enumerate(fused_mlp.mlp_unpack(p_before.cpu(), self.L1, self.L2).values())]
        W1, b1, W2, b2, W3, b3 = W
        Bp = o["x"].size(0)
        Xw, yw = R.ref_gather(self.x, self.y, self.order[cursor * self.B:cursor * self.B + rows], Bp, *self.affine)
        out = [("gather", R.cmp_equal(o["x"], Xw))]
        ez0 = False
        for name, a, w, b, got in (("H1", o["x"], W1, b1, o["h1"]), ("H2", o["h1"], W2, b2, o["h2"])):
            ref, bound = R.ref_h2(a, w, b)
            sure = self.exact and R.exact_certificate(a, w, b).ok
            out.append((name, R.cmp_equal(got, ref.to(torch.bfloat16).double()) if sure else R.cmp_bound(got, ref, bound)))
            ez0 = sure
        Z, ez = R.ref_logits(o["h2"], W3, b3)
        if ez0 and R.exact_certificate(o["h2"], W3, b3).ok:
            ez = torch.zeros_like(ez)
        out.append(("dZ", R.cmp_bound(o["dz"], *R.ref_dz(Z, ez, yw, rows))))
        st, got = R.ref_stats(Z, ez, yw), self.stats[(t - 1) % 8].cpu().double()
        out.append(("loss", R.cmp_bound(got[:1], torch.tensor([st.loss], dtype=torch.float64),
                                        st.loss_bound + (Bp + 2) * R.U24 * st.loss)))
        assert st.certain <= got[1] <= st.certain + st.ambiguous and got[2:].tolist() == [rows, t], (got, st)
        w3t = torch.zeros(self.L2, 16, dtype=torch.float64)
        w3t[:, :R.NC] = W3.t()
        out.append(("dH2", R.cmp_bound(o["dh2"], *R.ref_dh2(o["dz"], w3t, o["h2"]))))
        out.append(("dH1", R.cmp_bound(o["dh1"], *R.ref_dh1(o["dh2"], W2.t().contiguous(), o["h1"]))))
        out += R.grad_checks(grad, o, self.L1, self.L2)
        assert not R.report(tag, out), R.report(tag, out)


@pytest.mark.parametrize("family", ["random", "nozero"])
@pytest.mark.parametrize("L1,L2", WIDTHS)
@pytest.mark.parametrize("B", BS)
def test_gradients_against_fp64(B, L1, L2, family):
    c = Case(L1, L2, B, family)
    c.step(apply_adam=False)
    c.checks(c.p, 0, B, 1, c.g, f"grad {L1}/{L2} B={B} {family}")
    assert c.counters.tolist() == [1, 1]


@pytest.mark.parametrize("L1,L2", WIDTHS)
@pytest.mark.parametrize("B", BS)
def test_three_fused_adam_steps(B, L1, L2):
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


def test_accumulate_short_batch_and_f32_mode():
    a, b = Case(64, 128, 320), Case(64, 128, 320)
    plant = torch.randn(a.g.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    a.step(apply_adam=False)
    b.g.copy_(plant)
    b.step(apply_adam=False, accumulate_grad=True)
    assert torch.equal(b.g, a.g + plant)
    # the same pixels as fp32 rows: bitwise the u8 step
    idx = a.order[:320]
    f = Case(64, 128, 320)
    f.step(x_f32=fused_mlp.u8_to_input(a.x[idx]).to(DEV), labels=a.y[idx].to(DEV), apply_adam=False)
    assert torch.equal(f.g, a.g) and torch.equal(f.stats[0], a.stats[0])
    # five rows at the epoch's last cursor
    s = Case(64, 128, 320)
    s.counters[1] = 1
    s.step(apply_adam=False, last_rows=5)
    s.checks(s.p, 1, 5, 1, s.g, "last_rows=5")
    assert s.counters.tolist() == [1, 0]


def _engine(**kw):
    c = Case(64, 128, 320)
    eng = FusedMLPEngine(64, 128, 320, lr=CFG.lr, device=DEV, init_params=c.p.cpu(), stats_ring=8, **kw)
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
    assert torch.equal(eng.params, c.p) and torch.equal(eng.exp_avg_sq, c.v) and torch.equal(eng.stats, c.stats)
    assert eng.counters[:2].tolist() == [4, 0] and eng.health()["saturated"] == 0
    _, twin = _engine()
    twin.run(4)
    assert _same(eng, twin)                       # two runs from one state
    _, graph = _engine()
    assert graph.capture(1, remainders=False)     # one real warm-up step, then four replays
    graph.run(4)
    eng.run(1)
    torch.cuda.synchronize()
    assert graph._graph is not None and _same(eng, graph)


@pytest.mark.parametrize("kw", [dict(clip_norm=1.0), dict(accumulate=2), dict(optimizer="sgd"),
                                dict(dp_context=[1, 0, 0, 0, 0, 0, 0])], ids=lambda k: next(iter(k)))
def test_engine_refuses_what_stops_at_256_rows(kw):
    with pytest.raises(ValueError, match="256"):
        FusedMLPEngine(64, 128, 320, device=DEV, **kw)


def test_trainer_fits_batch_512_on_the_fused_step(tmpdir):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep, MNISTClassifier

    pl.seed_everything(0)
    model = MNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": 512})
    tr = pl.Trainer(default_root_dir=str(tmpdir), gpus=1, max_epochs=1, limit_train_batches=4,
                    checkpoint_callback=False, progress_bar_refresh_rate=0, num_sanity_val_steps=0)
    assert tr.fit(model) == 1
    assert isinstance(tr._fused, FusedMNISTStep) and tr._fused.eng is not None and tr._fused.eng.wide
    assert tr._fused.eng.global_step == 4 and tr.global_step == 4
    assert torch.isfinite(tr.callback_metrics["loss"]).all()
