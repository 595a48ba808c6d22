"""The one-workgroup MNIST step (csrc/mlp_kernels.hip ``mlp_train_kernel``, B <= 256, the path of
``FusedMNISTStep.train_batch`` and ``FusedMLPEngine._reference_step``) against float64, stage by
stage and row by row, through ``fused_mlp.mlp_train_step``.  The kernel keeps every activation in
LDS and exports six gradients and a stats row, so the stages are observed from outside through
the gate of tests/mlp_reference.py: a row with pixel 0 = 1 and label c0 is silent (dZ exactly 0),
and with all rows but one silent the gradients ARE that row's dZ, dH2, dH1 and rank-1 products
whose exact quotients give back its X, H1 and H2.  tests/test_mlp_probe_reference.py shows on the
CPU that the committed cases meet the method's preconditions and that the checks are sharp.

  probe          every row r of the batch speaks in turn (gate off, a genuine softmax):
                 EQUAL   db == one row, each dW == the outer product of the recovered factors
                         (tile placement; whatever a silent or padded row could touch is 0), every
                         factor a bf16 number, X == bf16(input); dyadic family: H1, H2 under
                         ``exact_certificate``; the counts of the stats row
                 BOUNDED H1 (``ref_h2``'s form, K = 784: layer 1 is a plain fp32 sum in any split),
                         H2, dZ (1 / B), dH2, dH1, the loss (NLL / B; 2 U24 for 1 / B and the
                         product): U8, U24, the MFMA factor 2 and SOFT, none read off the kernel
  exact batch    all rows gate-on, labels over the 10 classes, dyadic operands: every stage
                 predicted in float64 with bf16 roundings; prob[c0] is exactly 1.0f (logit gap
                 >= 128, asserted), so dZ is +-bf16(1 / B) or 0.  H1, H2, dH2, dH1 must be certified
                 (asserted); a gradient whose batch sum is certified, chunk adds included, is
                 EQUAL (``exact_grads``, asserted), the others take ``grad_checks``' bound
  superposition  all rows gate-off: the gradient within 2 Bp U24 sum_r |G_r| of the float64 sum
                 of the probe runs' G_r (Bp = chunks x chunk rows), the loss within ``ref_stats``'
                 bound + (Bp + 2) U24 loss of the rows' mean float64 NLL.  A row's values are the
                 same in both runs because rows are independent -- except for the order of layer
                 1's four atomic partial sums at L1 = 32, so there this test runs on dyadic operands
                 only (every order exact); from L1 = 64 on two partials add commutatively
  epilogues      accumulate_grad bitwise (one chunk, or silent chunks around one row); fused Adam
                 over several chunks with beta1 = 0 and a zeroed
                 exp_avg (m' is the applied gradient bit for bit) against ``ref_adam``; counters,
                 ``advance_step=False`` and the stats ring
  repeatability  two runs bitwise equal where the arithmetic is order-free (L1 >= 64, or dyadic)

Families: ``f32`` random weights and ``torch.rand`` pixels through ``x_f32=`` (the Trainer's path),
``norm`` dyadic ``exact_params`` / ``exact_data`` under NORM_PM1 in u8 mode (the NORM instance),
``u8`` random bytes under the default map.  32x64 and 32x32 take 64-row chunks above 32 rows,
every other width 32-row chunks; L1 = 32 / 64 / 128 split layer 1 over 4 / 2 / 1 waves; B = 33 and
65 leave a last chunk of one row; 256 runs 4 or 8 chunks.  A probe launch and its checks take
about a millisecond, so the full width x batch product runs (under half a second per case).
Worst error / bound per case: profiles/r25_one_workgroup_step/test_ratios.log."""
import functools
from types import SimpleNamespace

import pytest
import torch

import mlp_reference as R
import optim_reference as OR
from ray_lightning_accelerators_amd.ops import fused_mlp

gpu = pytest.mark.gpu
DEV = torch.device("cuda", 0)
C0 = 3
WIDTHS = ((32, 64), (32, 32), (64, 128), (128, 256), (128, 64))
BATCHES = (1, 32, 33, 64, 65, 100, 256)
SHAPES = [(L1, L2, B) for L1, L2 in WIDTHS for B in BATCHES]   # the full product: 551 probe launches per width
PROBE_CASES = [(L1, L2, B, fam) for fam in ("f32", "norm") for L1, L2, B in SHAPES] + [(32, 64, 65, "u8")]
EXACT_CASES = SHAPES
SUPER_CASES = [(L1, L2, B, "norm" if L1 == 32 else "f32") for L1, L2, B in SHAPES if B in (33, 65, 100, 256)] \
    + [(64, 128, 100, "norm")]
# (L1, L2, B, family): batches of several chunks, a ragged last one among them
ADAM_CASES = [(64, 128, 100, "u8"), (128, 256, 65, "f32"), (32, 64, 100, "norm"), (32, 64, 256, "f32")]
ADAM_CFGS = [OR.adam_cfg("adam", lr=1e-2, betas=(0.0, 0.999)),
             OR.adam_cfg("adamw_wd", lr=1e-2, betas=(0.0, 0.999), wd=0.05, adamw=True),
             OR.adam_cfg("lr_tensor", lr=3e-3, betas=(0.0, 0.999))]


def exact_grads(B):
    """The gradients whose batch sum the certificate proves exact in the exact-batch family (worked
    out by tests/test_mlp_probe_reference.py on the CPU; asserted there and here, as an equality of
    sets): with 1 / B a power of two all six (at 256 rows dW3's sum of H2 up to 64 is past it); else
    bf16(1 / B) spreads the granularity and db2, db3 remain."""
    if B & (B - 1):
        return {"db2", "db3"}
    return {"d" + k for k in R.NAMES} - ({"dW3"} if B == 256 else set())


def committed_cases():
    return sorted(set(PROBE_CASES) | {c[:3] + ("norm",) for c in EXACT_CASES} | set(SUPER_CASES) | set(ADAM_CASES))


def make_case(L1, L2, B, family):
    """The operands of one case on the CPU: gated parameters, ``gate_rows``' pair (rows 0..B-1 gate
    off with their labels, B..2B-1 silenced), the staged bf16 pixels X2 and the weights as the
    kernel reads them."""
    seed = 2500 + 7 * L1 + 3 * L2 + B
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(L1=L1, L2=L2, B=B, family=family, c0=C0, exact=family == "norm", affine=None,
                        BC=R.chunk_rows_1wg(L1, L2, B))
    if family == "f32":
        params, x = R.random_params(L1, L2, seed), torch.rand(B, 784, generator=g)
        y = torch.randint(0, 10, (B,), generator=g)
        c.x2, c.y2 = R.gate_rows(x, y, C0, 1.0, 0.0)
        c.X2 = c.x2.to(torch.bfloat16).double()
    else:
        params = R.exact_params(L1, L2, seed) if c.exact else R.random_params(L1, L2, seed)
        x, y = R.exact_data(B, seed) if c.exact else R.random_data(B, seed)
        c.affine = fused_mlp.input_affine(R.NORM_PM1 if c.exact else None)
        c.x2, c.y2 = R.gate_rows(x, y, C0, 255, 0)
        c.X2 = fused_mlp.u8_to_input(c.x2, *c.affine).to(torch.bfloat16).double()
    c.params = R.gate_params(params, L1, L2, C0)
    c.wt = R.step_weights(c.params, L1, L2)
    c.Bp = (B + c.BC - 1) // c.BC * c.BC
    return c


class Dev:
    """One case's state on the GPU; ``step(order)`` runs the rows ``order`` of the pair."""

    def __init__(self, c, ring=1):
        self.c = c
        self.p = c.params.to(DEV)
        self.g, self.m, self.v = (torch.zeros_like(self.p) for _ in range(3))
        self.stats = torch.zeros(ring, 4, device=DEV)
        self.counters = torch.zeros(2, dtype=torch.int64, device=DEV)
        self.x2, self.y2 = c.x2.to(DEV), c.y2.to(DEV)

    def step(self, order, **kw):
        c, o = self.c, order.to(DEV)
        if c.family == "f32":
            data = dict(x_f32=self.x2.index_select(0, o).contiguous(), labels=self.y2.index_select(0, o).contiguous())
        else:
            data = dict(x_u8=self.x2, labels=self.y2, order=o, n_batches=1, x_scale=c.affine[0], x_shift=c.affine[1])
        fused_mlp.mlp_train_step(self.p, self.g, L1=c.L1, L2=c.L2, B=c.B, counters=self.counters, exp_avg=self.m,
                                 exp_avg_sq=self.v, stats=self.stats, **data, **kw)
        return self.g


@functools.lru_cache(maxsize=None)
def sweep(L1, L2, B, family):
    """The B probe runs of one case, shared by the probe and the superposition test."""
    c = make_case(L1, L2, B, family)
    d = Dev(c)
    rows, stats, gsum, gabs, bad = R.probe_sweep(lambda order, t: (d.step(order), d.stats[0]), B, L1, L2)
    assert not bad, bad[:4]
    assert d.counters.tolist() == [B, 0]
    return c, rows, stats, gsum, gabs


def _tag(kind, c):
    return f"{kind} {c.L1}/{c.L2} B={c.B} {c.family} chunk={c.BC} split={R.nsplit_1wg(c.L1)}"


@gpu
@pytest.mark.parametrize("L1,L2,B,family", PROBE_CASES)
def test_every_row_speaks_in_turn(L1, L2, B, family):
    c, rows, stats, _, _ = sweep(L1, L2, B, family)
    res = R.probe_checks(rows, c.wt, c.X2[:B], c.y2[:B], B, exact=c.exact, stats=stats, steps=torch.arange(1, B + 1))
    bad = R.report(_tag("probe", c), res)
    assert not bad, bad


@gpu
@pytest.mark.parametrize("L1,L2,B", EXACT_CASES)
def test_exact_batch_of_gate_on_rows(L1, L2, B):
    c = make_case(L1, L2, B, "norm")
    d = Dev(c)
    y = c.y2[:B]
    d.y2 = torch.cat([y, y]).to(DEV)                  # the gate-on rows with their own labels
    assert R.gate_gap(c.X2[B:], c.wt, C0) >= R.GAP_MIN
    obs, cert = R.exact_batch(c.X2[B:], y, c.wt, B, C0)
    assert all(cert[k] for k in ("H1", "H2", "dH2", "dH1")), cert
    assert {"d" + k for k in R.NAMES if cert["d" + k]} == exact_grads(B), cert
    g = d.step(R.probe_order(B))
    res = R.exact_batch_checks(g, obs, cert, L1, L2, c.Bp)
    Z, ez = R.ref_logits(obs["h2"], c.wt.W3, c.wt.b3)
    if R.exact_certificate(obs["h2"], c.wt.W3, c.wt.b3).ok:
        ez = torch.zeros_like(ez)
    st, got = R.ref_stats(Z, ez, y), d.stats[0].cpu().double()
    res.append(("loss", R.cmp_bound(got[:1], torch.tensor([st.loss], dtype=torch.float64),
                                    st.loss_bound + (c.Bp + 2) * R.U24 * st.loss)))
    bad = R.report(_tag("exact", c), res)
    assert not bad, bad
    assert st.ambiguous == 0 and got[1:].tolist() == [int((y == C0).sum()), B, 1], (got, st)


@gpu
@pytest.mark.parametrize("L1,L2,B,family", SUPER_CASES)
def test_full_batch_is_the_sum_of_its_rows(L1, L2, B, family):
    c, rows, _, gsum, gabs = sweep(L1, L2, B, family)
    d = Dev(c)
    g = d.step(torch.arange(B))
    res = R.superposition_checks(g, gsum, gabs, c.Bp, L1, L2)
    y = c.y2[:B]
    Z, ez = R.ref_logits(rows["h2"], c.wt.W3, c.wt.b3)
    st, got = R.ref_stats(Z, ez, y), d.stats[0].cpu().double()
    res.append(("loss", R.cmp_bound(got[:1], torch.tensor([st.loss], dtype=torch.float64),
                                    st.loss_bound + (c.Bp + 2) * R.U24 * st.loss)))
    bad = R.report(_tag("super", c), res)
    assert not bad, bad
    assert st.certain <= got[1] <= st.certain + st.ambiguous and got[2:].tolist() == [B, 1], (got, st)


def _order_free(c):
    return c.L1 >= 64 or c.exact


# (L1, L2, B, family, speaking row): None = the whole genuine batch, in ONE chunk
ACCUMULATE_CASES = [(128, 256, 32, "f32", None), (64, 128, 100, "f32", 0), (64, 128, 100, "f32", 99),
                    (32, 64, 65, "norm", 3), (32, 64, 65, "norm", 64), (128, 256, 33, "u8", 32)]


@gpu
@pytest.mark.parametrize("L1,L2,B,family,r", ACCUMULATE_CASES)
def test_accumulate_onto_a_planted_gradient(L1, L2, B, family, r):
    """``accumulate_grad`` adds the planted gradient before the first chunk's, so over several
    genuine chunks ((plant + g0) + g1) is not (g0 + g1) + plant in fp32.  Bitwise equality is owed
    where one of the two adds is exact: a batch of one chunk, and a probe batch, whose silent
    chunks add exact zeros -- with the speaking row in the first chunk the plant is carried through
    every later chunk, with it in the last chunk through every earlier one."""
    c = make_case(L1, L2, B, family)
    order = torch.arange(B) if r is None else R.probe_order(B, r)
    assert _order_free(c) and (r is not None or c.Bp == c.BC)
    a, b = Dev(c), Dev(c)
    plant = torch.randn(a.g.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    a.step(order)
    b.g.copy_(plant)
    b.step(order, accumulate_grad=True)
    assert float(a.g.abs().sum()) > 0.0 and torch.equal(b.g, a.g + plant)


@gpu
@pytest.mark.parametrize("L1,L2,B,family", ADAM_CASES)
def test_three_fused_adam_steps_over_several_chunks(L1, L2, B, family):
    c = make_case(L1, L2, B, family)
    assert c.Bp // c.BC >= 2
    d, twin = Dev(c), Dev(c)
    lr_t = torch.tensor([ADAM_CFGS[2].lr], device=DEV)
    for t, cfg in enumerate(ADAM_CFGS, 1):
        d.m.zero_()
        before = {"p": d.p.clone(), "v": d.v.clone()}
        twin.p.copy_(d.p)
        twin.step(torch.arange(B))
        kw = dict(lr_tensor=lr_t) if cfg.name == "lr_tensor" else dict(lr=cfg.lr)
        d.step(torch.arange(B), apply_adam=True, betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.wd, adamw=cfg.adamw,
               **kw)
        # bitwise the gradient of the same step without Adam wherever the arithmetic is order-free
        applied = twin.g if (c.L1 >= 64 or (c.exact and t == 1)) else None
        res = R.adam_checks(before, {"p": d.p, "m": d.m, "v": d.v}, applied, cfg, t)
        bad = R.report(_tag(f"adam t={t} {cfg.name}", c), res)
        assert not bad, bad
        assert d.counters.tolist() == [t, 0] and d.stats[0, 2:].tolist() == [B, t]


@gpu
def test_counters_advance_step_and_the_stats_ring():
    c = make_case(32, 64, 33, "u8")
    d = Dev(c, ring=4)
    order = torch.cat([R.probe_order(33, r) for r in (0, 1, 2)]).to(DEV)
    d.counters.copy_(torch.tensor([5, 1]))
    kw = dict(L1=32, L2=64, B=33, counters=d.counters, stats=d.stats, x_u8=d.x2, labels=d.y2, order=order, n_batches=3)
    fused_mlp.mlp_train_step(d.p, d.g, advance_step=False, **kw)
    row1, _ = R.recover_row(d.g, 32, 64)
    assert d.counters.tolist() == [5, 2]                     # the cursor moves, the step does not
    assert d.stats[1, 2:].tolist() == [33, 6] and float(d.stats[[0, 2, 3]].abs().sum()) == 0.0   # slot (6 - 1) % 4
    fused_mlp.mlp_train_step(d.p, d.g, **kw)
    row2, _ = R.recover_row(d.g, 32, 64)
    assert d.counters.tolist() == [6, 0]                     # wraps at n_batches
    assert d.stats[1, 2:].tolist() == [33, 6]                # the same t again: the same slot
    # the cursor chose the batch: rows 1 and 2 spoke
    assert torch.equal(row1["x"], c.X2[1]) and torch.equal(row2["x"], c.X2[2])
    f = Dev(make_case(32, 64, 33, "f32"))
    f.counters.copy_(torch.tensor([9, 7]))
    f.step(torch.arange(33))
    assert f.counters.tolist() == [10, 7]                    # f32 mode leaves the cursor alone


@gpu
@pytest.mark.parametrize("L1,L2,B,family", [(64, 128, 100, "f32"), (128, 256, 256, "f32"), (32, 64, 100, "norm"),
                                            (32, 32, 65, "norm"), (128, 64, 33, "u8")])
def test_two_runs_agree_bitwise(L1, L2, B, family):
    c = make_case(L1, L2, B, family)
    assert _order_free(c)
    a, b = Dev(c), Dev(c)
    a.step(torch.arange(B))
    b.step(torch.arange(B))
    assert torch.equal(a.g, b.g) and torch.equal(a.stats[0, 1:], b.stats[0, 1:])
