"""tests/optim_reference.py checked on the CPU, before anything runs on a GPU: the float64
formulas agree with torch.optim stepping float64 tensors, both correct fp32 emulations of
every kernel (separate multiply / add, and contracted) pass the comparisons of
tests/test_optim_kernels.py on the inputs that file uses, and every deliberately wrong
variant fails on the input set named next to it."""
import math

import pytest
import torch

import optim_reference as R

D = 2.0 ** -53


def _close64(a, b, mag):
    """A few float64 roundings of the addends' magnitudes."""
    return bool(((a - b).abs() <= 64 * D * (mag + a.abs())).all())


# ------------------------------------------------------------------ float64 formulas vs torch.optim
@pytest.mark.parametrize("cfg", R.ADAM_CONFIGS, ids=lambda c: c.name)
def test_ref_adam_is_torch_optim_in_float64(cfg):
    st = R.make_state(257, 11, cfg.state)
    ref = R.ref_adam(st, cfg, exact_scalars=True, clamp=False)
    q = st["p"].double().requires_grad_(True)
    q.grad = st["g"].double() * R.f32(cfg.grad_scale)       # exact: 24 x 24 bits
    cls = torch.optim.AdamW if cfg.adamw else torch.optim.Adam
    opt = cls([q], lr=R.f32(cfg.lr), betas=(R.f32(cfg.betas[0]), R.f32(cfg.betas[1])), eps=R.f32(cfg.eps),
              weight_decay=R.f32(cfg.wd), maximize=cfg.maximize, foreach=False)
    m, v = st["m"].double(), st["v"].double()
    opt.state[q] = {"step": torch.tensor(float(cfg.t - 1)), "exp_avg": m, "exp_avg_sq": v}
    opt.step()
    assert float(opt.state[q]["step"]) == cfg.t
    assert _close64(ref["p"], q.detach(), ref["mag_p"])
    assert _close64(ref["m"], m, st["m"].double().abs() + st["g"].double().abs())
    assert _close64(ref["v"], v, ref["v"])


@pytest.mark.parametrize("cfg", R.SGD_CONFIGS, ids=lambda c: c.name)
def test_ref_sgd_is_torch_optim_in_float64(cfg):
    st = R.make_state(257, 12, cfg.state)
    ref = R.ref_sgd(st, cfg, exact_scalars=True, clamp=False)
    q = st["p"].double().requires_grad_(True)
    q.grad = st["g"].double() * R.f32(cfg.grad_scale)
    opt = torch.optim.SGD([q], lr=R.f32(cfg.lr), momentum=R.f32(cfg.momentum), dampening=R.f32(cfg.dampening),
                          weight_decay=R.f32(cfg.wd), nesterov=cfg.nesterov, maximize=cfg.maximize, foreach=False)
    if cfg.momentum != 0 and cfg.t > 1:
        opt.state[q] = {"momentum_buffer": st["buf"].double()}
    opt.step()
    assert _close64(ref["p"], q.detach(), ref["mag_p"])
    if cfg.momentum != 0:
        buf = opt.state[q]["momentum_buffer"]
        assert _close64(ref["buf"], buf, st["buf"].double().abs() + st["g"].double().abs() + st["p"].double().abs())
        if cfg.t == 1:   # overwritten, not blended with the stale buffer
            assert not _close64(ref["buf"], R.ref_sgd(st, cfg, t=2, exact_scalars=True)["buf"], ref["buf"].abs())
    else:
        assert ref["buf"] is None


def test_fp32_scalars_follow_the_kernel():
    """step_size and sqrt(bc2) are rounded to fp32 from double bias corrections; 1 - beta is exact
    in fp32 for beta >= 0.5 (Sterbenz), which every configuration satisfies."""
    ss, bs = R.adam_scalars(R.f32(3e-3), R.f32(0.9), R.f32(0.999), 7)
    assert ss == R.f32(ss) and bs == R.f32(bs)
    ssx, bsx = R.adam_scalars(R.f32(3e-3), R.f32(0.9), R.f32(0.999), 7, exact=True)
    assert ss != ssx and abs(ss - ssx) <= R.U * ssx and abs(bs - bsx) <= R.U * bsx
    for cfg in R.ADAM_CONFIGS:
        for b in cfg.betas:
            assert b >= 0.5 and R.f32(1.0 - R.f32(b)) == 1.0 - R.f32(b)


# ------------------------------------------------------------------ correct emulations pass
def _adam_check(cfg, n, fused, wrong=None, seed=21):
    st = R.make_state(n, seed, cfg.state)
    out = R.emu_adam(st, cfg, fused, wrong=wrong)
    return R.check_adam(out, R.ref_adam(st, cfg), out["shadow"])


def _sgd_check(cfg, n, fused, wrong=None, seed=22):
    st = R.make_state(n, seed, cfg.state)
    out = R.emu_sgd(st, cfg, fused, wrong=wrong)
    return R.check_sgd(out, R.ref_sgd(st, cfg), out["shadow"])


def _mlp_check(L1, L2, fused, wrong=None):
    st = R.make_state(R.mlp_param_count(L1, L2), 23 + L1 + L2)
    out = R.emu_mlp_adam(st, R.MLP_CFG, L1, L2, fused, wrong=wrong)
    return R.check_mlp_adam(out, R.ref_mlp_adam(st, R.MLP_CFG, L1, L2), L1, L2)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", R.ADAM_CASES, ids=lambda c: f"{c[0].name}-{c[1]}")
def test_correct_adam_emulations_pass(case, fused):
    c = _adam_check(*case, fused)
    assert c.ok, c.detail


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", R.SGD_CASES, ids=lambda c: f"{c[0].name}-{c[1]}")
def test_correct_sgd_emulations_pass(case, fused):
    c = _sgd_check(*case, fused)
    assert c.ok, c.detail


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("L", R.MLP_WIDTHS)
def test_correct_mlp_adam_emulations_pass(L, fused):
    c = _mlp_check(*L, fused)
    assert c.ok, c.detail


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_special_values_keep_their_class_in_both_emulations(kind):
    """The reference evaluated in fp32's range predicts the class of every output; the ordinary
    neighbours of the special gradients stay within their bound."""
    st = R.make_special()
    for cfg in (R.ADAM_CONFIGS[1],) if kind == "adam" else (R.SGD_CONFIGS[1], R.SGD_CONFIGS[2]):
        ref = (R.ref_adam if kind == "adam" else R.ref_sgd)(st, cfg)
        for fused in (False, True):
            out = (R.emu_adam if kind == "adam" else R.emu_sgd)(st, cfg, fused)
            c = R.check_special(out, ref, kind, out["shadow"])
            assert c.ok, c.detail
    if kind == "adam":
        assert torch.isnan(ref["p"][1]) and torch.isnan(ref["p"][3])       # NaN stays NaN; inf / inf
        assert ref["v"][4] == math.inf and torch.isfinite(ref["m"][4])     # (1e20)^2 overflows, m does not
        assert ref["p"][4] == st["p"][4].double()                          # ... so the update is zero
        assert torch.isfinite(ref["p"][[0, 2, 5, 6, 7]]).all()
    else:
        assert torch.isnan(ref["p"][1]) and ref["p"][3] == -math.inf and torch.isfinite(ref["p"][4])


# ------------------------------------------------------------------ wrong variants fail
# (kernel, wrong variant, configuration name, n): the input set of tests/test_optim_kernels.py
# on which the comparison rejects the variant
ADAM_MUTANTS = [
    ("t_minus_1", "t2", 1025),            # bc1 = 1 - 0.9 instead of 1 - 0.81
    ("eps_in_sqrt", "small_eps", 1025),   # sqrt(v) ~ eps: sqrt(v + eps) is ~1e-4 against ~1e-6
    ("scale_after_wd", "gs8_wd", 1025),   # the decay term shrinks by 8 too
    ("adamw_step_size", "adamw_wd", 1025),  # decay by lr / bc1, twice lr at t = 7
    ("no_maximize", "maximize", 1025),
    ("tail", "adam_wd", 1023),
    ("tail", "adam_wd", 1),
    ("second_pass", "adam_wd", R.BIG_N),
    ("truncate", "adam_wd", 1025),
    ("stale_shadow", "adam_wd", 1025),
]
SGD_MUTANTS = [
    ("first_t0", "t1", 1025),             # blends the stale buffer at t = 1
    ("dampen_first", "t1", 1025),
    ("nesterov_swapped", "nesterov", 1025),
    ("nesterov_swapped", "mom", 1025),
    ("wd_after_momentum", "wd", 1025),    # p agrees, the momentum buffer lacks wd * p
    ("tail", "wd", 1023),
    ("tail", "wd", 2),
    ("second_pass", "wd", R.BIG_N),
    ("truncate", "wd", 1025),
    ("stale_shadow", "wd", 1025),
]


def _cfg(cfgs, name):
    return next(c for c in cfgs if c.name == name)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("wrong,name,n", ADAM_MUTANTS)
def test_wrong_adam_variants_fail(wrong, name, n, fused):
    cfg = _cfg(R.ADAM_CONFIGS, name)
    assert (cfg, n) in R.ADAM_CASES
    assert _adam_check(cfg, n, fused).ok
    assert not _adam_check(cfg, n, fused, wrong).ok


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("wrong,name,n", SGD_MUTANTS)
def test_wrong_sgd_variants_fail(wrong, name, n, fused):
    cfg = _cfg(R.SGD_CONFIGS, name)
    assert (cfg, n) in R.SGD_CASES
    assert _sgd_check(cfg, n, fused).ok
    assert not _sgd_check(cfg, n, fused, wrong).ok


@pytest.mark.parametrize("wrong", ["w2_untransposed", "w3_pad", "truncate", "stale_shadow"])
def test_wrong_mlp_adam_layouts_fail(wrong):
    L1, L2 = R.MLP_WIDTHS[0]
    assert not _mlp_check(L1, L2, True, wrong).ok


def test_mlp_layout_is_the_package_layout():
    from ray_lightning_accelerators_amd.ops import fused_mlp

    for L1, L2 in sorted(fused_mlp.SUPPORTED):
        assert R.mlp_shadow_layout(L1, L2) == fused_mlp.mlp_shadow_layout(L1, L2)
    assert set(R.MLP_WIDTHS) <= fused_mlp.SUPPORTED
    assert min(fused_mlp.SUPPORTED) in R.MLP_WIDTHS and max(fused_mlp.SUPPORTED) in R.MLP_WIDTHS
    L1, L2 = 32, 64
    p = torch.arange(R.mlp_param_count(L1, L2), dtype=torch.float32)
    sh = torch.empty(fused_mlp.mlp_shadow_layout(L1, L2)["total"])
    fused_mlp.mlp_refresh_shadow(p, sh, L1, L2)        # the package's CPU path
    lay = R.mlp_shadow_layout(L1, L2)
    a, b, c = R.mlp_shadows(p, L1, L2)
    assert torch.equal(sh[:lay["np"]], a) and torch.equal(sh[lay["w2t"]:lay["w3t"]], b)
    assert torch.equal(sh[lay["w3t"]:], c)


# ------------------------------------------------------------------ sumsq / scale_
@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_sumsq_emulations(n):
    x = R.make_vector(n, 31)
    ref, bound = R.ref_sumsq(x)
    for fused in (False, True):
        assert abs(float(R.emu_sumsq(x, fused)) - ref) <= bound
    for pos in R.one_hot_positions(n):
        assert float(R.emu_sumsq(R.one_hot(n, pos))) == 1.0


def test_wrong_sumsq_variants_fail():
    # the tail dropped: random data at n = 3 (all tail) and 100,003, and the one-hot tail positions
    for n in (3, 100003):
        x = R.make_vector(n, 31)
        ref, bound = R.ref_sumsq(x)
        assert abs(float(R.emu_sumsq(x, wrong="tail")) - ref) > bound
        assert float(R.emu_sumsq(R.one_hot(n, n - 1), wrong="tail")) == 0.0
    # a block's partial dropped: random data at 1024 (one block), 100,003 and BIG_N, one-hot in the last block
    for n in (1024, 100003, R.BIG_N):
        x = R.make_vector(n, 31)
        ref, bound = R.ref_sumsq(x)
        assert abs(float(R.emu_sumsq(x, wrong="block")) - ref) > bound
    n = 100003
    assert float(R.emu_sumsq(R.one_hot(n, 4 * (n >> 2) - 1), wrong="block")) == 0.0


def test_sumsq_bound_counts_the_kernel_structure():
    assert R.sumsq_k(1) == 4 + 0 + 1 + 6 + 4 + 1
    assert R.sumsq_k(100003) == 4 + 1 + 1 + 6 + 4 + 98
    assert R.sumsq_k(R.BIG_N) == 4 + 2 + 1 + 6 + 4 + 2048
    assert R.opt_grid(R.GRID_SPAN) == 2048 and R.opt_grid(R.BIG_N) == 2048


def test_ref_scale_is_one_rounding():
    x = R.make_vector(1027, 32)
    for s in (0.125, 1.0 / 3.0, 1.0 / 8.0, 0.1):
        assert torch.equal(R.ref_scale(x, s), x * torch.tensor(s, dtype=torch.float32))


# ------------------------------------------------------------------ multi_copy
def _copy_check(sdt, ddt, scale, accumulate, fused, wrong=None):
    cs = []
    for s, so, d, do in R.make_copy_pairs(sdt, ddt, 41):
        src, dst = s[so:], d[do:]
        out = R.emu_multi_copy(src, dst, scale, accumulate, fused, wrong)
        cs.append(R.check_multi_copy(out, src, dst, scale, accumulate))
    return all(c.ok for c in cs), "; ".join(c.detail for c in cs)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("scale", [0.25, 1.0 / 3.0])
@pytest.mark.parametrize("sdt,ddt", R.COPY_DTYPE_PAIRS)
def test_correct_multi_copy_emulations_pass(sdt, ddt, scale, accumulate, fused):
    ok, detail = _copy_check(sdt, ddt, scale, accumulate, fused)
    assert ok, detail


def test_wrong_multi_copy_variants_fail():
    for fused in (False, True):
        # a bf16 destination's old value read as fp32 bits: every bf16-destination accumulate set
        for sdt in ("f32", "bf16"):
            for scale in (0.25, 1.0 / 3.0):
                assert not _copy_check(sdt, "bf16", scale, True, fused, "acc_bits")[0]
        # the scale applied after the cast: fp32 -> bf16 at scale 1/3 (two bf16 roundings: far more
        # than SHARE of the outputs land on another bf16) ...
        assert not _copy_check("f32", "bf16", 1.0 / 3.0, False, fused, "scale_after_cast")[0]
        assert not _copy_check("f32", "bf16", 1.0 / 3.0, True, fused, "scale_after_cast")[0]
        # ... and cannot be told apart at scale 0.25 without accumulation (a power of two commutes
        # with rounding) or from a bf16 source (the cast changes nothing): those results are the same bits
        assert _copy_check("f32", "bf16", 0.25, False, fused, "scale_after_cast")[0]
        assert _copy_check("bf16", "bf16", 1.0 / 3.0, False, fused, "scale_after_cast")[0]
