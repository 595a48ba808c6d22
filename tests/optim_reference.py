"""float64 single-step references of the flat-arena kernels in csrc/optim_kernels.hip
(adam_step, sgd_step, multi_copy, scale_, sumsq) and of csrc/mlp_adam.hip, the bounds
their fp32 results are held to, the input makers, and fp32 emulations of each kernel
(two correct forms and deliberately wrong variants) that tests/test_optim_reference.py
uses to show that the comparisons of tests/test_optim_kernels.py are sharp.

Every ``ref_*`` takes the state BEFORE the call and computes one step on the CPU, so a
multi-step test restarts the reference from the fp32 state the kernel was handed and a
bound never has to cover more than one step's roundings.  Hyperparameters enter at their
fp32 values, as the kernel receives them.

Bounds.  Each is (number of fp32 roundings + 1) x U x (sum of the magnitudes of the
stage's addends), plus the error carried in from the stage before; the count is written
where it is used.  The "+ 1" covers the second-order terms.  Device code is built with -O3
and the default -ffp-contract (ray_lightning_accelerators_amd/_build.py passes no
floating-point flag), so ``a + b * c`` may or may not become one fma: the fused form has
one rounding fewer, and the counts below are the unfused ones, which cover both.  hipcc
rounds ``sqrtf`` and ``/`` correctly by default (-fhip-fp32-correctly-rounded-divide-sqrt;
_build.py neither switches it off nor passes -ffast-math), so each counts as one
rounding.  Nothing here reads a kernel's output to decide a tolerance."""
import math
from collections import namedtuple

import torch

from bn_reference import SHARE, U, Cmp, cmp_bf16, cmp_bound, cmp_exact, round_bf16, same_bf16, to_bf16  # noqa: F401

TINY = 2.0 ** -140          # a few roundings of results below the normal range (spacing 2^-149)
OPT_THREADS = 256
OPT_MAX_BLOCKS = 2048
GRID_SPAN = OPT_MAX_BLOCKS * OPT_THREADS * 4   # elements one pass of the capped grid covers: 2048 x 1024 = 2,097,152
BIG_N = GRID_SPAN + 4 * OPT_THREADS * 3 + 3    # a second pass for the threads of three blocks, and a 3-element tail
CHUNK = 16384               # ops.optim.CHUNK_ELEMS
FLT_MAX = 3.4028234663852886e38
IN_FEATURES, NUM_CLASSES = 784, 10


def f32(x: float) -> float:
    """The fp32 value a kernel argument takes, as a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def opt_grid(n: int) -> int:
    return min(max(((n >> 2) + OPT_THREADS - 1) // OPT_THREADS, 1), OPT_MAX_BLOCKS)


def fp32_range(x: torch.Tensor) -> torch.Tensor:
    """float64 values as an fp32 evaluation classes them: beyond the largest fp32 -> inf."""
    return torch.where(x.abs() > FLT_MAX, torch.copysign(torch.full_like(x, math.inf), x), x)


# ------------------------------------------------------------------ configurations
AdamCfg = namedtuple("AdamCfg", "name lr betas eps wd grad_scale adamw maximize t state")
SGDCfg = namedtuple("SGDCfg", "name lr momentum dampening wd grad_scale nesterov maximize t state")


def adam_cfg(name, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, grad_scale=1.0, adamw=False, maximize=False, t=7,
             state="mid"):
    return AdamCfg(name, lr, betas, eps, wd, grad_scale, adamw, maximize, t, state)


def sgd_cfg(name, lr=0.05, momentum=0.0, dampening=0.0, wd=0.0, grad_scale=1.0, nesterov=False, maximize=False, t=5,
            state="mid"):
    return SGDCfg(name, lr, momentum, dampening, wd, grad_scale, nesterov, maximize, t, state)


# each switch at least once; no full product
ADAM_CONFIGS = [
    adam_cfg("adam"),
    adam_cfg("adam_wd", wd=0.01),
    adam_cfg("adamw_wd0", adamw=True),
    adam_cfg("adamw_wd", adamw=True, wd=0.05),
    adam_cfg("gs8_wd", wd=0.1, grad_scale=0.125),
    adam_cfg("maximize", maximize=True, wd=0.01),
    adam_cfg("small_eps", eps=1e-8, state="small"),
    adam_cfg("small_eps_big", eps=1e-3, state="small"),
    adam_cfg("betas", betas=(0.8, 0.95), eps=1e-6),
    adam_cfg("t1", t=1, wd=0.01),
    adam_cfg("t2", t=2),
    adam_cfg("t_large", t=100000),
]
SGD_CONFIGS = [
    sgd_cfg("plain_nobuf"),
    sgd_cfg("mom", momentum=0.9),
    sgd_cfg("nesterov", momentum=0.9, nesterov=True),
    sgd_cfg("dampening", momentum=0.9, dampening=0.1),
    sgd_cfg("wd", momentum=0.9, wd=1e-2),
    sgd_cfg("gs8_wd", momentum=0.9, wd=0.1, grad_scale=0.125),
    sgd_cfg("maximize", momentum=0.9, maximize=True, wd=1e-2),
    sgd_cfg("t1", momentum=0.9, dampening=0.1, t=1),
    sgd_cfg("t2", momentum=0.9, dampening=0.1, t=2),
]
SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 27882, BIG_N)
# (configuration, n): every size with one weight-decay configuration (1024 is one full block of
# float4s; 1, 2, 3 are tail only; BIG_N grid-strides), every configuration at 1025
ADAM_CASES = [(ADAM_CONFIGS[1], n) for n in SIZES] + [(c, 1025) for c in ADAM_CONFIGS if c is not ADAM_CONFIGS[1]]
SGD_CASES = [(SGD_CONFIGS[4], n) for n in SIZES] + [(c, 1025) for c in SGD_CONFIGS if c is not SGD_CONFIGS[4]] \
    + [(SGD_CONFIGS[0], 3)]
MLP_WIDTHS = [(32, 32), (64, 128), (128, 256)]   # smallest, one inside, largest of fused_mlp.SUPPORTED
MLP_CFG = adam_cfg("mlp", lr=1e-3, wd=0.01, grad_scale=0.5, t=7)
REDUCE_SIZES = (1, 3, 1024, 100003, BIG_N)


# ------------------------------------------------------------------ inputs
def _signs(n, g):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def make_state(n: int, seed: int, kind: str = "mid"):
    """Deterministic fp32 CPU state of one case: {p, g, m, v, buf}.

    "mid": a state in the middle of training -- m and buf nonzero, v >= 0, every sign
    present, |p| log-uniform on [1e-3, 10].  "small": |g| log-uniform on [1e-7, 1e-5] with
    m and sqrt(v) of the same order, so that sqrt(v) comes within a factor 10 of eps = 1e-8 and never exceeds 1e-5."""
    g = torch.Generator().manual_seed(1000003 * seed + n % 65521)
    p = _signs(n, g) * 10.0 ** (4 * torch.rand(n, generator=g) - 3)
    if kind == "small":
        gr = _signs(n, g) * 10.0 ** (2 * torch.rand(n, generator=g) - 7)
        m = _signs(n, g) * 10.0 ** (2 * torch.rand(n, generator=g) - 7)
        v = (10.0 ** (2 * torch.rand(n, generator=g) - 7)) ** 2
    else:
        gr = torch.randn(n, generator=g) * 10.0 ** (2 * torch.rand(n, generator=g) - 2)
        m = 0.1 * torch.randn(n, generator=g)
        v = (0.1 * torch.randn(n, generator=g)) ** 2 + 1e-6 * torch.rand(n, generator=g)
    buf = 0.5 * torch.randn(n, generator=g)
    return {"p": p.float(), "g": gr.float(), "m": m.float(), "v": v.float(), "buf": buf.float()}


SPECIAL_G = (0.3, math.nan, -0.2, math.inf, 1e20, 1e-40, -0.0, 0.7)   # n = 8: two float4s


def make_special(seed: int = 5):
    """n = 8 "mid" state whose gradient holds a NaN, +inf, 1e20 (g * g overflows), an fp32
    subnormal and -0.0 among ordinary values."""
    st = make_state(8, seed)
    st["g"] = torch.tensor(SPECIAL_G, dtype=torch.float32)
    return st


def one_hot(n: int, pos: int) -> torch.Tensor:
    x = torch.zeros(n)
    x[pos] = 1.0
    return x


def one_hot_positions(n: int):
    """First element, last element of the float4 body, every tail position, and (beyond
    one pass of the capped grid) an element only the second grid-stride pass reaches."""
    n4 = n >> 2
    pos = {0, n - 1}
    if n4:
        pos.add(4 * n4 - 1)
    pos.update(range(4 * n4, n))
    if n > GRID_SPAN:
        pos.add(GRID_SPAN + 5)
    return sorted(pos)


def make_vector(n: int, seed: int) -> torch.Tensor:
    """Sign-mixed fp32 data of one scale."""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + n % 65521))


# ------------------------------------------------------------------ float64 references
def _grad_stage(p, g, wd, grad_scale, maximize, l2, rng):
    """g' = (+-) g * grad_scale (+ wd * p) and its error bound."""
    gs = g * grad_scale
    Eg = 2 * U * gs.abs() if grad_scale != 1.0 else torch.zeros_like(gs)   # one product; k = 2 (exact for scale 1)
    if maximize:
        gs = -gs
    if l2 and wd != 0.0:
        w = wd * p
        # gs + wd * p: the product and the addition, k = 3, of |gs| + |wd p|; gs's own error passes through
        Eg = Eg + 3 * U * (gs.abs() + w.abs())
        gs = gs + w
    return rng(gs), Eg + TINY


def adam_scalars(lr, b1, b2, t, exact=False):
    """(step_size, sqrt(bc2)) as csrc adam_scalars computes them: bias corrections in double,
    both rounded to fp32 (``exact``: left in double, torch.optim's own values)."""
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    ss, bs = (lr / bc1 if bc1 else math.inf), math.sqrt(bc2)   # t = 0 only in a wrong variant
    return (ss, bs) if exact else (f32(ss), f32(bs))


def ref_adam(st, cfg, t=None, lr=None, exact_scalars=False, clamp=True):
    """One Adam / AdamW step in float64 from the fp32 state ``st`` (p, g, m, v); ``t`` is the
    step number after the update.  -> dict p, m, v (float64) and bp, bm, bv (bounds).
    ``exact_scalars``: hyperparameter-derived scalars left in double (for torch.optim)."""
    rng = fp32_range if clamp else (lambda x: x)
    t = cfg.t if t is None else t
    lr = f32(cfg.lr if lr is None else lr)
    b1, b2, eps, wd, gsc = f32(cfg.betas[0]), f32(cfg.betas[1]), f32(cfg.eps), f32(cfg.wd), f32(cfg.grad_scale)
    ss, bs = adam_scalars(lr, b1, b2, t, exact_scalars)
    p, g, m, v = (st[k].double() for k in ("p", "g", "m", "v"))
    gp, Eg = _grad_stage(p, g, wd, gsc, cfg.maximize, not cfg.adamw, rng)
    Ep = torch.zeros_like(p)
    if cfg.adamw and wd != 0.0:
        # p (1 - lr wd): lr wd, 1 - that (or both as one fma) and the product; k = 4 of |p| >= |p'|
        Ep = 4 * U * p.abs()
        p = p * (1.0 - lr * wd)
    # m + (1 - b1) (g' - m): 1 - b1, the difference, the product, the addition; k = 5 of |m| + (1 - b1)(|g'| + |m|)
    c1 = (1.0 - b1) if exact_scalars else f32(1.0 - b1)
    mn = rng(m + c1 * (gp - m))
    Em = c1 * Eg + 5 * U * (m.abs() + c1 * (gp.abs() + m.abs())) + TINY
    # v b2 + (1 - b2) g'^2: 1 - b2, the square, two products, the addition, all terms >= 0; k = 5 of v'
    c2 = (1.0 - b2) if exact_scalars else f32(1.0 - b2)
    vn = rng(v * b2 + c2 * rng(gp * gp))
    Ev = c2 * (2 * gp.abs() * Eg + Eg * Eg) + 5 * U * vn + TINY
    # sqrtf(v') / bs + eps: |sqrt a - sqrt b| <= min(sqrt|a - b|, |a - b| / sqrt b); then the root, the
    # quotient and the addition round once each; k = 4 of denom
    sq = torch.sqrt(vn)
    Es = torch.minimum(torch.sqrt(Ev), torch.where(sq > 0, Ev / sq, torch.full_like(sq, math.inf)))
    denom = sq / bs + eps
    Ed = Es / bs + 4 * U * denom
    # m' / denom: one rounding (k = 2), plus the operands' errors
    r = mn / denom
    Er = Em / denom + mn.abs() * Ed / (denom * (denom - Ed).clamp(min=1e-300)) + 2 * U * r.abs() + TINY
    # p + (-step_size) r: the product and the addition; k = 3 of |p| + |step_size r|
    pn = rng(p + (-ss) * r)
    Epn = Ep + ss * Er + 3 * U * (p.abs() + (ss * r).abs()) + TINY
    return {"p": pn, "m": mn, "v": vn, "bp": Epn, "bm": Em, "bv": Ev, "mag_p": p.abs() + (ss * r).abs()}


def ref_sgd(st, cfg, t=None, lr=None, exact_scalars=False, clamp=True):
    """One torch.optim.SGD step in float64 from (p, g, buf).  -> dict p, buf, bp, bb."""
    rng = fp32_range if clamp else (lambda x: x)
    t = cfg.t if t is None else t
    lr = f32(cfg.lr if lr is None else lr)
    mom, damp, wd, gsc = f32(cfg.momentum), f32(cfg.dampening), f32(cfg.wd), f32(cfg.grad_scale)
    p, g = st["p"].double(), st["g"].double()
    d, Ed = _grad_stage(p, g, wd, gsc, cfg.maximize, True, rng)
    buf = Eb = None
    if mom != 0.0:
        if t <= 1:
            buf, Eb = d, Ed                    # overwritten: a copy
        else:
            b0 = st["buf"].double()
            c = (1.0 - damp) if exact_scalars else f32(1.0 - damp)   # 1 - 0.1f rounds; no contraction changes it
            # buf mom + (1 - damp) g': 1 - damp, two products, the addition; k = 5 of both addends
            buf = rng(b0 * mom + c * d)
            Eb = c * Ed + 5 * U * ((b0 * mom).abs() + (c * d).abs()) + TINY
        if cfg.nesterov:
            # g' + mom buf': the product and the addition; k = 3
            Ed = Ed + mom * Eb + 3 * U * (d.abs() + (mom * buf).abs()) + TINY
            d = rng(d + mom * buf)
        else:
            d, Ed = buf, Eb
    # p + (-lr) d: the product and the addition; k = 3 of |p| + |lr d|
    pn = rng(p + (-lr) * d)
    Ep = lr * Ed + 3 * U * (p.abs() + (lr * d).abs()) + TINY
    return {"p": pn, "buf": buf, "bp": Ep, "bb": Eb, "mag_p": p.abs() + (lr * d).abs()}


def mlp_param_count(L1, L2):
    return L1 * IN_FEATURES + L1 + L2 * L1 + L2 + NUM_CLASSES * L2 + NUM_CLASSES


def mlp_shadow_layout(L1, L2):
    """The layout of ops.fused_mlp.mlp_shadow_layout, written out once more on purpose."""
    np_ = mlp_param_count(L1, L2)
    w2t = (np_ + 7) // 8 * 8
    w3t = w2t + L1 * L2
    return {"np": np_, "w2t": w2t, "w3t": w3t, "total": w3t + 16 * L2}


def mlp_shadows(p, L1, L2, untransposed=False, pad_value=0.0):
    """(row-major, W2^T [L1 * L2], W3^T padded to 16 classes [L2 * 16]) of a flat arena, in
    p's dtype.  ``untransposed`` / ``pad_value``: the wrong layouts."""
    o2 = L1 * IN_FEATURES + L1
    o3 = o2 + L2 * L1 + L2
    W2 = p[o2:o2 + L2 * L1].view(L2, L1)
    W3 = p[o3:o3 + NUM_CLASSES * L2].view(NUM_CLASSES, L2)
    w3t = torch.full((L2, 16), pad_value, dtype=p.dtype)
    w3t[:, :NUM_CLASSES] = W3.t()
    return p.clone(), (W2 if untransposed else W2.t()).reshape(-1).clone(), w3t.reshape(-1)


def ref_mlp_adam(st, cfg, L1, L2, t=None, lr=None):
    """ref_adam over the MNIST arena (the kernel has no maximize) plus the three shadow
    regions in float64, unrounded: "np", "w2t", "w3t" as laid out by mlp_shadow_layout."""
    assert not cfg.maximize and st["p"].numel() == mlp_param_count(L1, L2)
    r = ref_adam(st, cfg, t, lr)
    r["np"], r["w2t"], r["w3t"] = mlp_shadows(r["p"], L1, L2)
    r["mag_np"], r["mag_w2t"], r["mag_w3t"] = mlp_shadows(r["mag_p"], L1, L2)
    return r


K_SHADOW = 1   # cmp_bf16's k for a shadow: mag = (p's own bound) / U, so the fp32 error allowed is that bound


def ref_multi_copy(src, dst, scale, accumulate):
    """(value float64, sum of the addends' magnitudes) of dst (+)= src * scale."""
    v = src.double() * f32(scale)
    mag = v.abs()
    if accumulate:
        mag = mag + dst.double().abs()
        v = v + dst.double()
    return v, mag


K_COPY = 3        # src * scale and the accumulation round once each; k = 3


def sumsq_k(n: int) -> int:
    """fp32 roundings on the way of one x^2 into sumsq's result, from sumsq_kernel: the square and
    the three additions of its float4's term (4), ``acc +=`` once per grid-stride pass, once
    more for block 0's tail, six shuffle steps, four LDS partials, one atomic per block.  All
    terms are >= 0, so every partial sum is at most the total."""
    blocks = opt_grid(n)
    passes = -(-(n >> 2) // (blocks * OPT_THREADS))
    return 4 + passes + 1 + 6 + 4 + blocks


def ref_sumsq(x):
    """(sum x^2 float64, bound)."""
    s = float((x.double() ** 2).sum())
    return s, (sumsq_k(x.numel()) + 1) * U * s + TINY


def ref_scale(x, s):
    """x * fp32(s), exact in float64 (24 x 24 bits), rounded once: the bits scale_ must give."""
    return (x.double() * f32(s)).float()


# ------------------------------------------------------------------ fp32 emulation
class Arith:
    """fp32 arithmetic in one of the two correct forms: every operation rounded (separate
    multiply / add), or a * b + c computed in float64 and rounded once (contracted)."""

    def __init__(self, fused: bool):
        self.fused = fused

    @staticmethod
    def c(x):
        return torch.tensor(float(x), dtype=torch.float32)

    def mad(self, a, b, c):
        a, b, c = (x if torch.is_tensor(x) else self.c(x) for x in (a, b, c))
        if self.fused:
            return (a.double() * b.double() + c.double()).float()
        return a * b + c


def _bf(p32, truncate=False):
    return to_bf16(p32.double(), truncate)


def _untouched(out, st, n, tail, second_pass):
    """Layout mutants: the last n % 4 elements, or the float4s beyond one pass of the capped
    grid (the tail is block 0's and still done), left as they were."""
    spans = ([(n - n % 4, n)] if tail else []) + ([(GRID_SPAN, n - n % 4)] if second_pass and n > GRID_SPAN else [])
    for lo, hi in spans:
        for k in out:
            out[k][lo:hi] = st[k][lo:hi]


def emu_adam(st, cfg, fused=False, t=None, lr=None, wrong=None):
    """adam_elem in fp32 -> dict p, m, v, shadow (bf16).  ``wrong``: one of "t_minus_1",
    "eps_in_sqrt", "scale_after_wd", "adamw_step_size", "no_maximize", "tail", "second_pass",
    "truncate", "stale_shadow"."""
    A = Arith(fused)
    t = cfg.t if t is None else t
    lr = f32(cfg.lr if lr is None else lr)
    b1, b2, eps, wd, gsc = f32(cfg.betas[0]), f32(cfg.betas[1]), f32(cfg.eps), f32(cfg.wd), f32(cfg.grad_scale)
    ss, bs = adam_scalars(lr, b1, b2, t - 1 if wrong == "t_minus_1" else t)
    p, g, m, v = (st[k].float().clone() for k in ("p", "g", "m", "v"))
    p0 = p.clone()
    n = p.numel()
    c = A.c
    if wrong != "scale_after_wd":
        g = g * c(gsc)
    if cfg.maximize and wrong != "no_maximize":
        g = -g
    if wd != 0.0:
        if cfg.adamw:
            p = p * A.mad(c(-(ss if wrong == "adamw_step_size" else lr)), c(wd), c(1.0))
        else:
            g = A.mad(c(wd), p, g)
    if wrong == "scale_after_wd":
        g = g * c(gsc)
    mn = A.mad(c(1.0) - c(b1), g - m, m)
    vn = A.mad(c(1.0) - c(b2), g * g, v * c(b2))
    if wrong == "eps_in_sqrt":
        denom = torch.sqrt(vn + c(eps)) / c(bs)
    else:
        denom = torch.sqrt(vn) / c(bs) + c(eps)
    pn = A.mad(c(-ss), mn / denom, p)
    out = {"p": pn, "m": mn, "v": vn}
    _untouched(out, st, n, wrong == "tail", wrong == "second_pass")
    out["shadow"] = _bf(p0 if wrong == "stale_shadow" else out["p"], wrong == "truncate")
    return out


def emu_sgd(st, cfg, fused=False, t=None, lr=None, wrong=None):
    """sgd_elem in fp32 -> dict p, buf, shadow.  ``wrong``: "first_t0", "dampen_first",
    "nesterov_swapped", "wd_after_momentum", "tail", "second_pass", "truncate", "stale_shadow"."""
    A = Arith(fused)
    c = A.c
    t = cfg.t if t is None else t
    lr = f32(cfg.lr if lr is None else lr)
    mom, damp, wd, gsc = f32(cfg.momentum), f32(cfg.dampening), f32(cfg.wd), f32(cfg.grad_scale)
    p, g = st["p"].float().clone(), st["g"].float().clone()
    p0, n = p.clone(), p.numel()
    g = g * c(gsc)
    if cfg.maximize:
        g = -g
    if wd != 0.0 and wrong != "wd_after_momentum":
        g = A.mad(c(wd), p, g)
    buf = None
    if mom != 0.0:
        b0 = st["buf"].float().clone()
        first = (t <= 0) if wrong == "first_t0" else (t <= 1)
        if first:
            buf = (c(1.0) - c(damp)) * g if wrong == "dampen_first" else g.clone()
        else:
            buf = A.mad(c(1.0) - c(damp), g, b0 * c(mom))
        nest = cfg.nesterov != (wrong == "nesterov_swapped")
        g = A.mad(c(mom), buf, g) if nest else buf
    if wd != 0.0 and wrong == "wd_after_momentum":
        g = A.mad(c(wd), p, g)
    out = {"p": A.mad(c(-lr), g, p)}
    if buf is not None:
        out["buf"] = buf
    _untouched(out, st, n, wrong == "tail", wrong == "second_pass")
    out["shadow"] = _bf(p0 if wrong == "stale_shadow" else out["p"], wrong == "truncate")
    return out


def emu_mlp_adam(st, cfg, L1, L2, fused=True, t=None, lr=None, wrong=None):
    """mlp_adam_kernel(update = 1): adam1 (explicit fmas: the fused form is the kernel's own)
    and the shadow regions as bf16.  ``wrong``: emu_adam's, "w2_untransposed", "w3_pad"."""
    out = emu_adam(st, cfg, fused, t, lr, wrong if wrong in ("truncate", "stale_shadow") else None)
    src = st["p"].float() if wrong == "stale_shadow" else out["p"]
    np_, w2t, w3t = mlp_shadows(src, L1, L2, wrong == "w2_untransposed", 7.0 if wrong == "w3_pad" else 0.0)
    tr = wrong == "truncate"
    out["np"], out["w2t"], out["w3t"] = _bf(np_, tr), _bf(w2t, tr), _bf(w3t, tr)
    return out


def emu_sumsq(x, fused=False, wrong=None):
    """sumsq_kernel's structure in fp32: per-thread accumulators over the grid-stride passes,
    block 0's tail, the wave64 tree, the four LDS partials, the atomics (in block order).
    ``wrong``: "tail" (dropped), "block" (the last block's partial dropped)."""
    x = x.float()
    n = x.numel()
    n4 = n >> 2
    blocks = opt_grid(n)
    T = blocks * OPT_THREADS
    passes = -(-n4 // T)
    body = torch.zeros(max(passes, 1) * T, 4)
    body[:n4] = x[: 4 * n4].view(n4, 4)
    acc = torch.zeros(T)
    for j in range(passes):
        q = body[j * T:(j + 1) * T]
        if fused:
            term = (q.double() ** 2).sum(1).float()
        else:
            sq = q * q
            term = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
        acc = acc + term
    if wrong != "tail":
        tail = x[4 * n4:]
        acc[: tail.numel()] = acc[: tail.numel()] + tail * tail
    w = acc.view(-1, 64).clone()
    for off in (32, 16, 8, 4, 2, 1):
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
    part = w[:, 0].reshape(blocks, OPT_THREADS // 64)
    s = torch.zeros(blocks)
    for i in range(OPT_THREADS // 64):
        s = s + part[:, i]
    if wrong == "block":
        s = s[:-1]
    tot = torch.zeros(())
    for b in s:
        tot = tot + b
    return tot.reshape(1)


def emu_multi_copy(src, dst, scale, accumulate, fused=False, wrong=None):
    """One pair of multi_copy_kernel in fp32 -> the new dst.  ``wrong``: "acc_bits" (a bf16
    destination's old value read as fp32 bits), "scale_after_cast" (bf16 destination:
    src rounded to bf16 first, then scaled)."""
    A = Arith(fused)
    s = src.float()
    sc = A.c(f32(scale))
    if wrong == "scale_after_cast" and dst.dtype == torch.bfloat16:
        s = _bf(s).float()
    if accumulate:
        old = dst.float()
        if wrong == "acc_bits" and dst.dtype == torch.bfloat16:
            n = dst.numel()
            raw = torch.cat([dst, dst.new_zeros(n % 2 + 2)]).view(torch.float32)   # two bf16 per word
            old = raw[torch.arange(n) // 2]
            old = torch.where(torch.isfinite(old), old, torch.zeros_like(old))
        v = A.mad(s, sc, old)
    else:
        v = s * sc
    return _bf(v) if dst.dtype == torch.bfloat16 else v


# ------------------------------------------------------------------ checks
def classes(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    x = x.double()
    return torch.isnan(x) * 1 + (x == math.inf) * 2 + (x == -math.inf) * 3


def _join(names, cs) -> Cmp:
    return Cmp(all(c.ok for c in cs), max(c.ratio for c in cs), ", ".join(f"{n} {c.detail}" for n, c in zip(names, cs)))


def cmp_state(out, ref, pairs, skip=None) -> Cmp:
    """fp32 outputs by bound: ``pairs`` = (key, bound key) of ``ref``."""
    return _join([k for k, _ in pairs], [cmp_bound(out[k], ref[k], ref[b], skip) for k, b in pairs])


def check_adam(out, ref, shadow=None, skip=None) -> Cmp:
    """p, m, v by bound; the shadow bitwise RNE of the kernel's own p, and by cmp_bf16
    against the float64 p."""
    c = cmp_state(out, ref, (("p", "bp"), ("m", "bm"), ("v", "bv")), skip)
    return _with_shadow(c, out["p"], shadow, ref, skip)


def check_sgd(out, ref, shadow=None, skip=None) -> Cmp:
    pairs = (("p", "bp"),) + ((("buf", "bb"),) if ref["buf"] is not None else ())
    return _with_shadow(cmp_state(out, ref, pairs, skip), out["p"], shadow, ref, skip)


def _with_shadow(c, p_out, shadow, ref, skip):
    if shadow is None:
        return c
    e = cmp_exact(shadow, _bf(p_out))
    s = cmp_bf16(shadow, ref["p"], ref["bp"] / U, k=K_SHADOW, skip=skip)
    # the ratio reported is the fp32 state's: the shadow's is ~1 by construction (half a bf16 ulp)
    return Cmp(c.ok and e.ok and s.ok, max(c.ratio, e.ratio) if s.ok else math.inf,
               f"{c.detail}; shadow vs own p: {e.detail}; shadow vs fp64: {s.detail}")


def check_mlp_adam(out, ref, L1, L2) -> Cmp:
    """params, m, v by bound; each shadow region exactly RNE of the kernel's own params in
    the reference layout (so W2^T is transposed and the W3^T pad columns are zero) and by
    cmp_bf16 against the float64 params.  ``out``: p, m, v, np, w2t, w3t."""
    c = cmp_state(out, ref, (("p", "bp"), ("m", "bm"), ("v", "bv")))
    own = [_bf(r) for r in mlp_shadows(out["p"].float(), L1, L2)]
    bounds = mlp_shadows(ref["bp"], L1, L2)
    cs, names = [c], ["state"]
    for key, o, b in zip(("np", "w2t", "w3t"), own, bounds):
        cs.append(cmp_exact(out[key], o))
        cs.append(cmp_bf16(out[key], ref[key], b / U, k=K_SHADOW))
        names += [key + " vs own params", key + " vs fp64"]
    j = _join(names, cs)
    return Cmp(j.ok, c.ratio if j.ok else math.inf, j.detail)   # the fp32 state's ratio, as check_adam


def check_special(out, ref, kind, shadow=None) -> Cmp:
    """Special-value inputs: every output has the class (finite, NaN, +inf, -inf) of the
    reference evaluated in fp32's range; the finite ones with a finite bound are within it; where
    v overflowed and p stayed finite the update is zero (p moved by its decay's roundings at
    most); the shadow is RNE of the kernel's own p, NaN for NaN."""
    bkeys = {"p": "bp", "m": "bm", "v": "bv", "buf": "bb"}
    cs, names = [], []
    for k in (("p", "m", "v") if kind == "adam" else ("p", "buf")):
        if ref.get(k) is None:
            continue
        same = classes(out[k]) == classes(ref[k])
        cs.append(Cmp(bool(same.all()), 0.0 if bool(same.all()) else math.inf, f"{int((~same).sum())} classes differ"))
        skip = ~torch.isfinite(ref[k]) | ~torch.isfinite(ref[bkeys[k]])
        cs.append(cmp_bound(out[k], ref[k], ref[bkeys[k]], skip))
        names += [k + " class", k]
    if kind == "adam":
        z = torch.isinf(ref["v"]) & torch.isfinite(ref["p"])
        cs.append(cmp_bound(out["p"], ref["p"], 4 * U * ref["p"].abs() + TINY, ~z))
        names.append("zero update")
    if shadow is not None:
        cs.append(cmp_exact(shadow, _bf(out["p"])))
        names.append("shadow vs own p")
    return _join(names, cs)


def exact_sum_ok(a, b):
    """a + b is exact in float64 for these fp32 / bf16 values (Fast2Sum's test both ways)."""
    a, b = a.double(), b.double()
    s = a + b
    return bool(((s - a == b) & (s - b == a)).all())


def check_multi_copy(out, src, dst0, scale, accumulate) -> Cmp:
    """One pair.  scale a power of two: src * scale is exact, so the fp32 result is the float64
    value rounded once whatever the contraction -- compared bitwise (a bf16 destination: RNE
    of that fp32).  Otherwise by bound (k = K_COPY), a bf16 destination through cmp_bf16."""
    ref, mag = ref_multi_copy(src, dst0, scale, accumulate)
    m, _ = math.frexp(f32(scale))
    if m == 0.5:
        assert exact_sum_ok(src.double() * f32(scale), dst0 if accumulate else torch.zeros_like(dst0))
        exp32 = ref.float()
        return cmp_exact(out, _bf(exp32) if out.dtype == torch.bfloat16 else exp32)
    if out.dtype == torch.bfloat16:
        # The kernel rounds twice, to fp32 and then to bf16.  A bf16 source times fp32(1/3) is within
        # 2^-25 of a short value whenever the source is a multiple of 3, and adding a bf16 then lands
        # that close to a bf16 tie for percents of the elements: the fp32 rounding makes it an exact
        # tie and RNE may go the other way than the float64 value does.  Elements whose bf16 an
        # evaluation within its fp32 bound may decide either way are therefore held to the bound
        # (all elements are) but left out of the count of differing bf16s.
        e = K_COPY * U * mag
        amb = round_bf16(ref - e) != round_bf16(ref + e)
        b = cmp_bound(out, ref, 2.0 ** -8 * ref.abs() + e + 2.0 ** -133)
        c = cmp_bf16(out, ref, mag, k=K_COPY, skip=amb)
        return Cmp(b.ok and c.ok, max(b.ratio, c.ratio), f"{c.detail} ({int(amb.sum())} near a bf16 tie)")
    return cmp_bound(out, ref, K_COPY * U * mag + TINY)


# (elements, source offset, destination offset) of the pairs of one table: both sides sit at element
# offsets 0, 1 and 3 of their storage; 16,383 and 40,000 (three chunks) are 16-byte aligned on both
# sides, so an fp32 -> fp32 table runs the float4 body with a 3-element tail and the scalar path
COPY_LAYOUT = ((1, 3, 0), (CHUNK - 1, 0, 0), (CHUNK, 1, 1), (CHUNK + 1, 0, 3), (40000, 0, 0))
COPY_SIZES = tuple(n for n, _, _ in COPY_LAYOUT)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
COPY_DTYPE_PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")]


def make_copy_pairs(sdt, ddt, seed):
    """[(src storage, src offset, dst storage, dst offset)] of one table on the CPU."""
    g = torch.Generator().manual_seed(seed)
    pairs = []
    for n, so, do in COPY_LAYOUT:
        s = torch.randn(n + so, generator=g).to(DTYPES[sdt])
        d = torch.randn(n + do, generator=g).to(DTYPES[ddt])
        pairs.append((s, so, d, do))
    return pairs
