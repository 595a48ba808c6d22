"""float64 references of every stage of csrc/bn_act.hip and csrc/pool.hip, the input
generators and the comparison functions of tests/test_bn_kernels.py and
tests/test_pool_kernels.py, and an fp32 emulation of each stage (with deliberately
wrong variants) that tests/test_bn_reference.py uses to show the comparisons are sharp.

Every ``ref_*`` function takes the operands the kernel takes (rows [M, C], NHWC for the
pools) and computes in float64 on whatever device they live on.  Nothing here reads a
kernel's output to decide a tolerance: every bound is derived where it is computed."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # fp32 unit roundoff (half an ulp, relative)
HALF_BF16 = 2.0 ** -8   # bf16 keeps 8 significant bits: half an ulp is at most 2^-8 |v|
SHARE = 1e-3            # largest accepted share of bf16 outputs whose bits differ from the reference's
K_APPLY = 4             # fp32 roundings of a three-addend affine map: two products, two additions

Cmp = namedtuple("Cmp", "ok ratio detail")


# ------------------------------------------------------------------ bf16 rounding
def round_bf16(v: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even), returned as float64.  Explicit,
    because ``tensor.double().bfloat16()`` rounds to fp32 first (1 + 2^-8 + 2^-30 becomes
    1.0 that way instead of 1 + 2^-7).  ``truncate``: round toward zero (a wrong store)."""
    v = v.double()
    fin = torch.isfinite(v) & (v != 0)
    a = torch.where(fin, v, torch.ones_like(v))
    # integer arithmetic on the bit pattern only (no frexp / ldexp / pow / division, which
    # a device may evaluate inexactly): |a| = m * 2^e with m in [0.5, 1)
    e = ((a.view(torch.int64) >> 52) & 0x7FF) - 1022
    e = torch.clamp(e, min=-125)               # below 2^-126 the spacing stays 2^-133

    def pow2(k):                               # 2^k as float64, |k| < 1022
        return ((k + 1023) << 52).view(torch.float64)

    q = pow2(e - 8)                            # spacing of 8-bit significands at this exponent
    r = a * pow2(8 - e)                        # a / q, exact
    r = (torch.trunc(r) if truncate else torch.round(r)) * q   # torch.round: half to even
    r = torch.where(r.abs() >= 2.0 ** 128, torch.copysign(torch.full_like(r, math.inf), r), r)
    return torch.where(fin, r, v)


def to_bf16(v: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """The bf16 tensor holding ``round_bf16(v)`` (bf16 values are exact in fp32)."""
    return round_bf16(v, truncate).float().to(torch.bfloat16)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def same_bf16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise: the same bf16 bits, or both NaN (the payload is not specified)."""
    return (bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))


# ------------------------------------------------------------------ launch geometry
def rpi_of(C: int) -> int:
    return 256 // (C // 8)


def bn_plan(M: int, C: int):
    """(rows per block, blocks) of the partial kernels (csrc/bn_act.hip bn_plan)."""
    rpi = rpi_of(C)
    blocks = min(max(-(-M // (16 * rpi)), 1), 512)
    rpb = -(-M // blocks)
    return rpb, max(-(-M // rpb), 1)


def block_sums(t: torch.Tensor, rpb: int) -> torch.Tensor:
    """[M, C] float64 -> [blocks, C]: the sum of each run of ``rpb`` rows."""
    M, C = t.shape
    nb = -(-M // rpb)
    if nb * rpb != M:
        t = torch.cat([t, t.new_zeros(nb * rpb - M, C)])
    return t.view(nb, rpb, C).sum(1)


def block_terms(M: int, rpb: int, device=None) -> torch.Tensor:
    nb = -(-M // rpb)
    n = torch.full((nb,), float(rpb), dtype=torch.float64, device=device)
    n[-1] = M - (nb - 1) * rpb
    return n


# ------------------------------------------------------------------ references
def _partial(t1, t2, rpb):
    S = torch.stack([block_sums(t1, rpb), block_sums(t2, rpb)], 1)
    A = torch.stack([block_sums(t1.abs(), rpb), block_sums(t2.abs(), rpb)], 1)
    return S, A, block_terms(t1.shape[0], rpb, t1.device)


def ref_partial_fwd(x, rpb=None):
    """(S, Sabs, n): S [blocks, 2, C] = per-block sums of x and x^2, Sabs the sums of
    the terms' magnitudes, n [blocks] the rows of each block (one block when rpb is None)."""
    x = x.double().reshape(-1, x.shape[-1])
    return _partial(x, x * x, rpb or x.shape[0])


def ref_masked_d(x, dy, dy2=None, y=None, ss=None, relu=False, round_d=False, ge=False):
    """The gradient the backward kernels work on: dy (+ dy2), zeroed where the forward's
    ReLU output was not positive (read from y, or recomputed as x * scale + shift from
    the [4, C] stats), then rounded to bf16 when the kernel writes it (``dout``).
    ``ge``: the wrong mask >= 0."""
    d = dy.double()
    if dy2 is not None:
        d = d + dy2.double()
    if relu:
        act = x.double() * ss[2].double() + ss[3].double() if ss is not None else y.double()
        d = torch.where((act >= 0) if ge else (act > 0), d, torch.zeros_like(d))
    return round_bf16(d) if round_d else d


def ref_partial_bwd(x, dy, dy2=None, y=None, ss=None, relu=False, dout=False, rpb=None):
    """(d, S, Sabs, n): the masked d ([M, C] float64; with ``dout`` rounded to bf16 -- the
    expected dout) and the per-block sums of d and d * x as ref_partial_fwd's."""
    x = x.double().reshape(-1, x.shape[-1])
    d = ref_masked_d(x, dy.reshape(x.shape), None if dy2 is None else dy2.reshape(x.shape),
                     None if y is None else y.reshape(x.shape), ss, relu, dout)
    return (d,) + _partial(d, d * x, rpb or x.shape[0])


def ref_finalize(part, count, gamma, beta, rm, rv, nbt, momentum, eps, nbt_pending=0, biased=False,
                 ignore_pending=False):
    """float64 (stats [4, C], new running_mean, new running_var, tol): tol is a dict of the
    per-channel tolerances of the fp32 outputs (derived below).  ``momentum`` and ``eps`` are
    used at their fp32 values, as the kernel receives them; ``nbt`` is the counter's value
    when the kernel reads it.  ``biased`` / ``ignore_pending``: wrong variants."""
    p = part.double()
    C = p.shape[-1]
    a, b = p[:, 0].sum(0), p[:, 1].sum(0)
    one = torch.ones(C, dtype=torch.float64, device=p.device)
    zero = torch.zeros_like(one)
    g = gamma.double() if gamma is not None else one
    bt = beta.double() if beta is not None else zero
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mean = a / count
    var = torch.clamp(b / count - mean * mean, min=0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = g * invstd
    shift = bt - mean * scale
    # fp64 summation order: the kernel's slices and tree add the rows in another order than
    # torch.sum; each sum is within nparts * 2^-53 of exact, relative to its terms' magnitudes,
    # and var = b/count - mean^2 passes that on divided by (var + eps)
    n53 = p.shape[0] * 2.0 ** -52
    dvar = n53 * (p[:, 1].abs().sum(0) / count + 2 * mean.abs() * p[:, 0].abs().sum(0) / count)
    rel_is = torch.where(var > 0, 0.5 * dvar / (var + eps), zero)  # clamped: both sides use eps alone
    tol = {
        # (float)mean: one rounding; k = 2
        "mean": 2 * U * mean.abs() + n53 * p[:, 0].abs().sum(0) / count,
        # (float)(1 / sqrt(var + eps)): one rounding of an fp64 value; k = 2
        "invstd": (2 * U + rel_is) * invstd,
        # g * invstd: invstd's rounding and the product's; k = 3
        "scale": (3 * U + rel_is) * scale.abs(),
        # bt - (float)mean * sc: roundings of invstd, g * invstd, (float)mean, mean * sc and
        # the subtraction = 5 fp32 operations (a contracted fma saves one); each is at most
        # u relative to |mean * scale| or to the result, |result| <= |beta| + |mean * scale|
        "shift": (5 * U + rel_is) * (bt.abs() + (mean * scale).abs()),
    }
    stats = torch.stack([mean, invstd, scale, shift])
    new_rm = new_rv = None
    if rm is not None:
        if momentum >= 0:
            mom = float(torch.tensor(momentum, dtype=torch.float32))
        else:
            mom = 1.0 / float((int(nbt) + (0 if ignore_pending else int(nbt_pending))) if nbt is not None else 1)
        unb = var if (biased or count <= 1.0) else var * count / (count - 1.0)
        new_rm = (1.0 - mom) * rm.double() + mom * mean
        new_rv = (1.0 - mom) * rv.double() + mom * unb
        # (1 - mom) * r + mom * (float)v: 1 / nbt, 1 - mom, two products, the cast and the
        # addition = 6 fp32 operations, each at most u relative to one of the two addends
        tol["running_mean"] = 6 * U * (((1.0 - mom) * rm.double()).abs() + (mom * mean).abs()) + tol["mean"]
        tol["running_var"] = 6 * U * (((1.0 - mom) * rv.double()).abs() + (mom * unb).abs()) \
            + abs(mom) * dvar * (1.0 if count <= 1.0 else count / (count - 1.0))
    return stats, new_rm, new_rv, tol


def ref_bwd_finalize(part, count, gamma, mean, invstd, cc_no_count=False):
    """float64 (coef [5, C] = dgamma, dbeta, A, B, Cc; tol [5, C]).  ``cc_no_count``: wrong."""
    p = part.double()
    C = p.shape[-1]
    a, b = p[:, 0].sum(0), p[:, 1].sum(0)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device=p.device)
    mean, istd = mean.double(), invstd.double()
    dbeta = a
    dgamma = (b - mean * a) * istd
    A = g * istd
    B = -A * istd * dgamma / count
    t1 = A * dbeta if cc_no_count else A * dbeta / count
    Cc = -t1 - B * mean
    n53 = p.shape[0] * 2.0 ** -52  # fp64 summation order, as in ref_finalize
    da, db = n53 * p[:, 0].abs().sum(0), n53 * p[:, 1].abs().sum(0)
    ddg = (db + mean.abs() * da) * istd.abs()
    tol = torch.stack([
        2 * U * dgamma.abs() + ddg,            # one cast of an fp64 value; k = 2
        2 * U * dbeta.abs() + da,              # one cast; k = 2
        2 * U * A.abs(),                       # one product; k = 2
        # -A * istd * dgamma / (float)count: A, the cast of dgamma, two products, the
        # division = 5 roundings; k = 6
        6 * U * B.abs() + (A * istd / count).abs() * ddg,
        # -A * dbeta / count - B * mean: the first term carries 4 roundings (A, dbeta, product,
        # division), the second 6 (B's five and the product), the subtraction one more,
        # relative to at most |t1| + |t2|: k = 7
        7 * U * (t1.abs() + (B * mean).abs()) + (A / count).abs() * da + (A * istd / count * mean).abs() * ddg,
    ])
    return torch.stack([dgamma, dbeta, A, B, Cc]), tol


def ref_apply(x, scale, shift, res=None, relu=False):
    """(y float64, sum of the addends' magnitudes): relu(x * scale + shift (+ res))."""
    t = x.double() * scale.double()
    y = t + shift.double()
    mag = t.abs() + shift.double().abs()
    if res is not None:
        y = y + res.double()
        mag = mag + res.double().abs()
    return (torch.clamp(y, min=0.0) if relu else y), mag.expand_as(y)


def ref_bwd_apply(x, d, coef):
    """(dx float64, sum of the addends' magnitudes): A d + B x + Cc with the masked d."""
    A, B, Cc = coef[2].double(), coef[3].double(), coef[4].double()
    t1, t2 = A * d.double(), B * x.double()
    return t1 + t2 + Cc, t1.abs() + t2.abs() + Cc.abs()


def ambiguous(x, ss):
    """Elements whose recomputed ReLU mask an fp32 evaluation may decide either way:
    |x * scale + shift| <= 4 u (|x * scale| + |shift|) in float64."""
    t = x.double() * ss[2].double()
    return (t + ss[3].double()).abs() <= 4 * U * (t.abs() + ss[3].double().abs())


def pool_out(H, W, k, s, pad):
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


def ref_maxpool(x, k, s, pad, last_tie=False):
    """x [N, H, W, C] -> (y float64, arg uint8): a scan of the window in row-major order
    that takes an element when it is greater than the running maximum or NaN, starting
    from the first element inside the image (PyTorch's rule: the first maximum wins a
    tie, every NaN wins).  arg = kh * k + kw.  ``last_tie``: the wrong rule >=."""
    x = x.double()
    N, H, W, C = x.shape
    OH, OW = pool_out(H, W, k, s, pad)
    xp = torch.full((N, H + 2 * pad, W + 2 * pad, C), -math.inf, dtype=torch.float64, device=x.device)
    xp[:, pad:pad + H, pad:pad + W] = x
    inside = torch.zeros(1, H + 2 * pad, W + 2 * pad, 1, dtype=torch.bool, device=x.device)
    inside[:, pad:pad + H, pad:pad + W] = True
    m = torch.full((N, OH, OW, C), -math.inf, dtype=torch.float64, device=x.device)
    arg = torch.full((N, OH, OW, C), -1, dtype=torch.int16, device=x.device)
    for kh in range(k):
        for kw in range(k):
            sl = (slice(None), slice(kh, kh + (OH - 1) * s + 1, s), slice(kw, kw + (OW - 1) * s + 1, s))
            v, ok = xp[sl], inside[sl]
            take = ((v >= m) if last_tie else (v > m)) | torch.isnan(v) | (arg < 0)
            take = take & ok
            m = torch.where(take, v, m)
            arg = torch.where(take, torch.full_like(arg, kh * k + kw), arg)
    return m, arg.to(torch.uint8)


def ref_maxpool_bwd(dy, arg, H, W, k, s, pad):
    """float64 scatter-add of dy [N, OH, OW, C] through the argmax bytes -> [N, H, W, C]."""
    dy = dy.double()
    N, OH, OW, C = dy.shape
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=torch.float64, device=dy.device)
    for kh in range(k):
        for kw in range(k):
            sl = (slice(None), slice(kh, kh + (OH - 1) * s + 1, s), slice(kw, kw + (OW - 1) * s + 1, s))
            dxp[sl] += torch.where(arg == kh * k + kw, dy, torch.zeros_like(dy))
    return dxp[:, pad:pad + H, pad:pad + W].contiguous()


def ref_gap_bwd(dy, HW):
    """dy [N, C] -> float64 [N, HW, C]: dy / HW at every pixel."""
    return (dy.double() / HW)[:, None, :].expand(dy.shape[0], HW, dy.shape[1]).contiguous()


# ------------------------------------------------------------------ comparisons
def _ratio(err, bound):
    """max err / bound; inf where err exceeds a zero bound or is not a number."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def cmp_bound(out, ref, bound, skip=None) -> Cmp:
    """|out - ref| <= bound elementwise (``skip``: elements left out)."""
    err = (out.double() - ref.double()).abs()
    err = torch.where(torch.isnan(err) & torch.isnan(out.double()) & torch.isnan(ref.double()),
                      torch.zeros_like(err), err)
    if skip is not None:
        err = torch.where(skip, torch.zeros_like(err), err)
    r = _ratio(err, bound.double().expand_as(err))
    return Cmp(r <= 1.0, r, f"worst error / bound {r:.3g}")


def cmp_part(part, S, Sabs, n, extra=None) -> Cmp:
    """fp32 per-block sums against float64.  A block adds n terms in some order: n - 1
    roundings, each at most u times a partial sum of magnitudes <= sum |term|, plus at
    most one rounding forming a term (the products of two bf16 values are exact; d * x
    with an exact 24-bit d = dy + dy2 rounds once): n u sum |term|.  ``extra``: added to
    the bound (the ambiguous elements' share)."""
    if part.shape[0] != S.shape[0]:  # the blocks' row ranges are unknown: compare the totals
        M = n.sum()
        S, Sabs, part = (t.double().sum(0, keepdim=True) for t in (S, Sabs, part))
        n = M[None]
    bound = n[:, None, None] * U * Sabs
    if extra is not None:
        bound = bound + extra
    return cmp_bound(part, S, bound)


def cmp_bf16(out, ref, mag, k=K_APPLY, skip=None) -> Cmp:
    """A bf16 output of an fp32 evaluation against float64:
    |out - ref| <= 2^-8 |ref| + k u sum |addends|  -- the bf16 store is within half an ulp
    (<= 2^-8 |v|) of the fp32 value, which is within k roundings, each at most u times the
    addends' magnitudes, of the exact one (2^-133, the smallest bf16 spacing, covers
    results below the normal range) -- and at most SHARE of the outputs may differ from
    the reference's bf16 at all."""
    ref = ref.double()
    bound = HALF_BF16 * ref.abs() + k * U * mag.double() + 2.0 ** -133
    c = cmp_bound(out, ref, bound, skip)
    diff = ~same_bf16(out, to_bf16(ref))
    if skip is not None:
        diff = diff & ~skip
    share = float(diff.double().mean()) if diff.numel() else 0.0
    return Cmp(c.ok and share <= SHARE, c.ratio, f"{c.detail}, {share:.3g} of the bf16 outputs differ")


def cmp_exact(out, ref_bf16) -> Cmp:
    bad = int((~same_bf16(out, ref_bf16)).sum()) if out.dtype == torch.bfloat16 else int((out != ref_bf16).sum())
    return Cmp(bad == 0, 0.0 if bad == 0 else math.inf, f"{bad} of {out.numel()} elements differ")


# ------------------------------------------------------------------ inputs
def flush_small(t, lo=2.0 ** -9):
    """bf16 values with |v| >= lo: two such values below 2^4 add exactly in fp32."""
    f = t.float()
    return torch.where(f.abs() < lo, torch.where(f < 0, -lo, lo), f).to(torch.bfloat16)


def make_rows(C, M, seed, grid=False):
    """Deterministic CPU inputs of one [M, C] case.  x: per-channel means and spreads, both
    signs present.  ``grid``: x = i / 32, |i| <= 255, so that x * scale + shift is exact in
    fp32 for exact_ss's coefficients.  dy, dy2: |v| >= 2^-9, so dy + dy2 is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(C, generator=g) * 1.5
    sd = 0.25 + 2 * torch.rand(C, generator=g)
    x = torch.randn(M, C, generator=g) * sd + mu
    if grid:
        x = torch.clamp(torch.round(x * 32), -255, 255) / 32
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    return {
        "x": x.to(torch.bfloat16),
        "dy": flush_small(torch.randn(M, C, generator=g).to(torch.bfloat16)),
        "dy2": flush_small((0.5 * torch.randn(M, C, generator=g)).to(torch.bfloat16)),
        "res": torch.randn(M, C, generator=g).to(torch.bfloat16),
        "gamma": (0.5 + torch.rand(C, generator=g)) * sign,
        "beta": 0.5 * torch.randn(C, generator=g),
        "mu": mu, "sd": sd,
    }


def exact_ss(C, seed):
    """[4, C] fp32 stats whose scale = j / 64 (32 <= |j| <= 127, both signs) and
    shift = l / 64 (|l| <= 128) are bf16 values: with x = i / 32 the map is
    (i j + 32 l) / 2048, an integer below 2^16 over a power of two -- exact in fp32."""
    g = torch.Generator().manual_seed(seed + 7919)
    j = torch.randint(32, 128, (C,), generator=g).float() * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    sh = torch.randint(-128, 129, (C,), generator=g).float()
    return torch.stack([torch.zeros(C), torch.ones(C), j / 64, sh / 64])


def assert_exact_affine(x, ss):
    """The test's own check that the recomputed mask leaves no rounding freedom."""
    v = x.double() * ss[2].double() + ss[3].double()
    assert torch.equal(v.float().double(), v), "x * scale + shift is not exact in fp32"
    t = x.double() * ss[2].double()
    assert torch.equal(t.float().double(), t)


def make_fwd_parts(nparts, C, count, seed, clamp_channel=True):
    """Synthetic fp32 [nparts, 2, C] forward partials with per-channel mean m (both signs)
    and variance v >= 0.5, split over the rows with random positive weights; channel 0
    has sum x^2 / count = (1 - 1e-4) m^2, so b / count - mean^2 is slightly negative."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(C, generator=g, dtype=torch.float64) * 1.5
    v = 0.5 + 2 * torch.rand(C, generator=g, dtype=torch.float64)
    w = 0.5 + torch.rand(2, nparts, C, generator=g, dtype=torch.float64)
    w = w / w.sum(1, keepdim=True)
    ex2 = m * m + v
    if clamp_channel:
        m[0] = 1.5
        ex2[0] = (1 - 1e-4) * 2.25
    return torch.stack([count * m * w[0], count * ex2 * w[1]], 1).float()


def make_bwd_parts(nparts, C, seed):
    g = torch.Generator().manual_seed(seed)
    part = torch.randn(nparts, 2, C, generator=g) * 3
    mean = torch.randn(C, generator=g) * 1.5
    invstd = 0.3 + 2 * torch.rand(C, generator=g)
    return part, mean, invstd


def make_pool_x(N, H, W, C, seed, grid=False):
    """NHWC bf16 pool input: a few distinct values (ties inside and across windows), one
    constant plane, NaN, -inf (a whole corner of one plane, so border windows hold
    nothing else, and single pixels).  ``grid``: finite i / 32 values for the BN-folded form."""
    g = torch.Generator().manual_seed(seed)
    if grid:
        x = torch.randint(-96, 97, (N, H, W, C), generator=g).float() / 32
        x[0, :, :, 1] = 0.75
        return x.to(torch.bfloat16)
    x = torch.randint(-3, 4, (N, H, W, C), generator=g).float() / 2
    x[0, :, :, 1] = 0.5
    r = torch.rand(N, H, W, C, generator=g)
    x[r < 0.02] = math.nan
    x[(r >= 0.02) & (r < 0.05)] = -math.inf
    x[N - 1, : (H + 1) // 2, : (W + 1) // 2, 2] = -math.inf
    x[N - 1, H // 2:, W // 2:, 3] = -math.inf
    return x.to(torch.bfloat16)


def make_pool_dy(shape, seed):
    """i / 64, |i| <= 255: bf16 values whose sums of up to 2^9 terms are exact in fp32, so
    the gathered gradient has one rounding, the store's, in the kernel and the reference."""
    g = torch.Generator().manual_seed(seed + 104729)
    return (torch.randint(-255, 256, shape, generator=g).float() / 64).to(torch.bfloat16)


# ------------------------------------------------------------------ fp32 emulation
# What a correct kernel may compute: fp32 arithmetic (unfused), fp64 where the kernel uses
# it, a round-to-nearest bf16 store.  The keyword flags switch on one wrong behaviour each.
def emu_store(v32, truncate=False):
    return to_bf16(v32.double(), truncate)


def emu_partial(t1, t2, rpb, drop_last=False):
    """fp32 per-block sums of two fp32 term tensors [M, C] (sequential over the rows)."""
    M, C = t1.shape
    nb = -(-M // rpb)
    out = torch.zeros(nb, 2, C, dtype=torch.float32)
    for b in range(nb):
        lo, hi = b * rpb, min((b + 1) * rpb, M)
        if drop_last and b == nb - 1:
            hi -= 1
        out[b, 0] = t1[lo:hi].float().sum(0, dtype=torch.float32)
        out[b, 1] = t2[lo:hi].float().sum(0, dtype=torch.float32)
    return out


def emu_masked_d(x, dy, dy2=None, y=None, ss=None, relu=False, ge=False):
    d = dy.float()
    if dy2 is not None:
        d = d + dy2.float()
    if relu:
        act = x.float() * ss[2] + ss[3] if ss is not None else y.float()
        d = torch.where((act >= 0) if ge else (act > 0), d, torch.zeros_like(d))
    return d


def emu_finalize(part, count, gamma, beta, rm, rv, nbt, momentum, eps, nbt_pending=0, biased=False,
                 ignore_pending=False):
    p = part.double()
    C = p.shape[-1]
    a, b = p[:, 0].sum(0), p[:, 1].sum(0)
    g = gamma.float() if gamma is not None else torch.ones(C)
    bt = beta.float() if beta is not None else torch.zeros(C)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    mean = a / count
    var = torch.clamp(b / count - mean * mean, min=0.0)
    invstd = (1.0 / torch.sqrt(var + eps32)).float()
    sc = g * invstd
    stats = torch.stack([mean.float(), invstd, sc, bt - mean.float() * sc])
    if rm is None:
        return stats, None, None
    one = torch.tensor(1.0, dtype=torch.float32)
    if momentum >= 0:
        mom = torch.tensor(momentum, dtype=torch.float32)
    else:
        mom = one / torch.tensor(float(int(nbt) + (0 if ignore_pending else int(nbt_pending))), dtype=torch.float32)
    unb = var if (biased or count <= 1.0) else var * count / (count - 1.0)
    return stats, (one - mom) * rm.float() + mom * mean.float(), (one - mom) * rv.float() + mom * unb.float()


def emu_bwd_finalize(part, count, gamma, mean, invstd, cc_no_count=False):
    p = part.double()
    a, b = p[:, 0].sum(0), p[:, 1].sum(0)
    g = gamma.float() if gamma is not None else torch.ones(p.shape[-1])
    mean, istd = mean.float(), invstd.float()
    dbeta = a.float()
    dgamma = ((b - mean.double() * a) * istd.double()).float()
    cnt = torch.tensor(count, dtype=torch.float32)
    A = g * istd
    B = -A * istd * dgamma / cnt
    t1 = -A * dbeta if cc_no_count else -A * dbeta / cnt
    return torch.stack([dgamma, dbeta, A, B, t1 - B * mean])


def emu_apply(x, scale, shift, res=None, relu=False, truncate=False, drop_last=False):
    v = x.float() * scale.float() + shift.float()
    if res is not None:
        v = v + res.float()
    if relu:
        v = torch.clamp(v, min=0.0)
    y = emu_store(v, truncate)
    if drop_last:
        y[-1] = 0
    return y


def emu_bwd_apply(x, d32, coef, truncate=False):
    return emu_store(coef[2].float() * d32 + coef[3].float() * x.float() + coef[4].float(), truncate)


def emu_maxpool(x, k, s, pad, last_tie=False):
    """(y bf16, arg): the float64 scan on bf16 data is exact, so the emulation is the
    reference with the wrong tie rule switched on."""
    m, arg = ref_maxpool(x, k, s, pad, last_tie)
    return m.float().to(torch.bfloat16), arg


def torch_pool_bytes(x_nchw, k, s, pad):
    """The window position of F.max_pool2d's flat argmax indices, as the kernels' byte."""
    _, idx = F.max_pool2d(x_nchw, k, s, pad, return_indices=True)
    W = x_nchw.shape[-1]
    OH, OW = idx.shape[-2:]
    h, w = idx // W, idx % W
    oh = torch.arange(OH).view(1, 1, OH, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    return ((h - (oh * s - pad)) * k + (w - (ow * s - pad))).to(torch.uint8)


# ------------------------------------------------------------------ cases
CHANNELS = (8, 24, 40, 64, 136, 1032, 2048)


def small_rows(C, unroll):
    """1, rpi - 1, two ragged blocks, and a thread that walks unroll + 1 rows."""
    rpi = rpi_of(C)
    return sorted({1, rpi - 1, 16 * rpi + 3, unroll * rpi + 1} - {0})


# forward partial: every C with every small M; the block cap (512 blocks) at C = 2048 only
FWD_PARTIAL_CASES = [(C, M) for C in CHANNELS for M in small_rows(C, 8)] + [(2048, 8192 + 37)]
# backward partial, per variant: each C once, each kind of M at least once (U = 4)
BWD_PARTIAL_CASES = [(8, 4 * 256 + 1), (8, 255), (24, 16 * 85 + 3), (40, 4 * 51 + 1), (64, 16 * 32 + 3), (136, 14),
                     (1032, 5), (1032, 19), (2048, 1), (2048, 19)]
# apply kernels: small M per C, and above 2048 * rpi rows (one block per rpi rows up to 2048
# blocks): 2048 rpi + 7 gives some threads two rows in flight and the rest the lone tail,
# 2 * 2048 rpi + 5 gives some threads the pair AND the odd tail
APPLY_CASES = [(8, 255), (24, 16 * 85 + 3), (40, 50), (64, 31), (136, 243), (1032, 1), (2048, 19),
               (8, 2048 * 256 + 7), (64, 2 * 2048 * 32 + 5), (136, 2048 * 15 + 7), (1032, 2 * 2048 + 5),
               (2048, 2 * 2048 + 5)]
NPARTS = (1, 7, 64, 65, 512, 513, 520)
POOL_GEOMETRIES = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (1, 1, 0), (1, 2, 0), (2, 3, 0), (5, 3, 2), (4, 2, 2), (7, 2, 3),
                   (15, 4, 7)]
# backward variants reachable through the bindings: (mask, dy2, dout / dres)
#   mask None: no ReLU; "y": ReLU masked by the saved output; "ss": recomputed from the stats
BWD_PARTIAL_VARIANTS = [(m, d2, wd) for m in (None, "y", "ss") for d2 in (False, True) for wd in (False, True)
                        if not (m == "ss" and wd)]   # the binding rejects dout with ss
BWD_APPLY_VARIANTS = [(m, d2, dr) for m in (None, "y", "ss") for d2 in (False, True) for dr in (False, True)
                      if not (m == "ss" and dr)]     # the binding rejects dres with ss


def case_seed(C, M):
    return 1000 * C + M % 997


def pool_shape(k, s, pad, C):
    """(N, H, W): H != W, more than one block of 256 threads, N OH OW C/8 no multiple of 256."""
    H, W = max(k, 2) + 2 * s + 4, max(k, 2) + 3 * s + 3
    if H == W:
        W += 1
    return 3, H, W


def bwd_operands(C, M, mask):
    """The [M, C] operands of one backward case on the CPU: the rows (on the exact grid
    where the mask is recomputed from them), the [4, C] stats, and for the y mask the
    saved output of relu(bn(x) + res) (zeros included)."""
    inp = make_rows(C, M, case_seed(C, M), grid=mask == "ss")
    inp["ss"] = exact_ss(C, case_seed(C, M))
    if mask == "y":
        y, _ = ref_apply(inp["x"], inp["ss"][2], inp["ss"][3], inp["res"], True)
        inp["y"] = to_bf16(y)
    return inp


def check_partial_bwd(part, dout, inp, variant, rpb) -> Cmp:
    mask, dy2, wd = variant
    d, S, A, n = ref_partial_bwd(inp["x"], inp["dy"], inp["dy2"] if dy2 else None, inp["y"] if mask == "y" else None,
                                 inp["ss"] if mask == "ss" else None, mask is not None, wd, rpb)
    c = cmp_part(part, S, A, n)
    if wd:  # dy + dy2 is exact in fp32: the stored d has one rounding on both sides
        e = cmp_exact(dout, d.float().to(torch.bfloat16))
        return Cmp(c.ok and e.ok, c.ratio, c.detail + "; dout: " + e.detail)
    return c


def check_bwd_apply(dx, dres, inp, coef, variant) -> Cmp:
    mask, dy2, dr = variant
    d = ref_masked_d(inp["x"], inp["dy"], inp["dy2"] if dy2 else None, inp["y"] if mask == "y" else None,
                     inp["ss"] if mask == "ss" else None, mask is not None)
    ref, mag = ref_bwd_apply(inp["x"], d, coef)
    c = cmp_bf16(dx, ref, mag)
    if dr:
        e = cmp_exact(dres, to_bf16(d))
        return Cmp(c.ok and e.ok, c.ratio, c.detail + "; dres: " + e.detail)
    return c


def check_finalize(stats, new_rm, new_rv, part, count, gamma, beta, rm, rv, nbt, momentum, eps, pending) -> Cmp:
    ref, rrm, rrv, tol = ref_finalize(part, count, gamma, beta, rm, rv, nbt, momentum, eps, pending)
    cs = [cmp_bound(stats[i], ref[i], tol[k]) for i, k in enumerate(("mean", "invstd", "scale", "shift"))]
    names = ["mean", "invstd", "scale", "shift"]
    if rm is not None:
        cs += [cmp_bound(new_rm, rrm, tol["running_mean"]), cmp_bound(new_rv, rrv, tol["running_var"])]
        names += ["running_mean", "running_var"]
    return Cmp(all(c.ok for c in cs), max(c.ratio for c in cs),
               ", ".join(f"{n} {c.ratio:.3g}" for n, c in zip(names, cs)))


def check_bwd_finalize(coef, part, count, gamma, mean, invstd) -> Cmp:
    ref, tol = ref_bwd_finalize(part, count, gamma, mean, invstd)
    cs = [cmp_bound(coef[i], ref[i], tol[i]) for i in range(5)]
    return Cmp(all(c.ok for c in cs), max(c.ratio for c in cs),
               ", ".join(f"{n} {c.ratio:.3g}" for n, c in zip(("dgamma", "dbeta", "A", "B", "Cc"), cs)))


def pool_expected(x, k, s, pad, ss=None):
    """(y bf16, arg) of the pool, or of the BN-folded pool of bf16(relu(x scale + shift))
    for stats that make the map exact in fp32 (one rounding, the store's, on both sides)."""
    if ss is not None:
        x = round_bf16(torch.clamp(x.double() * ss[2].double() + ss[3].double(), min=0.0))
    m, arg = ref_maxpool(x, k, s, pad)
    return m.float().to(torch.bfloat16), arg


def apply_coefficients(inp):
    """fp32 scale / shift from the rows' population statistics (the sample's are degenerate
    for a single row): gamma / sd and beta - mu * scale, signs as gamma's."""
    scale = (inp["gamma"].double() / inp["sd"].double()).float()
    return scale, (inp["beta"].double() - inp["mu"].double() * scale.double()).float()


def bwd_coefficients(inp, M, variant):
    """fp32 [5, C] coefficients of one backward case: the reference chain's, from the float64
    sums of the case's own masked gradient and the population mean / invstd.  The count is
    at least 256: with a handful of rows A d and Cc = -A dbeta / count - B mean cancel almost
    entirely (dx of a single row is 0), which would measure fp32 cancellation, not the kernel."""
    mask, dy2, _ = variant
    _, S, _, _ = ref_partial_bwd(inp["x"], inp["dy"], inp["dy2"] if dy2 else None, inp["y"] if mask == "y" else None,
                                 inp["ss"] if mask == "ss" else None, mask is not None)
    coef, _ = ref_bwd_finalize(S, float(max(M, 256)), inp["gamma"], inp["mu"], 1.0 / inp["sd"])
    return coef.float()


FIN_CASES = [(n, C) for n in NPARTS for C in (24, 64)] + [(7, 8), (65, 2048), (520, 136), (513, 1032), (1, 40)]
FIN_COUNTS = (1.0, 50.0, 100352.0)
FIN_MOMENTA = [(0.1, 0), (0.0, 0), (-1.0, 0), (-1.0, 1)]   # (momentum, nbt_pending); < 0: cumulative


def finalize_operands(nparts, C, count, affine):
    """(part, gamma, beta, running_mean, running_var, nbt) of one forward-finalize case."""
    seed = 31 * nparts + C
    g = torch.Generator().manual_seed(seed)
    part = make_fwd_parts(nparts, C, count, seed)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    beta = torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    return part, (gamma if affine else None), (beta if affine else None), rm, rv, 3


# the stem's pooled BatchNorm backward: ((k, s, pad), C, (N, H, W)); the last case gives
# C = 8 (256 rows per pass) threads that run the unrolled loop and its tail
POOLED_BN_CASES = [(g, C, pool_shape(*g, C)) for g in ((3, 2, 1), (2, 3, 0), (5, 3, 2), (3, 1, 1)) for C in (8, 24)] \
    + [((3, 2, 1), 8, (2, 37, 30))]


def pooled_operands(geo, C, shape):
    """CPU operands of one pooled case: grid x [N, H, W, C], exact stats, the expected
    pooled output and argmax bytes, the pooled gradient, gamma."""
    k, s, pad = geo
    N, H, W = shape
    seed = 100 * k + 10 * s + C
    x = make_pool_x(N, H, W, C, seed, grid=True)
    ss = exact_ss(C, seed)
    y, arg = pool_expected(x, k, s, pad, ss)
    g = torch.Generator().manual_seed(seed)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    return {"x": x, "ss": ss, "y": y, "arg": arg, "dyp": make_pool_dy(tuple(y.shape), seed), "gamma": gamma,
            "geo": [H, W, k, s, pad]}


def pooled_reference(op, rpb):
    """The reference chain of the pooled backward: the float64 scatter rounded to bf16 (the
    gradient maxpool_bwd would have stored), masked by the recomputed activation, its
    per-block sums, fp32 coefficients from them, and dx.  -> (S, Sabs, n, coef, dx, mag)"""
    H, W, k, s, pad = op["geo"]
    C = op["x"].shape[-1]
    x = op["x"].reshape(-1, C)
    dfull = round_bf16(ref_maxpool_bwd(op["dyp"], op["arg"], H, W, k, s, pad)).reshape(-1, C)
    d, S, A, n = ref_partial_bwd(x, dfull, ss=op["ss"], relu=True, rpb=rpb)
    dev = x.device
    mean = torch.zeros(C, dtype=torch.float64, device=dev)              # x is uniform on [-3, 3]
    istd = torch.full((C,), 1 / math.sqrt(3.0), dtype=torch.float64, device=dev)
    coef, _ = ref_bwd_finalize(S, float(max(x.shape[0], 256)), op["gamma"], mean, istd)
    coef = coef.float()
    dx, mag = ref_bwd_apply(x, d, coef)
    return S, A, n, coef, dx, mag, d
