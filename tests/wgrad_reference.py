"""float64 reference of the convolution weight gradient (csrc/conv_wgrad.hip), the operand
makers and the two comparisons tests/test_conv_wgrad_fp64.py holds the kernels to, and the
geometry lists that file shares with tests/test_wgrad_reference.py (which checks all of
this on the CPU, before anything runs on a GPU).

    dW[co][r][s][ci] = sum over (n, oh, ow) of dy[n][oh][ow][co] * x[n][oh sh - ph + r][ow sw - pw + s][ci]

with x zero outside the image.  Tensors are NHWC; the result is [Cout, KH, KW, Cin], the
channels_last weight's memory order and the kernel's output layout.

Two kinds of operands:
  * integers in {+-1, +-2, +-3, +-4}, no zeros: exact in bf16, every product at most 16 in
    magnitude, so every partial sum of up to 2^20 rows is an integer below 2^24 and the fp32
    accumulation is exact in ANY order -- across waves, row splits and the reduce kernel.
    The comparison is ``torch.equal``; a dropped, doubled or misplaced row or tap changes
    every output it touches, because no operand is zero;
  * ``randn`` rounded to bf16, compared element by element under
    ``|got - ref| <= 2 K 2^-24 A`` with K = N OH OW the reduction length and A the same sum
    over |dy| and |x|: bf16 x bf16 products are exact in fp32, any-order fp32 summation of K
    terms errs by at most K 2^-24 A, the factor 2 covers the MFMA's internal adder (the
    accumulation term of tests/test_conv_partition.py's bound; the output is fp32, so there
    is no bf16 rounding term).  One missing term is about A / K, i.e. 2^23 / K^2 bounds:
    at K <= 512 more than 30 of them, which is why the random cases stay that short.
Nothing here reads a kernel's output to decide a tolerance."""
from collections import namedtuple

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
MAX_RANDOM_ROWS = 512      # the longest reduction the element-wise bound is used at
MAX_EXACT_ROWS = 1 << 20   # 16 * 2^20 = 2^24: integer operands stay exact in fp32 up to here


class Geo(namedtuple("Geo", "n h w kh kw sh sw ph pw")):
    """x [n, h, w, Cin], a kh x kw filter, strides (sh, sw), zero padding (ph, pw)."""
    __slots__ = ()

    @property
    def oh(self):
        return (self.h + 2 * self.ph - self.kh) // self.sh + 1

    @property
    def ow(self):
        return (self.w + 2 * self.pw - self.kw) // self.sw + 1

    @property
    def rows(self):
        return self.n * self.oh * self.ow

    @property
    def tag(self):
        return (f"{self.n}x{self.h}x{self.w}-k{self.kh}x{self.kw}-s{self.sh}x{self.sw}-p{self.ph}x{self.pw}")


def sq(n, h, w, k, s, p):
    """A square filter with equal strides and pads."""
    return Geo(n, h, w, k, k, s, s, p, p)


def pointwise(m):
    """A 1x1 / stride 1 layer of m rows (one image, one column: the kernels see only rows)."""
    return Geo(1, m, 1, 1, 1, 1, 1, 0, 0)


def halo(n, h, w):
    """3x3 / stride 1 / pad 1: the geometry of the halo kernel."""
    return Geo(n, h, w, 3, 3, 1, 1, 1, 1)


# ------------------------------------------------------------------ float64 reference
def wgrad_ref(dy, x, KH, KW, sh, sw, ph, pw):
    """float64 [Cout, KH, KW, Cin] from NHWC dy [N, OH, OW, Cout] and x [N, H, W, Cin] of any
    dtype and device: per tap dy2d^T @ x_shifted2d, the zero padding written out."""
    n, oh, ow, cout = dy.shape
    nx, h, w, cin = x.shape
    assert n == nx and oh == (h + 2 * ph - KH) // sh + 1 and ow == (w + 2 * pw - KW) // sw + 1, (dy.shape, x.shape)
    xp = F.pad(x.double(), (0, 0, pw, pw, ph, ph))
    d2 = dy.double().reshape(-1, cout).t().contiguous()
    out = torch.zeros(cout, KH, KW, cin, dtype=torch.float64, device=x.device)
    for r in range(KH):
        for s in range(KW):
            xs = xp[:, r:r + (oh - 1) * sh + 1:sh, s:s + (ow - 1) * sw + 1:sw, :]
            out[:, r, s, :] = d2 @ xs.reshape(-1, cin)
    return out


def wgrad_amp(dy, x, KH, KW, sh, sw, ph, pw):
    """The same sum over |dy| and |x|: the magnitude the rounding bound scales with."""
    return wgrad_ref(dy.abs(), x.abs(), KH, KW, sh, sw, ph, pw)


def geo_ref(dy, x, geo):
    return wgrad_ref(dy, x, *geo[3:])


def geo_amp(dy, x, geo):
    return wgrad_amp(dy, x, *geo[3:])


def padding_taps(geo):
    """The taps (r, s) whose every source pixel lies in the zero padding, from the geometry
    alone: their gradient is exactly zero whatever the operands."""
    def inside(k, o, stride, pad, size):
        return any(0 <= i * stride - pad + k < size for i in range(o))

    return [(r, s) for r in range(geo.kh) for s in range(geo.kw)
            if not (inside(r, geo.oh, geo.sh, geo.ph, geo.h) and inside(s, geo.ow, geo.sw, geo.pw, geo.w))]


# ------------------------------------------------------------------ operands
def _gen(geo, cin, cout, seed):
    return torch.Generator(device="cpu").manual_seed(1000 * seed + sum(geo) + 7 * cin + 13 * cout)


def int_operands(geo, cin, cout, seed=1, dtype=torch.bfloat16):
    """(dy, x) with integer values in {+-1, .., +-4}, no zeros (CPU, NHWC)."""
    assert geo.rows <= MAX_EXACT_ROWS
    g = _gen(geo, cin, cout, seed)

    def draw(*shape):
        mag = torch.randint(1, 5, shape, generator=g)
        sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
        return (mag * sign).to(dtype)

    return draw(geo.n, geo.oh, geo.ow, cout), draw(geo.n, geo.h, geo.w, cin)


def randn_operands(geo, cin, cout, seed=2, dtype=torch.bfloat16):
    """(dy, x) standard normal, rounded to ``dtype`` (CPU, NHWC)."""
    g = _gen(geo, cin, cout, seed)
    dy = torch.randn(geo.n, geo.oh, geo.ow, cout, generator=g).to(dtype)
    x = torch.randn(geo.n, geo.h, geo.w, cin, generator=g).to(dtype)
    return dy, x


# ------------------------------------------------------------------ comparisons
Cmp = namedtuple("Cmp", "ok ratio detail")


def _where(bad):
    """Which taps and which 64-channel blocks hold the wrong elements of a [Cout, KH, KW, Cin] mask."""
    cout, kh, kw, cin = bad.shape
    taps = [(r, s) for r in range(kh) for s in range(kw) if bool(bad[:, r, s, :].any())]
    cob = [b for b in range(-(-cout // 64)) if bool(bad[64 * b:64 * b + 64].any())]
    cib = [b for b in range(-(-cin // 64)) if bool(bad[..., 64 * b:64 * b + 64].any())]
    show = taps if len(taps) <= 12 else taps[:12] + ["..."]
    return f"{len(taps)} of {kh * kw} taps {show}, Cout blocks {cob}, Cin blocks {cib}"


def cmp_exact(got, ref) -> Cmp:
    """Integer operands: ``got`` (fp32) is bitwise the float64 reference rounded to fp32 (itself exact)."""
    want = ref.float()
    assert bool((want.double() == ref).all()), "the reference is not exact in fp32: not integer operands?"
    if got.shape != want.shape or got.dtype != torch.float32:
        return Cmp(False, float("inf"), f"shape / dtype {tuple(got.shape)} {got.dtype}")
    if torch.equal(got, want):
        return Cmp(True, 0.0, "exact")
    bad = got != want
    d = (got.double() - ref).abs()
    return Cmp(False, float("inf"),
               f"{int(bad.sum())} of {bad.numel()} elements differ (largest by {float(d.max()):g}): " + _where(bad))


def cmp_bound(got, ref, amp, k) -> Cmp:
    """Random operands: no element past 2 k 2^-24 amp of the float64 reference.  ratio = the
    worst error / bound."""
    if got.shape != ref.shape or got.dtype != torch.float32:
        return Cmp(False, float("inf"), f"shape / dtype {tuple(got.shape)} {got.dtype}")
    if not bool(torch.isfinite(got).all()):
        return Cmp(False, float("inf"), "non-finite output")
    err = (got.double() - ref).abs()
    bound = 2.0 * k * U24 * amp
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    bad = ratio > 1.0
    worst = float(ratio.max())
    if not bool(bad.any()):
        return Cmp(True, worst, f"worst {worst:.3f}")
    return Cmp(False, worst,
               f"{int(bad.sum())} of {bad.numel()} elements past the bound, worst {worst:.3g}: " + _where(bad))


# ------------------------------------------------------------------ geometry lists
# The generic tap-GEMM kernel (64 -> 128 channels in the GPU tests): every row count is at most
# MAX_RANDOM_ROWS, so each runs with random and with integer operands.
GENERIC_GEOMS = [
    sq(4, 14, 14, 3, 2, 1),            # stride 2 at even H: 14 -> 7 (ResNet's own 56 -> 28)
    sq(3, 15, 15, 3, 2, 1),            # stride 2 at odd H
    sq(3, 9, 9, 3, 1, 0),              # no padding
    sq(4, 14, 14, 1, 2, 0),            # the strided 1x1 of the downsample branch, even H
    Geo(3, 15, 13, 1, 1, 2, 2, 0, 0),  # ... odd H and W
    sq(5, 12, 10, 7, 2, 3),            # 7x7 / 2 / 3: 49 taps
    Geo(4, 9, 11, 1, 3, 2, 1, 0, 1),   # 1x3, stride (2, 1), pad (0, 1)
    Geo(4, 9, 11, 3, 1, 1, 2, 1, 0),   # 3x1, stride (1, 2), pad (1, 0)
    sq(7, 2, 3, 5, 1, 2),              # 5x5 on a 2x3 image: the taps of filter rows 0 and 4 lie wholly in padding
    halo(2, 3, 65),                    # 3x3 / 1 / 1 too wide for the halo kernel
    halo(2, 3, 70),
]
PADDING_GEOM = GENERIC_GEOMS[8]

# The halo kernel picks its stage shape by OW <= 16 / 32 / 64: R = 4 / 2 / 1 output rows per stage.
HALO_WIDTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64)
HALO_HN = ((1, 1), (2, 3), (3, 3), (5, 1), (5, 3))   # (H, N)
HALO_GEOMS = [halo(n, h, w) for w in HALO_WIDTHS for h, n in HALO_HN]


def halo_owp(ow):
    """Pixels per stage row of the halo kernel (wgrad3x3_owp)."""
    return 16 if ow <= 16 else 32 if ow <= 32 else 64


def halo_stages(geo):
    """(R output rows per stage, T stages in all) of the halo kernel: a stage never crosses an image."""
    r = 64 // halo_owp(geo.ow)
    return r, geo.n * (-(-geo.oh // r))
