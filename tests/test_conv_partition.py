"""The persistent convolution kernels (csrc/conv3x3.hip, csrc/conv1x1.hip, csrc/stem.hip)
at their production work split.

Each workgroup of these kernels owns a contiguous pixel range sized from the device's
CU count and walks several tiles of it as one stream.  On a 256-CU part every shape
small enough for a unit test gives each workgroup exactly one partial tile, so the
tile-to-tile hand-over, the shorter last tile, the statistics carried in registers
across tiles and the compile-time-shape 3x3 instances are never run by the other test
files.  Here the planning CU count is pinned (``set_plan_cus``) so that a small tensor
reproduces the per-workgroup geometry of ResNet-50 at batch 128 on 256 CUs; every test
first asserts from the plan query that it is on the path it claims.

Checks, per kernel family:
  * element-wise against an fp64 reference of the same bf16 operands:
    ``|y - ref| <= 2^-8 |ref| + 2 K 2^-24 A`` with A the fp64 convolution of |x| with
    |w| and K the reduction length (bf16 x bf16 products are exact in fp32; any-order
    fp32 summation errs by at most K 2^-24 A; the bf16 rounding adds 2^-8 relative; the
    factor 2 covers the MFMA's internal adder);
  * the output is bitwise the default plan's (a pixel's MFMA order does not depend on
    the tile it sits in);
  * every partial-statistics row against fp64 sums of the kernel's own bf16 output over
    exactly that row's pixels, within ``n 2^-24 sum|term|`` (fp32 summation of n terms);
  * two runs are bitwise equal; PRE equals the materialised activation's run bitwise.
Each test prints its worst error / bound ratio.  Measured on an MI355X with the factor 2
as stated: 3x3 forward / statistics 0.98, PRE 0.96, dgrad 0.90; 1x1 0.99 (PRE 0.99, fused
backward 0.99); stem 0.99 -- the bf16 rounding term, no element past the bound; the
partial rows stay under 0.06 of their tolerance.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

U24 = 2.0 ** -24
U8 = 2.0 ** -8


def _ops():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture
def plan_cus():
    """``pin(k)`` plans for k CUs (0: the device's); the device value is restored whatever
    the test does."""
    m = _ops()
    device = m.plan_cus()

    def pin(k):
        m.set_plan_cus(k)
        assert m.plan_cus() == (k if k > 0 else device)

    try:
        yield pin
    finally:
        m.set_plan_cus(0)


def _pin_tm(monkeypatch, tm):
    if tm is None:
        monkeypatch.delenv("RLA_CONV3X3_TM", raising=False)
    else:
        monkeypatch.setenv("RLA_CONV3X3_TM", str(tm))


def _worst(y, ref, amp, k, extra=None):
    """max of |y - ref| / (2^-8 |ref| + 2 k 2^-24 amp [+ extra]) and where it is."""
    err = (y.double() - ref).abs()
    bound = U8 * ref.abs() + 2.0 * k * U24 * amp
    if extra is not None:
        bound = bound + extra
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    i = int(ratio.argmax())
    nbad = int((ratio > 1.0).sum())
    return float(ratio.flatten()[i]), i, nbad


def _check_elementwise(tag, y, ref, amp, k, extra=None):
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert bool(torch.isfinite(y.float()).all()), f"{tag}: non-finite output"
    r, i, nbad = _worst(y, ref, amp, k, extra)
    print(f"[bound ratio] {tag}: worst {r:.3f}")
    row = i // ref.size(-1)
    assert r <= 1.0, f"{tag}: {nbad} of {ref.numel()} elements past the bound, worst {r:.3f} at pixel {row} " \
                     f"channel {i % ref.size(-1)}"


def _check_rows(tag, part, terms, ranges):
    """part [rows, 2, C] fp32; terms = (t0, t1) [M, C] fp64 whose sums over pixel range j
    rows 0 / 1 of part[j] must be, within n_j 2^-24 sum|term| (fp32 summation of n_j terms;
    an empty range must be exactly zero)."""
    assert part.dtype == torch.float32 and part.size(0) == len(ranges), (part.shape, len(ranges))
    worst = 0.0
    for j, (lo, hi) in enumerate(ranges):
        for s in range(2):
            got = part[j, s].double()
            if hi <= lo:
                assert bool((got == 0).all()), f"{tag}: padding row {j} stat {s} is not zero"
                continue
            t = terms[s][lo:hi]
            want, tol = t.sum(0), (hi - lo) * U24 * t.abs().sum(0)
            err = (got - want).abs()
            bad = err > tol
            assert not bool(bad.any()), f"{tag}: row {j} (pixels {lo}..{hi}) stat {s}: {int(bad.sum())} channels off, " \
                                        f"worst |err| {float(err.max()):.3e} (sum {float(want.abs().max()):.3e})"
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
    print(f"[row ratio] {tag}: worst {worst:.3f}")


def _stats4(c, seed):
    """bn_finalize's [4, C] layout with random scale / shift of both signs."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    st = torch.randn(4, c, generator=g)
    st[1] = st[1].abs() + 0.5
    return st.to(_dev()).contiguous()


def _apply(x, st):
    """The materialised activation bf16(relu(x * scale + shift)) from the production apply kernel."""
    y = torch.empty_like(x)
    _ops().bn_apply(x, st[2].contiguous(), st[3].contiguous(), None, True, y)
    return y


# ------------------------------------------------------------------------------ 3x3
def conv3x3_ref(x, wt):
    """fp64 y[n][oh][ow][co] = sum x[n][oh + r - 1][ow + s - 1][ci] wt[co][r][s][ci] (NHWC)."""
    n, h, w, _ = x.shape
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    wd = wt.double()
    out = torch.zeros(n, h, w, wt.size(0), dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            out += xp[:, r:r + h, s:s + w, :] @ wd[:, r, s, :].t()
    return out


def conv3x3_dgrad_ref(dy, wt):
    """fp64 dx[n][ih][iw][ci] = sum dy[n][ih - r + 1][iw - s + 1][co] wt[co][r][s][ci] (NHWC)."""
    n, h, w, _ = dy.shape
    dp = F.pad(dy.double(), (0, 0, 1, 1, 1, 1))
    wd = wt.double()
    out = torch.zeros(n, h, w, wt.size(3), dtype=torch.float64, device=dy.device)
    for r in range(3):
        for s in range(3):
            out += dp[:, 2 - r:2 - r + h, 2 - s:2 - s + w, :] @ wd[:, r, s, :]
    return out


# (shape (N, H, W, Cin, Cout), plan CUs, pinned tile size or None (auto),
#  expected (tm, pixels per range, most tiles per workgroup, halo pieces per thread, NX, compile-time instance))
# a small N with a pinned CU count gives the per-workgroup geometry of batch 128 on 256 CUs
C3_CASES = [
    ((2, 56, 56, 64, 64), 4, None, (512, 1568, 4, 6, 7, True)),     # 3 x 512 + 32
    ((3, 56, 56, 64, 64), 4, 512, (512, 2352, 5, 7, 7, True)),      # the NX = pieces edge
    ((2, 56, 56, 64, 64), 4, 256, (256, 1568, 7, 4, 4, False)),
    ((2, 28, 28, 128, 128), 4, None, (512, 784, 2, 5, 5, True)),    # 512 + 272
    ((2, 28, 28, 128, 128), 4, 256, (256, 784, 4, 3, 4, True)),
    ((3, 28, 28, 128, 128), 4, 256, (256, 1176, 5, 4, 4, True)),
    ((4, 14, 14, 256, 256), 8, None, (256, 392, 2, 3, 4, True)),    # 256 + 136
    ((8, 7, 7, 512, 512), 16, None, (256, 196, 1, 3, 4, True)),     # 4 images a range, one tile
    ((6, 7, 7, 512, 512), 8, 256, (256, 294, 2, 4, 4, True)),
    ((7, 11, 13, 48, 64), 1, 256, (256, 1001, 4, 4, 4, False)),
    ((7, 11, 13, 48, 64), 1, 512, (512, 1001, 2, 6, 6, False)),
    ((7, 11, 13, 48, 64), 2, 256, (256, 500.5, 2, 4, 4, False)),    # fractional range edges
    ((7, 11, 13, 48, 64), 2, 512, (512, 500.5, 1, 6, 6, False)),
    ((3, 30, 61, 16, 64), 2, 256, (256, 2745, 11, 5, 5, False)),    # one chunk per tile
    ((3, 30, 61, 16, 64), 2, 512, (512, 2745, 6, 7, 7, False)),
    ((3, 33, 20, 32, 128), 2, 512, (512, 1980, 4, 6, 6, False)),    # wpb 1, two channel blocks
]
_RESNET = {(56, 64), (28, 128), (14, 256), (7, 512)}
C3_DGRAD = [c for c in C3_CASES if c[0][3] % 64 == 0]
C3_PRE = [c for c in C3_CASES if (c[0][1], c[0][3]) in _RESNET or c[0][:3] == (7, 11, 13)]


def _c3_id(case):
    shape, cus, tm, _ = case
    return "x".join(map(str, shape)) + f"-cu{cus}-tm{tm or 'auto'}"


def _c3_plan(case, flip=False, stats=False, pre=False):
    """Asserts the case's plan (set_plan_cus and the tile pin are already in force) and
    returns (wpb, the pixel ranges)."""
    (n, h, w, cin, cout), _, _, (tm, per, tiles, pieces, nx, fixed) = case
    a, b = (cout, cin) if flip else (cin, cout)
    p_tm, wpb, _, p_pieces, p_nx, p_fixed = _ops().conv3x3_plan(n, h, w, a, b, flip, stats, pre)
    m = n * h * w
    ranges = [(m * j // wpb, m * (j + 1) // wpb) for j in range(wpb)]
    ntiles = [-((lo - hi) // p_tm) for lo, hi in ranges]
    assert p_tm == tm and m / wpb == per, (p_tm, m / wpb)
    assert max(ntiles) == tiles, ntiles
    assert p_pieces == pieces, p_pieces
    # PRE always runs a run-time-shape instance (of the same NX unless the case sits at NX - 1 pieces)
    assert bool(p_fixed) == (fixed and not pre), (p_fixed, fixed, pre)
    assert p_nx == (max(4, pieces) if pre else nx), p_nx
    return wpb, ranges


@functools.lru_cache(maxsize=None)
def _c3_data(shape):
    """Operands and fp64 references of a shape, computed once and never written again."""
    n, h, w, cin, cout = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(20 + sum(shape))
    x = torch.randn(n, h, w, cin, generator=g).to(dev).to(torch.bfloat16)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev).to(torch.bfloat16)
    return {"x": x, "wt": wt, "ref": conv3x3_ref(x, wt), "amp": conv3x3_ref(x.abs(), wt.abs())}


@functools.lru_cache(maxsize=None)
def _c3_dgrad_data(shape):
    n, h, w, cin, cout = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(40 + sum(shape))
    dy = torch.randn(n, h, w, cout, generator=g).to(dev).to(torch.bfloat16)
    wt = _c3_data(shape)["wt"]
    return {"dy": dy, "ref": conv3x3_dgrad_ref(dy, wt), "amp": conv3x3_dgrad_ref(dy.abs(), wt.abs())}


@functools.lru_cache(maxsize=None)
def _c3_pre_data(shape):
    d = _c3_data(shape)
    st = _stats4(shape[3], 60 + sum(shape))
    a = _apply(d["x"], st)
    return {"st": st, "a": a, "ref": conv3x3_ref(a, d["wt"]), "amp": conv3x3_ref(a.abs(), d["wt"].abs())}


@gpu
@pytest.mark.parametrize("case", C3_CASES, ids=_c3_id)
def test_conv3x3_forward_multi_tile(case, plan_cus, monkeypatch):
    """Forward over several tiles per workgroup (compile-time and run-time instances):
    element-wise within the fp32-summation bound of the fp64 reference, bitwise the
    default plan's output, and bitwise reproducible."""
    shape, cus, tm, _ = case
    n, h, w, cin, cout = shape
    _pin_tm(monkeypatch, tm)
    plan_cus(cus)
    _c3_plan(case)
    d = _c3_data(shape)
    y = _ops().conv3x3(d["x"], d["wt"], n, h, w, cin, cout)
    y2 = _ops().conv3x3(d["x"], d["wt"], n, h, w, cin, cout)
    plan_cus(0)
    y0 = _ops().conv3x3(d["x"], d["wt"], n, h, w, cin, cout)
    _check_elementwise("conv3x3 fwd " + _c3_id(case), y.reshape(-1, cout), d["ref"].reshape(-1, cout),
                       d["amp"].reshape(-1, cout), 9 * cin)
    assert torch.equal(y, y2), "two runs differ"
    assert torch.equal(y, y0), f"differs from the default plan at {int((y != y0).sum())} elements"


@gpu
@pytest.mark.parametrize("case", C3_DGRAD, ids=_c3_id)
def test_conv3x3_dgrad_multi_tile(case, plan_cus, monkeypatch):
    """The input gradient (FLIP: transposed LDS reads of the forward weight) over several
    tiles per workgroup, as the forward."""
    shape, cus, tm, _ = case
    n, h, w, cin, cout = shape
    _pin_tm(monkeypatch, tm)
    plan_cus(cus)
    _c3_plan(case, flip=True)
    wt, d = _c3_data(shape)["wt"], _c3_dgrad_data(shape)
    dx = _ops().conv3x3(d["dy"], wt, n, h, w, cout, cin, True)
    dx2 = _ops().conv3x3(d["dy"], wt, n, h, w, cout, cin, True)
    plan_cus(0)
    dx0 = _ops().conv3x3(d["dy"], wt, n, h, w, cout, cin, True)
    _check_elementwise("conv3x3 dgrad " + _c3_id(case), dx.reshape(-1, cin), d["ref"].reshape(-1, cin),
                       d["amp"].reshape(-1, cin), 9 * cout)
    assert torch.equal(dx, dx2), "two runs differ"
    assert torch.equal(dx, dx0), f"differs from the default plan at {int((dx != dx0).sum())} elements"


@gpu
@pytest.mark.parametrize("case", C3_CASES, ids=_c3_id)
def test_conv3x3_stats_rows_multi_tile(case, plan_cus, monkeypatch):
    """The statistics forward (ST): y as the plain forward's, and EVERY partial row equal to
    the fp64 sums of the kernel's bf16 y over that workgroup's own pixel range (the total
    alone would hide a tile counted in the wrong row)."""
    shape, cus, tm, _ = case
    n, h, w, cin, cout = shape
    _pin_tm(monkeypatch, tm)
    plan_cus(cus)
    wpb, ranges = _c3_plan(case, stats=True)
    d = _c3_data(shape)
    y, part = _ops().conv3x3_stats(d["x"], d["wt"], n, h, w, cin, cout)
    y2, part2 = _ops().conv3x3_stats(d["x"], d["wt"], n, h, w, cin, cout)
    plan_cus(0)
    y0 = _ops().conv3x3(d["x"], d["wt"], n, h, w, cin, cout)
    assert part.shape == (wpb, 2, cout)
    _check_elementwise("conv3x3 stats " + _c3_id(case), y.reshape(-1, cout), d["ref"].reshape(-1, cout),
                       d["amp"].reshape(-1, cout), 9 * cin)
    assert torch.equal(y, y0), f"differs from the default plan's forward at {int((y != y0).sum())} elements"
    yd = y.double().reshape(-1, cout)
    _check_rows("conv3x3 stats " + _c3_id(case), part, (yd, yd * yd), ranges)
    assert torch.equal(y, y2) and torch.equal(part, part2), "two runs differ"


@gpu
@pytest.mark.parametrize("case", C3_PRE, ids=_c3_id)
def test_conv3x3_pre_multi_tile(case, plan_cus, monkeypatch):
    """A deferred BatchNorm + ReLU staged by the statistics forward (PRE, always a run-time
    instance) on up to 7 halo pieces per thread: y and the partial rows bitwise those of
    the kernel on the materialised activation, y within the bound of the fp64 convolution
    of that activation, num_batches_tracked incremented once."""
    shape, cus, tm, _ = case
    n, h, w, cin, cout = shape
    _pin_tm(monkeypatch, tm)
    plan_cus(cus)
    wpb, ranges = _c3_plan(case, stats=True, pre=True)
    d, p = _c3_data(shape), _c3_pre_data(shape)
    nbt = torch.zeros((), dtype=torch.int64, device=_dev())
    y1, p1 = _ops().conv3x3_stats(d["x"], d["wt"], n, h, w, cin, cout, p["st"], nbt)
    y0, p0 = _ops().conv3x3_stats(p["a"], d["wt"], n, h, w, cin, cout)
    assert int(nbt) == 1
    assert p1.shape == (wpb, 2, cout)
    _check_elementwise("conv3x3 pre " + _c3_id(case), y1.reshape(-1, cout), p["ref"].reshape(-1, cout),
                       p["amp"].reshape(-1, cout), 9 * cin)
    assert torch.equal(y1, y0), f"PRE differs from the materialised run at {int((y1 != y0).sum())} elements"
    assert torch.equal(p1, p0)
    yd = y1.double().reshape(-1, cout)
    _check_rows("conv3x3 pre " + _c3_id(case), p1, (yd, yd * yd), ranges)


# ------------------------------------------------------------------------------ 1x1
# (M, K, N) at 4 plan CUs (want = 8 pixel ranges) and the expected
# (tnw, gy, gx, tiles_per_blk, variant): every launch variant -- weights resident beside
# 6 / 4 x stages (0 / 1) and streamed (2), 64- and 32-channel wave columns, K = 32.
# M % 128 != 0; mt = 50 / 9 leave the last non-empty range one tile (and at mt = 9 three
# all-padding rows of the XCD deal), mt = 18 fills 6 ranges and leaves 2 padding rows.
C1_CUS = 4
C1_CASES = [
    ((6349, 64, 256), (2, 2, 8, 7, 0)),
    ((6349, 256, 64), (1, 1, 8, 7, 1)),
    ((1101, 1024, 192), (1, 3, 8, 2, 2)),
    ((1101, 128, 512), (2, 4, 8, 2, 1)),
    ((2300, 512, 2048), (2, 16, 8, 3, 2)),
    ((1101, 32, 64), (1, 1, 8, 2, 0)),
]
C1_BWD_CASES = [
    ((6349, 64, 256), (1, 4, 8, 7, 0)),
    ((1101, 128, 512), (1, 8, 8, 2, 0)),
    ((1101, 32, 192), (1, 3, 8, 2, 0)),
]


def _c1_id(case):
    return "x".join(map(str, case[0]))


def _c1_plan(case, bwd=False):
    """Asserts the case's plan; returns the partial rows' pixel ranges (empty: padding rows)."""
    (m, k, n), want = case
    plan = tuple(_ops().conv1x1_plan(m, k, n, bwd))
    assert plan == want, plan
    _, _, gx, tpb, _ = plan
    mt = (m + 127) // 128
    nonempty = -(-mt // tpb)
    assert tpb >= 2 and m % 128 != 0 and gx % 8 == 0 and nonempty <= gx
    # a shorter last range or all-padding rows (mt = 50: 1 tile left of 7; mt = 9: both)
    assert mt - (nonempty - 1) * tpb < tpb or nonempty < gx
    return [(min(m, bx * tpb * 128), min(m, (bx + 1) * tpb * 128)) for bx in range(gx)]


@functools.lru_cache(maxsize=None)
def _c1_data(shape):
    m, k, n = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(80 + sum(shape))
    x = torch.randn(m, k, generator=g).to(dev).to(torch.bfloat16)
    wb = (torch.randn(n, k, generator=g) / k ** 0.5).to(dev).to(torch.bfloat16)
    return {"x": x, "w": wb, "ref": x.double() @ wb.double().t(), "amp": x.double().abs() @ wb.double().abs().t()}


@gpu
@pytest.mark.parametrize("case", C1_CASES, ids=_c1_id)
def test_conv1x1_stats_multi_tile(case, plan_cus):
    """Several 128-pixel tiles per workgroup with a shorter last range and all-padding
    rows: y element-wise within the bound and bitwise the default plan's, each partial row
    the fp64 sums over its own pixel range, padding rows exactly zero, reproducible."""
    (m, k, n), _ = case
    plan_cus(C1_CUS)
    ranges = _c1_plan(case)
    d = _c1_data(case[0])
    y, part = _ops().conv1x1_stats(d["x"], d["w"])
    y2, part2 = _ops().conv1x1_stats(d["x"], d["w"])
    plan_cus(0)
    assert _ops().conv1x1_plan(m, k, n)[3] < case[1][3]  # the default plan is another partition
    y0, _ = _ops().conv1x1_stats(d["x"], d["w"])
    assert part.shape == (len(ranges), 2, n)
    _check_elementwise("conv1x1 " + _c1_id(case), y, d["ref"], d["amp"], k)
    assert torch.equal(y, y0), f"differs from the default plan at {int((y != y0).sum())} elements"
    yd = y.double()
    _check_rows("conv1x1 " + _c1_id(case), part, (yd, yd * yd), ranges)
    assert torch.equal(y, y2) and torch.equal(part, part2), "two runs differ"


@gpu
@pytest.mark.parametrize("case", [c for c in C1_CASES if c[0][1] <= 512], ids=_c1_id)
def test_conv1x1_pre_multi_tile(case, plan_cus):
    """PRE over several tiles per workgroup: y and the partial rows bitwise those of the
    kernel on the materialised activation, num_batches_tracked incremented once."""
    (m, k, n), _ = case
    assert _ops().conv1x1_pre_ok(m, k, n)
    plan_cus(C1_CUS)
    ranges = _c1_plan(case)
    d = _c1_data(case[0])
    st = _stats4(k, 90 + k)
    nbt = torch.zeros((), dtype=torch.int64, device=_dev())
    y1, p1 = _ops().conv1x1_stats(d["x"], d["w"], st, nbt)
    a = _apply(d["x"], st)
    y0, p0 = _ops().conv1x1_stats(a, d["w"])
    assert int(nbt) == 1
    assert torch.equal(y1, y0), f"PRE differs from the materialised run at {int((y1 != y0).sum())} elements"
    assert torch.equal(p1, p0)
    _check_elementwise("conv1x1 pre " + _c1_id(case), y1, a.double() @ d["w"].double().t(),
                       a.double().abs() @ d["w"].double().abs().t(), k)
    yd = y1.double()
    _check_rows("conv1x1 pre " + _c1_id(case), p1, (yd, yd * yd), ranges)


@gpu
@pytest.mark.parametrize("case", C1_BWD_CASES, ids=_c1_id)
def test_conv1x1_bn_bwd_multi_tile(case, plan_cus):
    """The fused input gradient + BatchNorm backward partial over several tiles per
    workgroup (two alternating prefetch register sets): d = bf16((bf16(dy1 . W) + dy2) *
    (yb > 0)) element-wise against r = (dy1 . W + dy2) * (yb > 0) in fp64, the partial
    rows (sums of d and d * xb) per row of the kernel's own d.

    Bound on d: with s the fp64 product and b1 = 2^-8 |s| + 2 K 2^-24 A the forward's
    bound on da = bf16(fp32 sum), t = fp32(da + dy2) is within b1 + 2^-24 |t| of s + dy2
    and d = bf16(t) adds 2^-8 |t|, |t| <= |r| + b1:  |d - r| <= b1 + (2^-8 + 2^-24)(|r| + b1);
    masked elements are exactly zero."""
    (m, k, n), _ = case
    assert _ops().conv1x1_bn_bwd_ok(m, k, n)
    plan_cus(C1_CUS)
    ranges = _c1_plan(case, bwd=True)
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(100 + m + k + n)
    dy1 = torch.randn(m, k, generator=g).to(dev).to(torch.bfloat16)
    w = (torch.randn(k, n, generator=g) / k ** 0.5).to(dev).to(torch.bfloat16)  # conv weight [Cout = k, Cin = n]
    dy2 = torch.randn(m, n, generator=g).to(dev).to(torch.bfloat16)
    yb = torch.randn(m, n, generator=g).to(dev).to(torch.bfloat16).clamp_min(0)  # a ReLU output (zeros included)
    xb = torch.randn(m, n, generator=g).to(dev).to(torch.bfloat16)
    wt = w.t().contiguous()
    d, part = _ops().conv1x1_bn_bwd(dy1, wt, dy2, yb, xb)
    d2, part2 = _ops().conv1x1_bn_bwd(dy1, wt, dy2, yb, xb)
    plan_cus(0)
    d0, _ = _ops().conv1x1_bn_bwd(dy1, wt, dy2, yb, xb)
    assert d.shape == (m, n) and d.dtype == torch.bfloat16 and part.shape == (len(ranges), 2, n)
    mask = (yb.double() > 0).double()
    s = dy1.double() @ w.double()
    amp = dy1.double().abs() @ w.double().abs()
    r = (s + dy2.double()) * mask
    b1 = (U8 * s.abs() + 2.0 * k * U24 * amp) * mask
    # _worst's own terms: 2^-8 |r| + 2 K 2^-24 (A mask); the rest of the derivation as `extra`
    extra = U8 * s.abs() * mask + (U8 + U24) * b1 + U24 * r.abs()
    _check_elementwise("conv1x1 bn_bwd " + _c1_id(case), d, r, amp * mask, k, extra)
    assert bool((d[mask == 0] == 0).all())
    assert torch.equal(d, d0), f"differs from the default plan at {int((d != d0).sum())} elements"
    dd = d.double()
    _check_rows("conv1x1 bn_bwd " + _c1_id(case), part, (dd, dd * xb.double()), ranges)
    assert torch.equal(d, d2) and torch.equal(part, part2), "two runs differ"


# ------------------------------------------------------------------------------ stem
def stem_ref(x, wt):
    """fp64 y[n][oh][ow][co] = sum x[n][2 oh - 3 + r][2 ow - 3 + s][c] wt[co][r][s][c] (NHWC)."""
    n, h, w, _ = x.shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = F.pad(x.double(), (0, 0, 3, 3, 3, 3))
    wd = wt.double()
    out = torch.zeros(n, oh, ow, 64, dtype=torch.float64, device=x.device)
    for r in range(7):
        for s in range(7):
            out += xp[:, r:r + 2 * oh - 1:2, s:s + 2 * ow - 1:2, :] @ wd[:, r, s, :].t()
    return out


# ((N, H, W), plan CUs, tiles (2 output rows of one image) per workgroup)
STEM_CASES = [
    ((2, 224, 224), 4, [28, 28, 28, 28]),  # production's 28 tiles per workgroup
    ((3, 32, 32), 4, [6, 6, 6, 6]),
    ((2, 30, 46), 4, [4, 4, 4, 4]),        # odd OH: each image's last tile is one row
    ((1, 17, 20), 2, [2, 3]),
]


def _stem_id(case):
    return "x".join(map(str, case[0])) + f"-cu{case[1]}"


def _stem_plan(case):
    """Asserts the grid and the tiles per workgroup; returns the partial rows' pixel ranges."""
    (n, h, w), cus, tiles = case
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    grid = _ops().stem_grid(n, h, w)
    ohp = (oh + 1) // 2
    ntile = n * ohp
    cuts = [ntile * b // grid for b in range(grid + 1)]
    assert grid == cus and [b - a for a, b in zip(cuts, cuts[1:])] == tiles and min(tiles) >= 2, (grid, cuts)

    def first_pixel(t):  # of tile t = (image t // ohp, output rows 2 (t % ohp) .. + 2)
        return ((t // ohp) * oh + min(2 * (t % ohp), oh)) * ow if t < ntile else n * oh * ow

    return [(first_pixel(a), first_pixel(b)) for a, b in zip(cuts, cuts[1:])]


@functools.lru_cache(maxsize=None)
def _stem_data(shape):
    n, h, w = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(120 + sum(shape))
    x = torch.randn(n, h, w, 3, generator=g).to(dev).to(torch.bfloat16)
    wt = (torch.randn(64, 7, 7, 3, generator=g) / 12).to(dev).to(torch.bfloat16)
    return {"x": x, "wt": wt, "ref": stem_ref(x, wt), "amp": stem_ref(x.abs(), wt.abs())}


@gpu
@pytest.mark.parametrize("case", STEM_CASES, ids=_stem_id)
def test_stem_forward_stats_multi_tile(case, plan_cus):
    """The stem forward with statistics over many 2-row tiles per workgroup (uneven tile
    splits included): element-wise within the bound (K = 147), bitwise the default plan's
    output, every partial row the fp64 sums over its workgroup's own tiles, reproducible."""
    shape, cus, _ = case
    plan_cus(cus)
    ranges = _stem_plan(case)
    d = _stem_data(shape)
    y, part = _ops().stem_fwd(d["x"], d["wt"], True)
    y2, part2 = _ops().stem_fwd(d["x"], d["wt"], True)
    (yp,) = _ops().stem_fwd(d["x"], d["wt"], False)
    plan_cus(0)
    assert _ops().stem_grid(*shape) > cus
    y0, _ = _ops().stem_fwd(d["x"], d["wt"], True)
    assert part.shape == (cus, 2, 64)
    _check_elementwise("stem " + _stem_id(case), y.reshape(-1, 64), d["ref"].reshape(-1, 64),
                       d["amp"].reshape(-1, 64), 147)
    assert torch.equal(y, y0), f"differs from the default plan at {int((y != y0).sum())} elements"
    assert torch.equal(y, yp), "the plain forward differs from the statistics forward"
    yd = y.double().reshape(-1, 64)
    _check_rows("stem " + _stem_id(case), part, (yd, yd * yd), ranges)
    assert torch.equal(y, y2) and torch.equal(part, part2), "two runs differ"


@gpu
@pytest.mark.parametrize("case", STEM_CASES, ids=_stem_id)
def test_stem_wgrad_multi_tile(case, plan_cus):
    """Stem weight gradient with every workgroup accumulating over many tiles, against
    fp32 autograd of the same bf16 operands (test_stem_wgrad_matches_fp32's reference and
    tolerance)."""
    from ray_lightning_accelerators_amd.ops.conv import stem_wgrad_hip

    (n, h, w), cus, _ = case
    plan_cus(cus)
    _stem_plan(case)
    torch.manual_seed(6)
    dev = _dev()
    x = torch.randn(n, 3, h, w, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = torch.randn(n, 64, oh, ow, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dw = stem_wgrad_hip(x, dy)
    dw2 = stem_wgrad_hip(x, dy)
    plan_cus(0)
    w32 = torch.zeros(64, 3, 7, 7, device=dev, requires_grad=True)
    F.conv2d(x.float(), w32, stride=2, padding=3).backward(dy.float())
    assert dw.shape == (64, 3, 7, 7) and dw.dtype == torch.float32
    rel = float((dw - w32.grad).norm() / w32.grad.norm().clamp_min(1e-30))
    print(f"[rel] stem wgrad {_stem_id(case)}: {rel:.3e}")
    assert rel < 1e-4, rel
    assert torch.equal(dw, dw2), "two runs differ"
