"""The 3x3 / stride 2 / pad 1 MFMA forward (csrc/conv3x3s2.hip) from the kernel up to
``_ConvNHWCFn``: ResNet-50's downsample conv2 layers.

Kernel checks, on the raw bindings (NHWC memory):
  * against fp32 ``F.conv2d`` of the same bf16 operands, ``tests/test_conv3x3.py``'s two
    bounds for a bf16-rounded output (relative norm error < 8e-3, max error < 5 % of the
    largest reference value);
  * element-wise against fp64, ``tests/test_conv_partition.py``'s derived bound unchanged:
    ``|y - ref| <= 2^-8 |ref| + 2 K 2^-24 A`` with K = 9 Cin and A the fp64 stride-2
    convolution of |x| with |w|;
  * the statistics variant's y bitwise the plain variant's, every ``part`` row the fp64
    sums of the kernel's own bf16 output over exactly that workgroup's pixel range
    (from ``conv3x3s2_plan``) within ``n 2^-24 sum|term|``, an empty row exactly zero;
  * at a pinned planning CU count (several tiles per workgroup with a shorter last one):
    y bitwise the default plan's, the rows as above, two runs bitwise equal;
  * the kernel's largest ResNet halo (a full tile of the 56x56 layer across an image
    boundary, which unaligned batch sizes such as 24 produce) is run, and the three
    ResNet layers are taken at every batch size 1..256; the predicate follows a changed
    planning CU count.
The shapes: ResNet's three layers at small batch, the 4x4 image the 64x64-image ResNet
test produces, odd H and W (the bottom / right padding is read, tiles cross images,
Cin % 64 != 0), one reduction chunk, two channel blocks on a 2x2 output, and images
where only the centre tap (1x1) or four taps (2x2) are inside.  Each test prints its
worst error / bound ratio; measured on an MI355X: element-wise 0.31-0.96 (the bf16
rounding term; worst at 2x5x9x16x64), partial rows under 0.31 of their tolerance,
relative norm error against fp32 1.4e-3 - 1.8e-3.

Dispatch checks: the candidate tables ``_ConvNHWCFn`` builds for the layer, every
in-tree forward candidate forced in turn against the all-MIOpen run, deterministic
mode, refused shapes, a downsample ``Bottleneck`` with and without the epilogue
statistics, and the CPU guard.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import conv as C

gpu = pytest.mark.gpu

U24 = 2.0 ** -24
U8 = 2.0 ** -8

SHAPES = [
    (2, 56, 56, 128, 128), (2, 28, 28, 256, 256), (3, 14, 14, 512, 512),  # ResNet's three layers
    (2, 4, 4, 512, 512),                                                  # layer4 of a 64x64 image
    (3, 7, 7, 64, 64), (7, 11, 13, 48, 64),                               # odd H, W
    (2, 5, 9, 16, 64), (1, 3, 3, 32, 128),                                # one chunk; two channel blocks, 2x2 output
    (1, 1, 1, 64, 64), (1, 2, 2, 16, 64),                                 # centre tap only; four taps
]
# (shape, plan CUs): every workgroup gets at least three 128-pixel tiles and a shorter last one
SPLIT_CASES = [
    ((2, 56, 56, 128, 128), 8),   # 4 ranges of 392 output pixels per channel block
    ((2, 28, 28, 256, 256), 4),   # one range of 392
    ((9, 14, 14, 512, 512), 8),   # one range of 441: 7x7 outputs, every tile crosses images
    ((7, 11, 13, 48, 64), 1),     # odd sizes, one range of 294
]
# (shape, plan CUs): a full 128-pixel tile of a 56x56 input that starts in the last output
# row of one image at column >= 13 and runs into the next: 14 virtual halo rows x 57 = 798
# entries, the kernel's largest ResNet halo (7 pieces per thread).  The first is one range
# of three images (its tile at pixel 1536 starts at row 26, column 24 of the second); the
# second is batch 24 on 256 CUs, a batch size whose partition has such tiles
CROSSING_CASES = [
    ((3, 56, 56, 128, 128), 2),
    ((24, 56, 56, 128, 128), 256),
]
# refused by the predicate: Cout % 64 != 0, and a row too wide for the kernel's LDS halo
# image (three halo rows of 2 * 300 + 1 entries against 896)
REFUSED = [((4, 64, 8, 8), 24), ((1, 64, 4, 600), 64)]


def _ops():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


def _dev():
    return torch.device("cuda", 0)


def _id(shape):
    return "x".join(map(str, shape))


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


@pytest.fixture
def plan_cus():
    """``pin(k)`` plans for k CUs (0: the device's); the device value is restored whatever
    the test does."""
    m = _ops()

    def pin(k):
        m.set_plan_cus(k)

    try:
        yield pin
    finally:
        m.set_plan_cus(0)


def s2_ref(x, wt):
    """fp64 y[n][oh][ow][co] = sum x[n][2 oh + r - 1][2 ow + s - 1][ci] wt[co][r][s][ci] (NHWC)."""
    n, h, w, _ = x.shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    wd = wt.double()
    out = torch.zeros(n, oh, ow, wt.size(0), dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            out += xp[:, r:r + 2 * oh - 1:2, s:s + 2 * ow - 1:2, :] @ wd[:, r, s, :].t()
    return out


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Operands (NHWC memory) and fp64 references of a shape, computed once and never written again."""
    n, h, w, cin, cout = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(300 + sum(shape))
    x = torch.randn(n, h, w, cin, generator=g).to(dev).to(torch.bfloat16)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev).to(torch.bfloat16)
    return {"x": x, "wt": wt, "ref": s2_ref(x, wt), "amp": s2_ref(x.abs(), wt.abs())}


def _check_elementwise(tag, y, ref, amp, k):
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert bool(torch.isfinite(y.float()).all()), f"{tag}: non-finite output"
    err = (y.double() - ref).abs()
    bound = U8 * ref.abs() + 2.0 * k * U24 * amp
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst, nbad = float(ratio.max()), int((ratio > 1.0).sum())
    print(f"[bound ratio] {tag}: worst {worst:.3f}")
    assert nbad == 0, f"{tag}: {nbad} of {ref.numel()} elements past the bound, worst {worst:.3f}"


def _check_rows(tag, part, y, ranges):
    """part [rows, 2, C] fp32 against the fp64 sums of y [M, C] (fp64 of the kernel's bf16
    output) and y^2 over each row's pixel range, within n 2^-24 sum|term|."""
    assert part.dtype == torch.float32 and part.size(0) == len(ranges), (part.shape, len(ranges))
    worst = 0.0
    for j, (lo, hi) in enumerate(ranges):
        for s, terms in enumerate((y, y * y)):
            got = part[j, s].double()
            if hi <= lo:
                assert bool((got == 0).all()), f"{tag}: empty row {j} stat {s} is not zero"
                continue
            t = terms[lo:hi]
            want, tol = t.sum(0), (hi - lo) * U24 * t.abs().sum(0)
            err = (got - want).abs()
            bad = err > tol
            assert not bool(bad.any()), f"{tag}: row {j} (pixels {lo}..{hi}) stat {s}: {int(bad.sum())} channels " \
                                        f"off, worst |err| {float(err.max()):.3e}"
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
    print(f"[row ratio] {tag}: worst {worst:.3f}")


def _plan(shape, stats=False):
    """(tm, wpb, the part rows' output-pixel ranges, compile-time instance) of the current plan."""
    n, h, w, cin, cout = shape
    tm, wpb, _, pieces, nx, fixed, oh, ow = _ops().conv3x3s2_plan(n, h, w, cin, cout, stats)
    assert (oh, ow) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1) and pieces <= nx
    m = n * oh * ow
    return tm, wpb, [(m * j // wpb, m * (j + 1) // wpb) for j in range(wpb)], bool(fixed)


# ------------------------------------------------------------------------------ kernel
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_forward_matches_fp32(shape):
    """``conv3x3s2_hip`` against fp32 ``F.conv2d`` of the same bf16 operands."""
    n, h, w, cin, cout = shape
    d = _data(shape)
    x, wb = d["x"].permute(0, 3, 1, 2), d["wt"].permute(0, 3, 1, 2)
    assert C.conv3x3s2_ok(x, wb, (2, 2), (1, 1))
    y = C.conv3x3s2_hip(x, wb)
    ref = F.conv2d(x.float(), wb.float(), stride=2, padding=1)
    assert y.shape == ref.shape == (n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    rel, mx = _rel(y, ref), float((y.float() - ref).abs().max())
    print(f"[rel] conv3x3s2 {_id(shape)}: {rel:.3e}, max |err| {mx:.3e} of {float(ref.abs().max()):.3e}")
    assert rel < 8e-3, rel
    assert mx < 0.05 * float(ref.abs().max()), mx


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_forward_elementwise_fp64(shape):
    """No element past ``2^-8 |ref| + 2 K 2^-24 A`` of the fp64 reference (K = 9 Cin)."""
    n, h, w, cin, cout = shape
    d = _data(shape)
    y = _ops().conv3x3s2(d["x"], d["wt"], n, h, w, cin, cout)
    assert y.dtype == torch.bfloat16 and y.shape == d["ref"].shape
    _check_elementwise("conv3x3s2 " + _id(shape), y.reshape(-1, cout), d["ref"].reshape(-1, cout),
                       d["amp"].reshape(-1, cout), 9 * cin)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_stats_rows(shape):
    """The statistics variant: y bitwise the plain variant's, every partial row the fp64
    sums of the kernel's bf16 y over that workgroup's own pixel range."""
    n, h, w, cin, cout = shape
    d = _data(shape)
    x, wb = d["x"].permute(0, 3, 1, 2), d["wt"].permute(0, 3, 1, 2)
    _, wpb, ranges, _ = _plan(shape, stats=True)
    y0 = C.conv3x3s2_hip(x, wb)
    y, part = C.conv3x3s2_stats_hip(x, wb)
    assert torch.equal(y, y0), f"differs from the plain forward at {int((y != y0).sum())} elements"
    assert y.is_contiguous(memory_format=torch.channels_last) and part.shape == (wpb, 2, cout)
    _check_rows("conv3x3s2 stats " + _id(shape), part, y.permute(0, 2, 3, 1).double().reshape(-1, cout), ranges)


@gpu
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: _id(c[0]) + f"-cu{c[1]}")
def test_production_split(case, plan_cus):
    """Several tiles per workgroup with a shorter last one (the per-workgroup geometry of a
    full-size layer): y element-wise within the bound and bitwise the default plan's, the
    rows over their own ranges, two runs bitwise equal."""
    shape, cus = case
    n, h, w, cin, cout = shape
    m = _ops()
    d = _data(shape)
    plan_cus(cus)
    tm, wpb, ranges, fixed = _plan(shape, stats=True)
    assert wpb == max(1, cus // (cout // 64)), wpb
    for lo, hi in ranges:
        assert -((lo - hi) // tm) >= 3 and (hi - lo) % tm != 0, (lo, hi, tm)
    # the kernel has one instance, shapes at run time: that is the one under test at ResNet's widths too
    assert not fixed and _plan(shape)[3] == fixed
    y, part = m.conv3x3s2_stats(d["x"], d["wt"], n, h, w, cin, cout)
    y2, part2 = m.conv3x3s2_stats(d["x"], d["wt"], n, h, w, cin, cout)
    yp = m.conv3x3s2(d["x"], d["wt"], n, h, w, cin, cout)
    plan_cus(0)
    assert _plan(shape)[1] != wpb  # the default plan is another partition
    y0 = m.conv3x3s2(d["x"], d["wt"], n, h, w, cin, cout)
    tag = f"conv3x3s2 split {_id(shape)}-cu{cus}"
    _check_elementwise(tag, y.reshape(-1, cout), d["ref"].reshape(-1, cout), d["amp"].reshape(-1, cout), 9 * cin)
    assert torch.equal(y, y0), f"differs from the default plan at {int((y != y0).sum())} elements"
    assert torch.equal(yp, y0), "the plain variant differs from the default plan"
    assert part.shape == (wpb, 2, cout)
    _check_rows(tag, part, y.double().reshape(-1, cout), ranges)
    assert torch.equal(y, y2) and torch.equal(part, part2), "two runs differ"


@gpu
@pytest.mark.parametrize("case", CROSSING_CASES, ids=lambda c: _id(c[0]) + f"-cu{c[1]}")
def test_image_crossing_full_tile(case, plan_cus):
    """The largest halo of the 56x56 layer (a full tile across an image boundary: 14 halo
    rows, 7 pieces per thread) is taken, not refused: element-wise within the bound, the
    statistics rows over their own ranges, the plain variant bitwise equal."""
    shape, cus = case
    n, h, w, cin, cout = shape
    m = _ops()
    plan_cus(cus)
    assert m.conv3x3s2_supported(n, h, w, cin, cout)
    vrows, pieces, nx = m.conv3x3s2_plan(n, h, w, cin, cout, True)[2:5]
    assert (vrows, pieces, nx) == (14, 7, 7), (vrows, pieces, nx)
    _, wpb, ranges, _ = _plan(shape, stats=True)
    d = _data(shape)
    y, part = m.conv3x3s2_stats(d["x"], d["wt"], n, h, w, cin, cout)
    yp = m.conv3x3s2(d["x"], d["wt"], n, h, w, cin, cout)
    tag = f"conv3x3s2 crossing {_id(shape)}-cu{cus}"
    _check_elementwise(tag, y.reshape(-1, cout), d["ref"].reshape(-1, cout), d["amp"].reshape(-1, cout), 9 * cin)
    assert torch.equal(y, yp), "the plain variant differs"
    assert part.shape == (wpb, 2, cout)
    _check_rows(tag, part, y.double().reshape(-1, cout), ranges)


@gpu
def test_resnet_shapes_supported_at_every_batch(plan_cus):
    """The predicate follows the work split: ResNet's three layers are taken at every
    batch size 1..256 on 256 CUs (unaligned ones included), and the Python predicate
    answers for the plan in force, not for the one it first saw."""
    m = _ops()
    plan_cus(256)
    for h, c in ((56, 128), (28, 256), (14, 512)):
        bad = [n for n in range(1, 257) if not m.conv3x3s2_supported(n, h, h, c, c)]
        assert not bad, (h, c, bad)
    # (1, 8, 200): 4 x 100 output pixels; 13 ranges of ~30 pixels span two rows (5 x 201
    # halo entries, refused), 8 ranges of 50 stay in one (3 x 201, taken)
    x = torch.zeros(1, 64, 8, 200, device=_dev(), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wb = torch.zeros(64, 64, 3, 3, device=_dev(), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert not C.conv3x3s2_ok(x, wb, (2, 2), (1, 1))
    plan_cus(8)
    assert C.conv3x3s2_ok(x, wb, (2, 2), (1, 1))
    assert C.conv3x3s2_hip(x, wb).shape == (1, 64, 4, 100)
    plan_cus(256)
    assert not C.conv3x3s2_ok(x, wb, (2, 2), (1, 1))


# ------------------------------------------------------------------------------ dispatch
def _operands(shape, cout, device="cuda", seed=0):
    """x bf16 channels_last, the fp32 master weight, its bf16 copy and an output gradient."""
    g = torch.Generator().manual_seed(seed)
    n, cin, h, w = shape
    x = torch.randn(n, cin, h, w, generator=g).to(torch.bfloat16)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    dy = torch.randn(n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1, generator=g).to(torch.bfloat16)
    x, wt, dy = (t.to(device).contiguous(memory_format=torch.channels_last) for t in (x, wt, dy))
    return x, wt, wt.to(torch.bfloat16), dy


def _convs2(x, wt, wb, dy, bn_stats=None):
    x, wt = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = C._ConvNHWCFn.apply(x, wt, wb, (2, 2), (1, 1), None, bn_stats)
    y.backward(dy)
    return y.detach(), x.grad, wt.grad


def _autograd(x, wb, dy):
    """``F.conv2d``'s autograd on the bf16 weight; the weight gradient widened to fp32."""
    x, wb = x.clone().requires_grad_(True), wb.clone().requires_grad_(True)
    y = F.conv2d(x, wb, stride=2, padding=1)
    y.backward(dy)
    return y.detach(), x.grad, wb.grad.float()


@gpu
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "bn_stats"])
def test_dispatch_tables_and_candidates(monkeypatch, stats):
    """The layer's candidate tables, and every in-tree forward candidate forced in turn
    against the all-MIOpen run (test_conv_dispatch.py's bounds: 1e-2, input gradient 2e-2)."""
    ops = _operands((4, 64, 8, 8), 64)
    fwd = ("fwd_kxk_st", ("miopen", "hip_st")) if stats else ("fwd_kxk", ("miopen", "hip"))
    want, seen, keys = {}, {}, {}

    def pick(op, key, cands):
        seen[op] = tuple(cands)
        keys[op] = key
        return want.get(op, "miopen")

    monkeypatch.setattr(C, "_pick", pick)
    st = C.BNStats() if stats else None
    ref = _convs2(*ops, bn_stats=st)
    assert seen == dict([fwd, ("wgrad_kxk", ("miopen", "hip"))])
    assert keys[fwd[0]] == (4 * 8 * 8, 64, 64, 3, 3, 2, 1)
    assert st is None or st.part is None  # MIOpen ran: the BatchNorm makes its own pass
    for name in fwd[1][1:]:
        want[fwd[0]] = name
        st = C.BNStats() if stats else None
        got = _convs2(*ops, bn_stats=st)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert _rel(a, b) < (2e-2 if i == 1 else 1e-2), (name, i, _rel(a, b))
        if name == "hip_st":
            assert st.part is not None and st.part.shape[1:] == (2, 64) and st.part.dtype == torch.float32
            yd = got[0].permute(0, 2, 3, 1).double().reshape(-1, 64)
            torch.testing.assert_close(st.part.double().sum(0)[0], yd.sum(0), rtol=1e-4, atol=1e-2)


@gpu
def test_deterministic_mode_runs_plain_kernel(monkeypatch):
    """Under deterministic algorithms the forward is the in-tree plain kernel (nothing
    timed, no statistics hand-off) and two calls are bitwise equal."""
    x, wt, wb, _ = _operands((4, 64, 8, 8), 64)
    calls = {"hip": 0}
    real = C.conv3x3s2_hip

    def counted(*a):
        calls["hip"] += 1
        return real(*a)

    monkeypatch.setattr(C, "conv3x3s2_hip", counted)
    monkeypatch.delenv("RLA_CONV1X1", raising=False)
    before = dict(C._choice)
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        st = C.BNStats()
        y1 = C._ConvNHWCFn.apply(x, wt, wb, (2, 2), (1, 1), None, st)
        assert calls["hip"] == 1 and st.part is None
        y2 = C._ConvNHWCFn.apply(x, wt, wb, (2, 2), (1, 1), None, C.BNStats())
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    assert calls["hip"] == 2 and C._choice == before
    assert torch.equal(y1, y2)
    assert _rel(y1, F.conv2d(x.float(), wb.float(), stride=2, padding=1)) < 8e-3


@gpu
@pytest.mark.parametrize("shape,cout", REFUSED, ids=["cout24", "wide"])
def test_refused_shape_goes_to_miopen(monkeypatch, shape, cout):
    """A shape the predicate refuses consults no forward table and makes exactly the
    library calls of any strided layer.  Compared with ``F.conv2d``'s autograd (the same
    library entry points) within test_conv_dispatch.py's candidate bounds rather than
    bitwise: the library's own split reductions need not repeat bit for bit."""
    x, wt, wb, dy = _operands(shape, cout)
    assert not C.conv3x3s2_ok(x, wb, (2, 2), (1, 1))
    seen, calls = [], []

    def pick(op, key, cands):
        seen.append(op)
        return "miopen"

    monkeypatch.setattr(C, "_pick", pick)
    for name in ("_miopen_fwd", "_miopen_bwd"):
        def counting(*a, _name=name, _real=getattr(C, name)):
            calls.append(_name)
            return _real(*a)

        monkeypatch.setattr(C, name, counting)
    got = _convs2(x, wt, wb, dy, bn_stats=C.BNStats())
    assert seen == ["wgrad_kxk"] and calls == ["_miopen_fwd", "_miopen_bwd"]
    for i, (a, b) in enumerate(zip(got, _autograd(x, wb, dy))):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert _rel(a, b) < (2e-2 if i == 1 else 1e-2), (i, _rel(a, b))


@gpu
def test_downsample_block_bn2_uses_stats(monkeypatch):
    """A downsample bottleneck's stride-2 conv2 hands bn2 its epilogue statistics: output,
    gradients and bn2's running variance match the path where bn2 makes its own pass."""
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck, _bn, _conv1x1
    from ray_lightning_accelerators_amd.parallel.arena import ParamArena
    from torch import nn

    dev = _dev()
    calls = {"st": 0}
    real = C.conv3x3s2_stats_hip

    def st(*a, **k):
        calls["st"] += 1
        return real(*a, **k)

    monkeypatch.setattr(C, "conv3x3s2_stats_hip", st)
    monkeypatch.setenv("RLA_CONV1X1", "hip_st")  # pins the stats kernel in _pick (other ops: auto)
    outs = {}
    for mode in ("auto", "off"):
        monkeypatch.setenv("RLA_CONV3X3_STATS", mode)
        torch.manual_seed(0)
        down = nn.Sequential(_conv1x1(256, 512, 2, fused=True), _bn(512, True, act=None))
        blk = Bottleneck(256, 128, 2, down, fused_bn=True).to(dev).to(memory_format=torch.channels_last)
        arena = ParamArena(blk)
        arena.enable_bf16_shadow(blk)
        torch.manual_seed(1)
        x = torch.randn(4, 256, 16, 16, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = blk(x)
        y.float().square().mean().backward()
        outs[mode] = (y.detach().float(), x.grad.float(), blk.conv2.weight.grad.clone(), blk.bn2.running_var.clone())
        if mode == "auto":
            ran = calls["st"]
    assert ran >= 1 and calls["st"] == ran  # off: the epilogue statistics are not computed
    assert outs["auto"][0].shape == (4, 512, 8, 8)
    for a, b in zip(outs["auto"], outs["off"]):
        assert _rel(a, b.float()) < 2e-2, _rel(a, b.float())


# ------------------------------------------------------------------------------ CPU
def test_cpu_layer_stays_on_the_stock_path(monkeypatch):
    """On the CPU the predicate is false before the extension is touched: the layer equals
    ``F.conv2d``'s autograd exactly and sees no forward table."""
    x, wt, wb, dy = _operands((2, 64, 6, 5), 64, device="cpu")
    assert not C.conv3x3s2_ok(x, wb, (2, 2), (1, 1))
    seen = []

    def pick(op, key, cands):
        seen.append(op)
        return "miopen"

    monkeypatch.setattr(C, "_pick", pick)
    for a, b in zip(_convs2(x, wt, wb, dy), _autograd(x, wb, dy)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a, b), float((a.float() - b.float()).abs().max())
    assert seen == ["wgrad_kxk"]
