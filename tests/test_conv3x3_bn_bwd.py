"""The 3x3 input gradient with the preceding BatchNorm + ReLU's backward in its epilogue
(csrc/conv3x3.hip BWD, binding ``conv3x3_dgrad_bn``), at the production work split.

The planning CU count and the tile size are pinned as in tests/test_conv_partition.py, so
a small tensor gives each workgroup several tiles (asserted from ``conv3x3_dgrad_bn_plan``,
with the instance the case is there for):
the per-lane sums are then carried in registers across tiles, ranges end in shorter tiles
and tiles cross images.

Checks, per case:
  * ``d`` is BITWISE ``where(mask, dx_plain, 0)``: ``dx_plain`` from the plain input
    gradient kernel (``conv3x3(..., flip=True)``), ``mask = x * scale + shift > 0`` in
    fp64 (the sign of the fp32 fused multiply-add except at fp32 underflow);
  * every row of ``part`` against fp64 sums of the kernel's own ``d`` and ``d * xb`` over
    exactly that row's pixel range, within ``n 2^-24 sum|term|`` (fp32 summation of n
    terms; an empty range must be exactly zero);
  * two runs are bitwise equal (``d`` and ``part``), and ``d`` is bitwise the default
    plan's (the mask and the MFMA order of a pixel do not depend on the work split).
"""
import functools

import pytest
import torch

gpu = pytest.mark.gpu

U24 = 2.0 ** -24


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


# (shape (N, H, W, Cin, Cout) of the FORWARD layer, plan CUs, pinned tile size or None (auto),
#  expected (tile size, NX of the instance, compile-time-shape instance, most tiles per workgroup)):
# the input gradient reads dy [N, H, W, Cout] and writes d [N, H, W, Cin]; Cin is the
# BatchNorm's channel count.  Together the cases run all thirteen instances: the five
# compile-time shapes, and NX 4..7 at 256- and at 512-pixel tiles at run-time shape (the
# 6- and 7-piece 512-pixel ones and the 56x56 one have one register stage).
CASES = [
    ((2, 56, 56, 64, 64), 4, None, (512, 7, True, 4)),     # ResNet 56x56 shape
    ((2, 28, 28, 128, 128), 4, 256, (256, 4, True, 4)),    # ResNet 28x28 shape
    ((4, 14, 14, 256, 256), 8, None, (256, 4, True, 2)),   # ResNet 14x14 shape
    ((6, 7, 7, 512, 512), 8, 256, (256, 4, True, 2)),      # tiles that cross images
    ((7, 11, 13, 64, 48), 1, 256, (256, 4, False, 4)),     # non-ResNet shape
    ((7, 11, 13, 64, 48), 2, 256, (256, 4, False, 2)),     # fractional range edges
    ((3, 33, 20, 128, 32), 2, 512, (512, 6, False, 4)),    # wpb 1, two channel blocks
    # the remaining instances
    ((3, 56, 56, 64, 64), 4, 512, (512, 7, True, 5)),      # 56x56 at 7 pieces
    ((2, 28, 28, 128, 128), 4, None, (512, 5, True, 2)),   # 28x28 at 512-pixel tiles
    ((2, 28, 28, 64, 16), 2, None, (512, 5, False, 2)),
    ((3, 30, 61, 64, 16), 2, 512, (512, 7, False, 6)),
    ((2, 14, 14, 64, 16), 1, 512, (512, 4, False, 1)),     # (a range shorter than the tile: the only way to 4 pieces)
    ((3, 30, 61, 64, 16), 2, 256, (256, 5, False, 11)),
    ((1, 10, 140, 64, 16), 1, 256, (256, 6, False, 6)),
    ((1, 10, 170, 64, 16), 1, 256, (256, 7, False, 7)),
]


def _id(case):
    shape, cus, tm, _ = case
    return "x".join(map(str, shape)) + f"-cu{cus}-tm{tm or 'auto'}"


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Operands of a shape, made once and never written again."""
    n, h, w, cin, cout = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(90 + sum(shape))
    dy = torch.randn(n, h, w, cout, generator=g).to(dev).to(torch.bfloat16)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev).to(torch.bfloat16)
    xb = torch.randn(n, h, w, cin, generator=g).to(dev).to(torch.bfloat16)
    st = _stats4(cin, 70 + sum(shape))
    mask = (xb.double() * st[2].double() + st[3].double()) > 0
    return {"dy": dy, "wt": wt, "xb": xb, "st": st, "mask": mask}


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_conv3x3_dgrad_bn_multi_tile(case, plan_cus, monkeypatch):
    shape, cus, tm, (want_tm, want_nx, want_fixed, want_tiles) = case
    n, h, w, cin, cout = shape
    m = _ops()
    _pin_tm(monkeypatch, tm)
    plan_cus(cus)
    assert m.conv3x3_dgrad_bn_ok(n, h, w, cout, cin)
    p_tm, wpb, _, pieces, nx, fixed = m.conv3x3_dgrad_bn_plan(n, h, w, cout, cin)
    # the plain input gradient's work split and instance choice (its plan query)
    assert [p_tm, wpb, pieces, nx, fixed] == [m.conv3x3_plan(n, h, w, cout, cin, True)[i] for i in (0, 1, 3, 4, 5)]
    assert (p_tm, nx, bool(fixed)) == (want_tm, want_nx, want_fixed), (p_tm, pieces, nx, fixed)
    px = n * h * w
    ranges = [(px * j // wpb, px * (j + 1) // wpb) for j in range(wpb)]
    tiles = max(-((lo - hi) // p_tm) for lo, hi in ranges)
    assert tiles == want_tiles, f"{tiles} tiles per workgroup: {ranges} at {p_tm}"
    d_ = _data(shape)
    d, part = m.conv3x3_dgrad_bn(d_["dy"], d_["wt"], n, h, w, cout, cin, d_["xb"], d_["st"])
    d2, part2 = m.conv3x3_dgrad_bn(d_["dy"], d_["wt"], n, h, w, cout, cin, d_["xb"], d_["st"])
    dx_plain = m.conv3x3(d_["dy"], d_["wt"], n, h, w, cout, cin, True)
    plan_cus(0)
    d0, _ = m.conv3x3_dgrad_bn(d_["dy"], d_["wt"], n, h, w, cout, cin, d_["xb"], d_["st"])
    assert d.shape == (n, h, w, cin) and d.dtype == torch.bfloat16 and tuple(part.shape) == (wpb, 2, cin)
    want = torch.where(d_["mask"], dx_plain, torch.zeros_like(dx_plain))
    diff = d.view(torch.int16) != want.view(torch.int16)
    assert not bool(diff.any()), f"d differs from the masked plain gradient at {int(diff.sum())} of {d.numel()} elements"
    assert 0.2 < float(d_["mask"].double().mean()) < 0.8  # the mask clips, and not everything
    dd = d.double().reshape(px, cin)
    _check_rows("dgrad_bn " + _id(case), part, (dd, dd * d_["xb"].double().reshape(px, cin)), ranges)
    assert torch.equal(d.view(torch.int16), d2.view(torch.int16)) and torch.equal(part, part2), "two runs differ"
    assert torch.equal(d.view(torch.int16), d0.view(torch.int16)), \
        f"differs from the default plan at {int((d.view(torch.int16) != d0.view(torch.int16)).sum())} elements"


@gpu
def test_conv3x3_dgrad_bn_refuses_what_it_does_not_cover():
    m = _ops()
    assert not m.conv3x3_dgrad_bn_ok(2, 8, 8, 64, 1024)  # the coefficient table limit (as conv3x3 PRE's)
    assert not m.conv3x3_dgrad_bn_ok(2, 8, 8, 64, 96)    # Co % 64
    assert m.conv3x3_dgrad_bn_ok(2, 8, 8, 64, 64)
    d_ = _data((2, 8, 8, 64, 64))
    with pytest.raises(RuntimeError):
        m.conv3x3_dgrad_bn(d_["dy"], d_["wt"], 2, 8, 8, 64, 64, d_["xb"], d_["st"][:, :32].contiguous())
    # the plain plan query keeps refusing statistics on the input gradient
    with pytest.raises(RuntimeError):
        m.conv3x3_plan(2, 8, 8, 64, 64, True, True)
