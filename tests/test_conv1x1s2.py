"""The MFMA 1x1 / stride-2 forward with BatchNorm statistics (csrc/conv1x1s2.hip) on the raw
bindings ``conv1x1s2`` / ``conv1x1s2_stats`` and through ``conv_nhwc``, element by element
against ``F.conv2d`` in float64 on the CPU.

  * integer operands (x in {-1, 0, 1}, w in {-2 .. 2}): every fp32 partial sum is exact, so y is
    the bf16 rounding of the float64 result bit for bit, and ``part`` added in float64 equals
    the sums of the ROUNDED y and of its square exactly (128 max y^2 < 2^24 is asserted);
  * bf16 ``randn`` operands: no element past 2^-8 |ref| (one bf16 rounding) plus
    Cin 2^-24 (|x| * |w|) (fp32 accumulation); ``part`` against float64 sums of the kernel's own
    y within 2 M 2^-24 sum |term| (tests/test_conv1x1_wide.py's statistics bound).
Worst error / bound ratio of the random cases on an MI355X: profiles/r24_conv1x1s2/test_ratios.log.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import conv as C

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout): one K-pair of stages and one partial tile (18 rows); odd H / W, 8
# stages, one partial tile; 147 rows = a full 128-row tile and a short one, two channel
# tiles; a single output pixel
SHAPES = [(2, 6, 6, 64, 128), (2, 7, 7, 256, 128), (3, 14, 14, 128, 256), (1, 2, 2, 64, 128)]


def _C():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


@functools.lru_cache(maxsize=None)
def _data(shape, kind):
    """NHWC x and [Cout, Cin] w on the device, the float64 NHWC result and |x| * |w|; made once."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    if kind == "int":
        x = torch.randint(-1, 2, (n, h, w, cin), generator=g).to(torch.bfloat16)
        wt = torch.randint(-2, 3, (cout, cin), generator=g).to(torch.bfloat16)
    else:
        x = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16)
        wt = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(torch.bfloat16)
    conv = lambda a, b: F.conv2d(a.double().permute(0, 3, 1, 2), b.double()[:, :, None, None], stride=2)
    ref, absdot = conv(x, wt).permute(0, 2, 3, 1), conv(x.abs(), wt.abs()).permute(0, 2, 3, 1)
    return x.cuda(), wt.cuda(), ref.contiguous(), absdot.contiguous()


def _check_part(part, y, exact):
    m = y.numel() // y.size(-1)
    assert part.shape == ((m + 127) // 128, 2, y.size(-1)) and part.dtype == torch.float32
    yd, s = y.double().cpu().flatten(0, 2), part.double().sum(0).cpu()
    for got, term in ((s[0], yd), (s[1], yd * yd)):
        tol = 0.0 if exact else 2 * m * 2.0 ** -24 * term.abs().sum(0)
        assert bool(((got - term.sum(0)).abs() <= tol).all())


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("shape", SHAPES)
def test_both_instances_match_fp64(shape, kind):
    n, h, w, cin, cout = shape
    x, wt, ref, absdot = _data(shape, kind)
    y0 = _C().conv1x1s2(x, wt)
    y, part = _C().conv1x1s2_stats(x, wt)
    assert y.shape == (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout) and y.dtype == torch.bfloat16
    assert torch.equal(y, y0)
    if kind == "int":
        assert 128 * float(ref.abs().max()) ** 2 < 2 ** 24
        assert torch.equal(y.cpu(), ref.to(torch.bfloat16))
    else:
        bound = 2.0 ** -8 * ref.abs() + cin * 2.0 ** -24 * absdot
        ratio = ((y.double().cpu() - ref).abs() / bound).max().item()
        print(f"conv1x1s2 {shape}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0
    _check_part(part, y, kind == "int")


@pytest.mark.parametrize("shape", SHAPES)
def test_skipped_pixels_never_read_and_reproducible(shape):
    x, wt, _, _ = _data(shape, "randn")
    y0, p0 = _C().conv1x1s2_stats(x, wt)
    y1, p1 = _C().conv1x1s2_stats(x, wt)
    assert torch.equal(y1, y0) and torch.equal(p1, p0)
    xn = x.clone()
    xn[:, 1::2] = float("nan")
    xn[:, :, 1::2] = float("nan")
    yn, pn = _C().conv1x1s2_stats(xn, wt)
    assert torch.equal(yn, y0) and torch.equal(pn, p0) and torch.equal(_C().conv1x1s2(xn, wt), y0)


@pytest.mark.parametrize("mode", ["hip", "deterministic", "miopen"])
def test_dispatch(monkeypatch, mode):
    n, h, w, cin, cout = SHAPES[1]
    xh, wt, _, _ = _data(SHAPES[1], "randn")
    x = xh.permute(0, 3, 1, 2).requires_grad_(True)
    conv = torch.nn.Conv2d(cin, cout, 1, 2, bias=False).cuda()
    wb = wt.view(cout, cin, 1, 1).contiguous(memory_format=torch.channels_last)
    monkeypatch.setenv("RLA_CONV1X1S2", "auto" if mode == "deterministic" else mode)
    before = dict(C._choice)
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(mode == "deterministic", warn_only=True)
    try:
        st = C.BNStats()
        y = C.conv_nhwc(x, conv, wb, bn_stats=st)
        y.float().sum().backward()
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert x.grad is not None and conv.weight.grad.shape == conv.weight.shape
    want, wpart = _C().conv1x1s2_stats(xh, wt)
    if mode == "miopen":
        assert not C.conv1x1s2_ok(x, wb, (2, 2), (0, 0)) and st.part is None
        assert torch.equal(y, C._miopen_fwd(x.detach(), wb, (2, 2), (0, 0)))
    else:
        # pinned: the statistics instance hands part over; deterministic: plain, BN's own pass
        assert torch.equal(y.permute(0, 2, 3, 1), want)
        assert (st.part is None) if mode == "deterministic" else torch.equal(st.part, wpart)
    assert {k for k in C._choice if k[0].startswith("fwd_1x1s2")} == {k for k in before if k[0].startswith("fwd_1x1s2")}


@pytest.mark.parametrize("case", ["cpu", "fp32", "nchw", "misaligned", "Cin=96", "stride1", "wb_cin"])
def test_refused_before_launch(case):
    n, h, w, cin, cout = 2, 6, 6, (96 if case == "Cin=96" else 64), 128
    assert _C().conv1x1s2_ok(n, h, w, cin, cout) == (case != "Cin=96")
    if case == "stride1":
        assert not _C().conv1x1s2_ok(n, h, w, cin, cout, 1, 1, 1, 1, 0, 0)
        return
    dev = "cpu" if case == "cpu" else "cuda"
    x = torch.zeros(n * h * w * cin + 8, device=dev, dtype=torch.float32 if case == "fp32" else torch.bfloat16)
    off = 4 if case == "misaligned" else 0
    x = x[off:off + n * h * w * cin]
    x = x.view(n, cin, h, w).permute(0, 2, 3, 1) if case == "nchw" else x.view(n, h, w, cin)
    wt = torch.zeros(cout, 128 if case == "wb_cin" else cin, device="cuda", dtype=torch.bfloat16)
    name = "conv1x1s2: w" if case == "wb_cin" else "unsupported shape" if case == "Cin=96" else "conv1x1s2: x"
    for fn in (_C().conv1x1s2, _C().conv1x1s2_stats):
        with pytest.raises(RuntimeError, match=name):
            fn(x, wt)
