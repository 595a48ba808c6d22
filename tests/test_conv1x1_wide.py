"""The wide-tile, fixed-order split-K 1x1 forward with BatchNorm statistics
(csrc/conv1x1_wide.hip) on the raw binding ``conv1x1_wide(x, w, bn, splits)``, every
instance forced in turn, element by element against float64.

  * integer operands (x in {-1, 0, 1}, w in {-2 .. 2}): every fp32 partial sum is exact in
    any order, so y must be the bf16 rounding of the float64 product bit for bit -- a
    dropped or doubled stage, slice, row or column cannot hide;
  * bf16 ``randn`` operands: no element past 2^-8 |ref| (the bf16 rounding) plus
    2 K 2^-24 (|x| . |w|^T) (the any-order fp32 dot-product bound, the project's factor 2);
  * the partial sums against float64 sums of the kernel's own y and y^2, within
    2 M 2^-24 sum |term|.
A plan the shape does not admit (bn not dividing N, slices on a persistent range) must raise.
The last shape runs with 4 planning CUs: several tiles per workgroup, carried statistics.

Worst error / bound ratio of the random cases, measured on an MI355X: 0.58 (K = 2048) to
0.96 (K = 256), the same for every instance of a shape -- the rounding term is tight by
construction, the summation term is far from reached.  The file takes about 5 s.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

PLANS = [(256, 1), (256, 2), (256, 4), (128, 1), (128, 2), (128, 4)]
# (M, K, N): one short tile with K shorter than ring depth x slices; a pixel tail with 5
# stages (unequal slices) and three 128-channel columns; a ResNet shape at batch 4; long K;
# many columns; a persistent range (4 planning CUs)
SHAPES = [(77, 256, 128), (300, 320, 384), (784, 1024, 256), (98, 2048, 512), (1000, 256, 1024), (3000, 512, 256)]
PLAN_CUS = {(3000, 512, 256): 4}


def _C():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


@functools.lru_cache(maxsize=None)
def _data(shape, kind):
    """Operands on the device, the float64 product and |x| . |w|^T; made once, never written."""
    m, k, n = shape
    g = torch.Generator().manual_seed(m + k + n)
    if kind == "int":
        x = torch.randint(-1, 2, (m, k), generator=g).to(torch.bfloat16)
        w = torch.randint(-2, 3, (n, k), generator=g).to(torch.bfloat16)
    else:
        x = torch.randn(m, k, generator=g).to(torch.bfloat16)
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
    x, w = x.cuda(), w.cuda()
    return x, w, x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()


def _bound(ref, absdot, k):
    return 2.0 ** -8 * ref.abs() + 2 * k * 2.0 ** -24 * absdot


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("plan", PLANS)
def test_every_instance_matches_fp64(plan, shape, kind):
    (bn, splits), (m, k, n) = plan, shape
    x, w, ref, absdot = _data(shape, kind)
    _C().set_plan_cus(PLAN_CUS.get(shape, 0))
    try:
        if shape in PLAN_CUS:
            p = _C().conv1x1_wide_plan(m, k, n)
            assert p[1] == 1 and p[3] > 1, p  # a persistent range, never sliced
        if n % bn != 0 or (splits > 1 and shape in PLAN_CUS):
            with pytest.raises(RuntimeError, match="does not admit"):
                _C().conv1x1_wide(x, w, bn, splits)
            return
        y, part = _C().conv1x1_wide(x, w, bn, splits)
    finally:
        _C().set_plan_cus(0)
    assert y.shape == (m, n) and y.dtype == torch.bfloat16
    assert part.dim() == 3 and part.shape[1:] == (2, n) and part.size(0) % 8 == 0 and part.dtype == torch.float32
    if kind == "int":
        assert torch.equal(y, ref.to(torch.bfloat16))
    else:
        ratio = ((y.double() - ref).abs() / _bound(ref, absdot, k)).max().item()
        print(f"conv1x1_wide bn={bn} splits={splits} {shape}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0
    yd, s = y.double(), part.double().sum(0)
    for got, term in ((s[0], yd), (s[1], yd * yd)):
        assert bool(((got - term.sum(0)).abs() <= 2 * m * 2.0 ** -24 * term.abs().sum(0)).all())


def test_split_is_bitwise_repeatable():
    """Four slices per tile, whoever arrives last: y and part never change from call to call
    (the binding hands every call freshly zeroed ticket counters)."""
    x, w, _, _ = _data((784, 1024, 256), "randn")
    y0, p0 = _C().conv1x1_wide(x, w, 0, 4)
    for _ in range(5):
        y, p = _C().conv1x1_wide(x, w, 0, 4)
        assert torch.equal(y, y0) and torch.equal(p, p0)


@pytest.mark.parametrize("case", ["K=128", "K=288", "N=64", "fp32", "misaligned"])
def test_refused_before_launch(case):
    m, k, n = {"K=128": (256, 128, 128), "K=288": (256, 288, 128), "N=64": (256, 256, 64)}.get(case, (256, 256, 128))
    x = torch.zeros(m * k + 8, device="cuda", dtype=torch.float32 if case == "fp32" else torch.bfloat16)
    off = 4 if case == "misaligned" else 0
    w = torch.zeros(n, k, device="cuda", dtype=torch.bfloat16)
    assert _C().conv1x1_wide_ok(m, k, n) == (case in ("fp32", "misaligned"))
    with pytest.raises(RuntimeError):
        _C().conv1x1_wide(x[off:off + m * k].view(m, k), w)


def test_dispatch_hands_statistics_to_batchnorm(monkeypatch):
    """``Conv1x1NHWC(512, 256)`` pinned to ``hip_wide`` against the same layer pinned to
    ``hip``, each followed by a training BatchNormAct2d (the bounds of
    test_conv1x1_stats.py::test_bn_consumes_conv_epilogue_stats).  Integer operands: the two
    kernels add in different orders, and only exact sums give both the same y.  The input
    gradient is pinned to the GEMM in both runs, so it compares what the forward fed."""
    from ray_lightning_accelerators_amd.ops import conv as C
    from ray_lightning_accelerators_amd.ops.bn import BatchNormAct2d

    monkeypatch.setitem(C._choice, ("dgrad", 4 * 14 * 14, 512, 256), "gemm")

    g = torch.Generator().manual_seed(3)
    conv = C.Conv1x1NHWC(512, 256).cuda()
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-2, 3, conv.weight.shape, generator=g))
    x0 = torch.randint(-1, 2, (4, 512, 14, 14), generator=g).to(torch.bfloat16).cuda()
    x0 = x0.contiguous(memory_format=torch.channels_last)
    outs = []
    for mode in ("hip", "hip_wide"):
        monkeypatch.setenv("RLA_CONV1X1", mode)
        bn = BatchNormAct2d(256).cuda()
        bn.momentum = None
        x = x0.clone().requires_grad_(True)
        for _ in range(2):
            st = C.BNStats()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = conv(x, bn_stats=st)
                assert st.part is not None
                z = bn(y, None, bn_stats=st)
        z.float().square().sum().backward()
        outs.append((z.detach().float(), x.grad.float(), bn.running_mean.clone(), bn.running_var.clone(),
                     int(bn.num_batches_tracked)))
    (z0, g0, m0, v0, n0), (z1, g1, m1, v1, n1) = outs
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    assert n0 == n1 == 2
    assert rel(z1, z0) < 1e-5 and rel(g1, g0) < 1e-4
    assert torch.allclose(m1, m0, rtol=1e-5, atol=1e-6) and torch.allclose(v1, v0, rtol=1e-5, atol=1e-6)

    # the candidate tables: the wide kernel (it wins no ResNet-50 shape) only where pinned and
    # Cin >= 256; the timed tables are what they were
    seen = []
    monkeypatch.setattr(C, "_pick", lambda op, key, cands: seen.append((key[1], tuple(cands))) or "hip")
    x64 = x0[:, :64].contiguous(memory_format=torch.channels_last)
    for mode in ("hip_wide", "auto"):
        monkeypatch.setenv("RLA_CONV1X1", mode)
        with torch.no_grad():
            conv(x0, bn_stats=C.BNStats())
            C.Conv1x1NHWC(64, 64).cuda()(x64, bn_stats=C.BNStats())
    stock = ("hip", "gemm", "miopen")
    assert seen == [(512, ("hip", "hip_wide", "gemm", "miopen")), (64, stock), (512, stock), (64, stock)]
