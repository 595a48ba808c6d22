"""The 3x3 / stride 2 / pad 1 MFMA input gradient (csrc/conv3x3s2_dgrad.hip) from the kernel
up to ``_ConvNHWCFn``: ResNet-50's downsample conv2 layers, backward.

The fp64 oracle is a tap scatter: ``dxp[:, r:r+2OH-1:2, s:s+2OW-1:2] += dy @ w[:, r, s, :]`` on
a padded [2 OH + 1, 2 OW + 1] image, cropped to [1:H+1, 1:W+1]; a CPU test holds it against
fp64 ``F.conv2d`` autograd (1e-12) on even and odd sizes, 1x1 and 2x2 images.

Kernel checks, on the raw binding (NHWC memory; layer shapes (N, H, W, Cin, Cout), so the
kernel's Cr = Cout and Co = Cin):
  * against fp32 autograd of ``F.conv2d`` on the same bf16 operands, ``tests/test_conv3x3.py``'s
    two bounds (relative norm error < 8e-3, max error < 5 % of the largest reference value);
  * element-wise against the oracle: ``|dx - ref| <= 2^-8 |ref| + 2 K 2^-24 A`` with
    K = 4 Cout (no input pixel receives more than four taps) and A the oracle on |dy|, |w|:
    bf16 rounding of the output plus fp32 accumulation of K products.  No element is left
    out and the output is finite;
  * every element of dx is written: a run on dy = 0 into memory a run on random data (and a
    NaN fill) just left behind gives exact zeros everywhere, half-empty quads included;
  * at pinned planning CU counts every workgroup has at least three tiles and a shorter last
    one (asserted from ``conv3x3s2_dgrad_plan``): dx within the bound, bitwise the default
    plan's, two runs bitwise equal.  The cases: ResNet's 56x56 and 28x28 layers, the odd-size
    11x13 shape, and the 14x14 layer at batch 22, where the tile at quad 1024 starts in the
    last quad row of image 20 (row 6, column 2) and runs into image 21;
  * ResNet's three shapes are taken at every batch size 1..256 on 256 planning CUs, and the
    Python predicate follows a re-pinned plan;
  * bad operands (wrong device, dtype, non-contiguous, 2 bytes off alignment, one element
    short) and unsupported shapes (Cr % 16, Co % 64) raise before any launch.

The shapes: ResNet's three layers at small batch, the 4x4 image, odd H and W, one reduction
chunk, two channel blocks, 1x1 and 2x2 images, and two wide rows that run the 3- and 4-piece
halo instances (every other shape runs the 2-piece one).  Each test prints its worst error /
bound ratio; measured on an MI355X: element-wise 0.66-0.99 (the bf16 rounding term: an output
just above a power of two is rounded by up to 2^-8 of itself), relative norm error against
fp32 1.6e-3 - 1.8e-3.

Dispatch checks: ``RLA_CONV3X3S2_DGRAD`` forced to ``hip`` and ``miopen`` (the forced backend is
the one that runs; results within test_conv_dispatch.py's bounds of each other), deterministic
mode (the in-tree kernel, nothing timed, no library backward, bitwise repeatable), a downsample
``Bottleneck``, a forked input, and a shape the forward predicate refuses.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import conv as C

gpu = pytest.mark.gpu

U24 = 2.0 ** -24
U8 = 2.0 ** -8

# layer shapes (N, H, W, Cin, Cout)
SHAPES = [
    (2, 56, 56, 128, 128), (2, 28, 28, 256, 256), (3, 14, 14, 512, 512),  # ResNet's three layers
    (2, 4, 4, 512, 512),                                                  # layer4 of a 64x64 image
    (3, 7, 7, 64, 64), (7, 11, 13, 64, 48),                               # odd H, W: half-empty quads; Cout % 64 != 0
    (2, 5, 9, 64, 16),                                                    # one reduction chunk
    (1, 3, 3, 128, 32),                                                   # two channel blocks
    (1, 1, 1, 64, 64),                                                    # only the even/even class exists
    (1, 2, 2, 64, 16), (1, 2, 5, 64, 16),
    (1, 2, 257, 64, 16), (1, 2, 383, 64, 16),                             # the 3- and 4-piece halo instances
]
# halo pieces per thread of the instance a shape runs (every other shape above: 2)
INSTANCE_NX = {(1, 2, 257, 64, 16): 3, (1, 2, 383, 64, 16): 4}
# (shape, plan CUs): every workgroup gets at least three 128-quad tiles and a shorter last one
SPLIT_CASES = [
    ((2, 56, 56, 128, 128), 8),    # 4 ranges of 392 quads per channel block
    ((2, 28, 28, 256, 256), 4),    # one range of 392
    ((7, 11, 13, 64, 48), 1),      # odd sizes, one range of 294
    ((22, 14, 14, 512, 512), 8),   # one range of 1078: 7x7 quads per image, tiles cross images
]
CROSSING = ((22, 14, 14, 512, 512), 8)


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


def dgrad_ref(dy, wt, h, w):
    """fp64 dx[n][ih][iw][ci] = sum dy[n][oh][ow][co] wt[co][r][s][ci] over 2 oh + r - 1 = ih,
    2 ow + s - 1 = iw (NHWC; wt is the forward weight [Cout][3][3][Cin])."""
    n, oh, ow, _ = dy.shape
    assert (oh, ow) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    dxp = torch.zeros(n, 2 * oh + 1, 2 * ow + 1, wt.size(3), dtype=torch.float64, device=dy.device)
    dyd, wd = dy.double(), wt.double()
    for r in range(3):
        for s in range(3):
            dxp[:, r:r + 2 * oh - 1:2, s:s + 2 * ow - 1:2, :] += dyd @ wd[:, r, s, :]
    return dxp[:, 1:h + 1, 1:w + 1, :].contiguous()


def _autograd_dx(dy, wt, h, w, dtype):
    """``F.conv2d``'s autograd input gradient in ``dtype`` from NHWC operands; NHWC result."""
    x = torch.zeros(dy.size(0), wt.size(3), h, w, dtype=dtype, device=dy.device, requires_grad=True)
    y = F.conv2d(x, wt.to(dtype).permute(0, 3, 1, 2), stride=2, padding=1)
    y.backward(dy.to(dtype).permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Operands (NHWC memory) and fp64 references of a shape, computed once and never written again."""
    n, h, w, cin, cout = shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(500 + sum(shape))
    dy = torch.randn(n, oh, ow, cout, generator=g).to(dev).to(torch.bfloat16)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) / (2 * cout ** 0.5)).to(dev).to(torch.bfloat16)
    return {"dy": dy, "wt": wt, "ref": dgrad_ref(dy, wt, h, w), "amp": dgrad_ref(dy.abs(), wt.abs(), h, w)}


def _run(shape, dy=None):
    n, h, w, cin, cout = shape
    d = _data(shape)
    return _ops().conv3x3s2_dgrad(d["dy"] if dy is None else dy, d["wt"], n, h, w, cout, cin)


def _check_elementwise(tag, dx, ref, amp, k):
    assert dx.shape == ref.shape, (dx.shape, ref.shape)
    assert bool(torch.isfinite(dx.float()).all()), f"{tag}: non-finite output"
    err = (dx.double() - ref).abs()
    bound = U8 * ref.abs() + 2.0 * k * U24 * amp
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst, nbad = float(ratio.max()), int((ratio > 1.0).sum())
    print(f"[bound ratio] {tag}: worst {worst:.3f}")
    assert nbad == 0, f"{tag}: {nbad} of {ref.numel()} elements past the bound, worst {worst:.3f}"


def _plan(shape):
    """(tq, the workgroups' quad ranges, OH, OW) of the current plan."""
    n, h, w, cin, cout = shape
    tq, wpb, _, pieces, nx, fixed, oh, ow = _ops().conv3x3s2_dgrad_plan(n, h, w, cout, cin)
    assert (oh, ow) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1) and pieces <= nx and not fixed
    q = n * oh * ow
    return tq, [(q * j // wpb, q * (j + 1) // wpb) for j in range(wpb)], oh, ow


# ------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("geo", [(2, 6, 8), (2, 7, 5), (3, 1, 1), (2, 2, 2), (1, 2, 5), (2, 11, 13), (1, 8, 7)],
                         ids=lambda g: "x".join(map(str, g)))
def test_oracle_equals_fp64_autograd(geo):
    """The tap-scatter oracle is ``F.conv2d``'s fp64 input gradient on even and odd sizes."""
    n, h, w = geo
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator().manual_seed(7 + sum(geo))
    dy = torch.randn(n, oh, ow, 5, generator=g, dtype=torch.float64)
    wt = torch.randn(5, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = dgrad_ref(dy, wt, h, w)
    want = _autograd_dx(dy, wt, h, w, torch.float64)
    assert ref.shape == want.shape == (n, h, w, 3)
    assert float((ref - want).abs().max()) < 1e-12


def _operands(shape, cout, device="cuda", seed=0):
    """x bf16 channels_last, the fp32 master weight, its bf16 copy and an output gradient."""
    g = torch.Generator().manual_seed(seed)
    n, cin, h, w = shape
    x = torch.randn(n, cin, h, w, generator=g).to(torch.bfloat16)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    dy = torch.randn(n, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1, generator=g).to(torch.bfloat16)
    x, wt, dy = (t.to(device).contiguous(memory_format=torch.channels_last) for t in (x, wt, dy))
    return x, wt, wt.to(torch.bfloat16), dy


def _convs2(x, wt, wb, dy, fork=None):
    x, wt = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = C._ConvNHWCFn.apply(x, wt, wb, (2, 2), (1, 1), fork, None)
    y.backward(dy)
    return y.detach(), x.grad, wt.grad


def _autograd(x, wb, dy):
    """``F.conv2d``'s autograd on the bf16 weight; the weight gradient widened to fp32."""
    x, wb = x.clone().requires_grad_(True), wb.clone().requires_grad_(True)
    y = F.conv2d(x, wb, stride=2, padding=1)
    y.backward(dy)
    return y.detach(), x.grad, wb.grad.float()


def test_cpu_layer_and_predicate(monkeypatch):
    """On the CPU the predicate is false before the extension is touched and the layer
    equals ``F.conv2d``'s autograd exactly."""
    from ray_lightning_accelerators_amd import ops

    def no_extension():
        raise AssertionError("the CPU path loaded the extension")

    monkeypatch.setattr(ops, "require", no_extension)
    monkeypatch.setattr(C, "_pick", lambda op, key, cands: "miopen")  # nothing to time on the CPU
    x, wt, wb, dy = _operands((2, 64, 6, 5), 64, device="cpu")
    assert not C.conv3x3s2_dgrad_ok(dy, wb, 6, 5)
    for a, b in zip(_convs2(x, wt, wb, dy), _autograd(x, wb, dy)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a, b), float((a.float() - b.float()).abs().max())


# ------------------------------------------------------------------------------ kernel
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_matches_fp32_autograd(shape):
    """``conv3x3s2_dgrad_hip`` against fp32 ``F.conv2d`` autograd of the same bf16 operands."""
    n, h, w, cin, cout = shape
    d = _data(shape)
    dy, wb = d["dy"].permute(0, 3, 1, 2), d["wt"].permute(0, 3, 1, 2)
    assert C.conv3x3s2_dgrad_ok(dy, wb, h, w)
    dx = C.conv3x3s2_dgrad_hip(dy, wb, h, w)
    assert dx.shape == (n, cin, h, w) and dx.dtype == torch.bfloat16
    assert dx.is_contiguous(memory_format=torch.channels_last)
    ref = _autograd_dx(d["dy"], d["wt"], h, w, torch.float32).permute(0, 3, 1, 2)
    rel, mx = _rel(dx, ref), float((dx.float() - ref).abs().max())
    print(f"[rel] conv3x3s2_dgrad {_id(shape)}: {rel:.3e}, max |err| {mx:.3e} of {float(ref.abs().max()):.3e}")
    assert rel < 8e-3
    assert mx < 0.05 * float(ref.abs().max())


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_elementwise_against_fp64(shape):
    """Every element within the derived bound: bf16 rounding + fp32 accumulation of K = 4 Cout products."""
    d = _data(shape)
    n, h, w, cin, cout = shape
    assert _ops().conv3x3s2_dgrad_plan(n, h, w, cout, cin)[4] == INSTANCE_NX.get(shape, 2)
    dx = _run(shape)
    _check_elementwise("conv3x3s2_dgrad " + _id(shape), dx, d["ref"], d["amp"], 4 * shape[4])


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_every_element_is_written(shape):
    """dx comes from ``torch.empty``: a run on dy = 0 into memory that a run on random data and
    a NaN fill of the same size just released must give exact zeros everywhere (the pixels of
    half-empty quads included), so no element is left to the allocator's old contents."""
    d = _data(shape)
    dx = _run(shape)
    assert dx.numel() == d["ref"].numel() and bool(torch.isfinite(dx.float()).all())
    del dx
    junk = torch.full_like(d["ref"], float("nan"), dtype=torch.bfloat16)
    del junk
    dx0 = _run(shape, dy=torch.zeros_like(d["dy"]))
    assert int((dx0.float() != 0).sum() + torch.isnan(dx0.float()).sum()) == 0


@gpu
@pytest.mark.parametrize("shape,cus", SPLIT_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else f"cu{v}")
def test_pinned_plan_is_bitwise_the_default(plan_cus, shape, cus):
    """Several tiles per workgroup with a shorter last one: dx within the bound, bitwise the
    default plan's, and two runs bitwise equal."""
    d = _data(shape)
    dx0 = _run(shape)
    plan_cus(cus)
    tq, ranges, oh, ow = _plan(shape)
    for lo, hi in ranges:
        assert hi - lo >= 2 * tq + 1 and (hi - lo) % tq != 0, (lo, hi, tq)
    if (shape, cus) == CROSSING:
        # some tile starts in the last quad row of an image and runs into the next image
        tiles = [(q0, min(q0 + tq, hi)) for lo, hi in ranges for q0 in range(lo, hi, tq)]
        hit = [(q0, q1) for q0, q1 in tiles if (q0 % (oh * ow)) // ow == oh - 1
               and q1 - 1 >= (q0 // (oh * ow) + 1) * oh * ow]
        assert hit, tiles
    dx1 = _run(shape)
    dx2 = _run(shape)
    tag = f"conv3x3s2_dgrad split {_id(shape)}-cu{cus}"
    _check_elementwise(tag, dx1, d["ref"], d["amp"], 4 * shape[4])
    assert torch.equal(dx1, dx0), f"{tag}: differs from the default plan"
    assert torch.equal(dx1, dx2), f"{tag}: two runs differ"


@gpu
def test_resnet_shapes_supported_at_every_batch(plan_cus):
    """ResNet's three layers are taken at every batch size 1..256 on 256 CUs, and the Python
    predicate answers for the plan in force, not for the one it first saw."""
    m = _ops()
    plan_cus(256)
    for h, c in ((56, 128), (28, 256), (14, 512)):
        bad = [n for n in range(1, 257) if not m.conv3x3s2_dgrad_supported(n, h, h, c, c)]
        assert not bad, (h, c, bad)
    # dy of a (1, 8, 400) input: 4 x 200 quads, halo rows of 201 entries against 512.  25 ranges
    # of 32 quads: some span two quad rows (3 halo rows, refused); 8 ranges of 100 stay in one
    # (2 halo rows, taken)
    dy = torch.zeros(1, 64, 4, 200, device=_dev(), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wb = torch.zeros(64, 64, 3, 3, device=_dev(), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert not C.conv3x3s2_dgrad_ok(dy, wb, 8, 400)
    plan_cus(8)
    assert C.conv3x3s2_dgrad_ok(dy, wb, 8, 400)
    dx = C.conv3x3s2_dgrad_hip(dy, wb, 8, 400)
    assert dx.shape == (1, 64, 8, 400) and int((dx.float() != 0).sum()) == 0
    assert C.conv3x3s2_dgrad_ok(dy, wb, 7, 399)      # OH does not determine H: the odd sizes too
    assert not C.conv3x3s2_dgrad_ok(dy, wb, 6, 400)  # dy is not that input's output gradient
    plan_cus(256)
    assert not C.conv3x3s2_dgrad_ok(dy, wb, 8, 400)


def _break(t, how):
    if how == "cpu":
        return t.cpu()
    if how == "fp32":
        return t.float()
    if how == "noncontiguous":  # same shape and element count, every other element of a wider buffer
        wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
        v = wide[..., ::2]
        assert v.shape == t.shape and not v.is_contiguous() and v.data_ptr() % 16 == 0
        return v
    if how == "offset":  # contiguous, the right size, 2 bytes off every wider alignment
        v = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 4 == 2
        return v
    if how == "numel":  # one element short
        return torch.zeros(t.numel() - 1, dtype=t.dtype, device=t.device)
    raise AssertionError(how)


@gpu
@pytest.mark.parametrize("how", ["cpu", "fp32", "noncontiguous", "offset", "numel"])
@pytest.mark.parametrize("which", ["dy", "w"])
def test_bad_operand_is_refused(which, how):
    """A bad operand raises before any launch."""
    m = _ops()
    args = (1, 4, 4, 16, 64)  # N, H, W, Cr, Co
    assert m.conv3x3s2_dgrad_supported(*args)
    o = {"dy": torch.zeros(1, 2, 2, 16, dtype=torch.bfloat16, device=_dev()),
         "w": torch.zeros(16, 3, 3, 64, dtype=torch.bfloat16, device=_dev())}
    o[which] = _break(o[which], how)
    with pytest.raises(RuntimeError, match="conv3x3s2_dgrad"):
        m.conv3x3s2_dgrad(o["dy"], o["w"], *args)


@gpu
@pytest.mark.parametrize("cr,co", [(24, 64), (16, 48)], ids=["cr24", "co48"])
def test_unsupported_shape_raises(cr, co):
    m = _ops()
    assert not m.conv3x3s2_dgrad_supported(1, 4, 4, cr, co)
    dy = torch.zeros(1, 2, 2, cr, dtype=torch.bfloat16, device=_dev())
    w = torch.zeros(cr, 3, 3, co, dtype=torch.bfloat16, device=_dev())
    with pytest.raises(RuntimeError, match="unsupported shape"):
        m.conv3x3s2_dgrad(dy, w, 1, 4, 4, cr, co)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        m.conv3x3s2_dgrad_plan(1, 4, 4, cr, co)


# ------------------------------------------------------------------------------ dispatch
def _count_backends(monkeypatch):
    """Counts calls of the in-tree input gradient and of ``_miopen_bwd`` asked for dx."""
    calls = {"hip": 0, "miopen_dx": 0, "miopen_bwd": 0}
    real_hip, real_bwd = C.conv3x3s2_dgrad_hip, C._miopen_bwd

    def hip(*a):
        calls["hip"] += 1
        return real_hip(*a)

    def bwd(dy, x, w4, stride, padding, need_dx, need_dw):
        calls["miopen_bwd"] += 1
        calls["miopen_dx"] += bool(need_dx)
        return real_bwd(dy, x, w4, stride, padding, need_dx, need_dw)

    monkeypatch.setattr(C, "conv3x3s2_dgrad_hip", hip)
    monkeypatch.setattr(C, "_miopen_bwd", bwd)
    return calls


@gpu
def test_forced_backend_is_the_one_that_runs(monkeypatch):
    """``RLA_CONV3X3S2_DGRAD=hip|miopen``: the forced backend computes the input gradient, and
    the two runs agree within test_conv_dispatch.py's bounds (1e-2; input gradient 2e-2)."""
    ops = _operands((4, 64, 8, 8), 64)
    calls = _count_backends(monkeypatch)
    timed = {k for k in C._choice if k[0] == "dgrad_s2"}
    out = {}
    for mode in ("hip", "miopen"):
        monkeypatch.setenv("RLA_CONV3X3S2_DGRAD", mode)
        calls.update(hip=0, miopen_dx=0, miopen_bwd=0)
        out[mode] = _convs2(*ops)
        if mode == "hip":
            assert calls["hip"] == 1 and calls["miopen_dx"] == 0, calls
        else:
            assert calls["hip"] == 0 and calls["miopen_dx"] >= 1, calls
    for i, (a, b) in enumerate(zip(out["hip"], out["miopen"])):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert _rel(a, b) < (2e-2 if i == 1 else 1e-2), (i, _rel(a, b))
    assert {k for k in C._choice if k[0] == "dgrad_s2"} == timed  # a forced backend times nothing


@gpu
def test_deterministic_mode_runs_the_kernel(monkeypatch):
    """Under deterministic algorithms the layer's backward is in-tree end to end: the input
    gradient on the MFMA kernel, no library backward call, nothing timed, and two backward
    passes bitwise equal in dx and dw."""
    ops = _operands((4, 64, 8, 8), 64)
    calls = _count_backends(monkeypatch)
    for name in ("RLA_CONV1X1", "RLA_CONV_WGRAD", "RLA_CONV3X3S2_DGRAD"):
        monkeypatch.delenv(name, raising=False)
    before = dict(C._choice)
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        y1, dx1, dw1 = _convs2(*ops)
        y2, dx2, dw2 = _convs2(*ops)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    assert calls["hip"] == 2 and calls["miopen_bwd"] == 0, calls
    assert C._choice == before
    assert torch.equal(dx1, dx2) and torch.equal(dw1, dw2) and torch.equal(y1, y2)
    ref = _autograd(*ops[:1], ops[2], ops[3])
    assert _rel(dx1, ref[1]) < 2e-2 and _rel(dw1, ref[2]) < 1e-2


@gpu
def test_downsample_block_hip_against_miopen(monkeypatch):
    """A downsample bottleneck with its conv2 input gradient on the in-tree kernel against
    the library's: output, ``x.grad`` and ``conv2.weight.grad`` within 2e-2."""
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck, _bn, _conv1x1
    from ray_lightning_accelerators_amd.parallel.arena import ParamArena
    from torch import nn

    dev = _dev()
    calls = _count_backends(monkeypatch)
    outs, ran = {}, {}
    for mode in ("hip", "miopen"):
        monkeypatch.setenv("RLA_CONV3X3S2_DGRAD", mode)
        calls.update(hip=0, miopen_dx=0, miopen_bwd=0)
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
        outs[mode] = (y.detach().float(), x.grad.float(), blk.conv2.weight.grad.clone())
        ran[mode] = calls["hip"]
    assert ran == {"hip": 1, "miopen": 0}, ran
    assert outs["hip"][0].shape == (4, 512, 8, 8)
    for a, b in zip(outs["hip"], outs["miopen"]):
        assert _rel(a, b.float()) < 2e-2, _rel(a, b.float())


@gpu
@pytest.mark.parametrize("s2_last", [True, False], ids=["s2_parks", "s2_adds"])
def test_forked_input_receives_the_sum(monkeypatch, s2_last):
    """A 1x1 conv and the stride-2 3x3 conv reading one tensor through a ``GradFork``: whichever
    backward runs second returns the sum of both input gradients."""
    monkeypatch.setenv("RLA_CONV3X3S2_DGRAD", "hip")
    calls = _count_backends(monkeypatch)
    x, w3, wb3, dy3 = _operands((4, 64, 8, 8), 64)
    g = torch.Generator().manual_seed(3)
    w1 = (torch.randn(64, 64, 1, 1, generator=g) / 8).to(_dev())
    dy1 = torch.randn(4, 64, 8, 8, generator=g).to(torch.bfloat16).to(_dev()).contiguous(
        memory_format=torch.channels_last)
    xs, w1s, w3s = (t.clone().requires_grad_(True) for t in (x, w1, w3))
    fork = C.GradFork()
    y1 = y3 = None
    for s2 in (not s2_last, s2_last):  # the layer applied last runs its backward first and parks
        if s2:
            y3 = C._ConvNHWCFn.apply(xs, w3s, wb3, (2, 2), (1, 1), fork)
        else:
            y1 = C._Conv1x1Fn.apply(xs, w1s, None, fork, None, False)
    torch.autograd.backward([y1, y3], [dy1, dy3])
    assert fork.dx is None and calls["hip"] == 1
    xr = x.clone().float().requires_grad_(True)
    torch.autograd.backward([F.conv2d(xr, w1.to(torch.bfloat16).float()),
                             F.conv2d(xr, wb3.float(), stride=2, padding=1)], [dy1.float(), dy3.float()])
    assert xs.grad.shape == xr.grad.shape
    assert _rel(xs.grad, xr.grad) < 2e-2, _rel(xs.grad, xr.grad)


@gpu
def test_forward_refused_shape_keeps_the_library_calls(monkeypatch, plan_cus):
    """A shape the FORWARD predicate refuses (a halo row too wide for its LDS image) makes
    exactly the library calls of any strided layer, even where the input-gradient kernel
    would take it and is forced."""
    monkeypatch.setenv("RLA_CONV3X3S2_DGRAD", "hip")
    plan_cus(8)
    x, wt, wb, dy = _operands((1, 64, 8, 400), 64)
    assert not C.conv3x3s2_ok(x, wb, (2, 2), (1, 1)) and C.conv3x3s2_dgrad_ok(dy, wb, 8, 400)
    hip = _count_backends(monkeypatch)
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
    got = _convs2(x, wt, wb, dy)
    assert seen == ["wgrad_kxk"] and calls == ["_miopen_fwd", "_miopen_bwd"] and hip["hip"] == 0
    for i, (a, b) in enumerate(zip(got, _autograd(x, wb, dy))):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert _rel(a, b) < (2e-2 if i == 1 else 1e-2), (i, _rel(a, b))
