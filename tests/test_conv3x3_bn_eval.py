"""csrc/conv3x3.hip's ACT epilogue against float64: out = bf16(act(fma(acc, scale, shift))) with
scale = gamma / sqrt(var + eps), shift = fma(-mean, scale, beta), through the binding at every
instance family (cases of test_conv_partition.py C3_CASES), through ``Bottleneck`` in eval mode,
and the eval-mode stem route through ``ResNet``.  Measured ratios on an MI355X:
profiles/r31_conv3x3_bn_eval/test_ratios.log."""
import functools

import pytest
import torch

from bn_reference import HALF_BF16, U, same_bf16, to_bf16
from ray_lightning_accelerators_amd.ops import conv as C
from test_conv1x1_bn_eval import _C, _block, _block_fp64

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout), pinned CUs, pinned tile, the instance (tm, nx, compile-time shape)
CASES = [
    ((1, 4, 4, 16, 64), None, None, None),            # one chunk, one short tile
    ((7, 11, 13, 48, 64), 2, 256, (256, 4, False)),   # run-time shape, fractional range edges
    ((3, 33, 20, 32, 128), 2, 512, (512, 6, False)),  # two channel blocks: the table follows nblk
    ((2, 56, 56, 64, 64), 4, None, (512, 7, True)),
    ((2, 28, 28, 128, 128), 4, None, (512, 5, True)),
    ((2, 28, 28, 128, 128), 4, 256, (256, 4, True)),
    ((4, 14, 14, 256, 256), 8, None, (256, 4, True)),
    ((8, 7, 7, 512, 512), 16, None, (256, 4, True)),
]


@functools.lru_cache(maxsize=None)
def _data(shape, kind):
    """CPU operands of one shape and their float64 convolution, made once.  ``int``: every fp32
    intermediate is exact (|acc| <= 16 * 9 Cin < 2^24, var = 1, eps = 0, scale in {+-0.5, +-1, +-2})."""
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(n + 3 * h + 5 * w + 7 * cin + 11 * cout)
    sign = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
    if kind == "int":
        x = torch.randint(1, 5, (n, h, w, cin), generator=g) * sign(n, h, w, cin)
        wt = torch.randint(1, 5, (cout, 3, 3, cin), generator=g) * sign(cout, 3, 3, cin)
        mean, beta = (torch.randint(-8, 9, (cout,), generator=g).float() for _ in range(2))
        gamma = 2.0 ** torch.randint(-1, 2, (cout,), generator=g).float() * sign(cout)
        var, eps = torch.ones(cout), 0.0
    else:
        x, wt = torch.randn(n, h, w, cin, generator=g), torch.randn(cout, 3, 3, cin, generator=g) / (9 * cin) ** 0.5
        mean, beta = 0.5 * torch.randn(cout, generator=g), torch.randn(cout, generator=g)
        gamma = (0.5 + torch.rand(cout, generator=g)) * sign(cout)
        var, eps = 0.25 + 3.75 * torch.rand(cout, generator=g), 1e-5
    x, wt = x.to(torch.bfloat16), wt.to(torch.bfloat16)
    conv = lambda a, b: torch.nn.functional.conv2d(a.double().permute(0, 3, 1, 2), b.double().permute(0, 3, 1, 2),
                                                   padding=1).permute(0, 2, 3, 1)
    return {"x": x, "w": wt, "mean": mean, "var": var, "gamma": gamma, "beta": beta, "eps": eps,
            "acc": conv(x, wt), "absdot": conv(x.abs(), wt.abs())}


def _reference(d, relu):
    """(out float64, bound): test_conv1x1_bn_eval._reference's bound with K = 9 Cin and no residual:
    K u A |scale| (accumulator), 3 u |acc scale| (scale's roundings), 4 u (|beta| + |mean scale|)
    (shift), one rounding of the fma, then half a bf16 ulp."""
    s = lambda t: t.double()
    acc, k = d["acc"], 9 * d["x"].size(3)
    scale = s(d["gamma"]) / torch.sqrt(s(d["var"]) + float(torch.tensor(d["eps"], dtype=torch.float32)))
    shift = s(d["beta"]) - s(d["mean"]) * scale
    out = acc * scale + shift
    assert bool((out > 0).any() and (out < 0).any() and (scale < 0).any())  # both ReLU branches, a negative gamma
    err = U * (scale.abs() * k * d["absdot"] + 3 * (acc * scale).abs()
               + 4 * (s(d["beta"]).abs() + (s(d["mean"]) * scale).abs()) + (acc * scale).abs() + shift.abs())
    out = torch.clamp(out, min=0.0) if relu else out
    return out, HALF_BF16 * out.abs() + (1 + HALF_BF16) * err


def _run(d, shape, relu):
    dev = lambda t: t.cuda()
    return _C().conv3x3_bn_act(dev(d["x"]), dev(d["w"]), *shape, dev(d["mean"]), dev(d["var"]), dev(d["gamma"]),
                               dev(d["beta"]), d["eps"], relu)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-cu{c[1]}-tm{c[2]}")
def test_matches_fp64(monkeypatch, case, relu, kind):
    shape, cus, tm, instance = case
    d = _data(shape, kind)
    monkeypatch.delenv("RLA_CONV3X3_TM", raising=False)
    out = _run(d, shape, relu)  # the default plan
    assert out.shape == shape[:3] + shape[4:] and out.dtype == torch.bfloat16
    if instance is not None:  # the pinned plan reaches the instance it names: the same bits
        if tm:
            monkeypatch.setenv("RLA_CONV3X3_TM", str(tm))
        _C().set_plan_cus(cus)
        try:
            p_tm, _, _, _, p_nx, p_fixed = _C().conv3x3_plan(*shape)
            assert (p_tm, p_nx, bool(p_fixed)) == instance
            pinned = _run(d, shape, relu)
        finally:
            _C().set_plan_cus(0)
        assert torch.equal(pinned, out)
    ref, bound = _reference(d, relu)
    if kind == "int":
        assert bool(same_bf16(out.cpu(), to_bf16(ref)).all())
    else:
        ratio = ((out.double().cpu() - ref).abs() / bound).max().item()
        print(f"conv3x3_bn_act {shape} cu{cus} tm{tm} relu={relu}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("case", ["Cin=24", "Cout=96", "fp32_x", "long_var", "short_w"])
def test_refused_before_launch(case):
    n, h, w, cin, cout = 2, 5, 6, (24 if case == "Cin=24" else 32), (96 if case == "Cout=96" else 64)
    assert _C().conv3x3_bn_act_ok(n, h, w, cin, cout) == (case not in ("Cin=24", "Cout=96"))
    x = torch.zeros(n, h, w, cin, device="cuda", dtype=torch.float32 if case == "fp32_x" else torch.bfloat16)
    wt = torch.zeros(cout - (case == "short_w"), 3, 3, cin, device="cuda", dtype=torch.bfloat16)
    vec = [torch.ones(cout + (case == "long_var" and i == 1), device="cuda") for i in range(4)]
    name = {"Cin=24": "unsupported shape", "Cout=96": "unsupported shape", "fp32_x": "conv3x3_bn_act: x",
            "long_var": "conv3x3_bn_act: var", "short_w": "conv3x3_bn_act: w"}[case]
    with pytest.raises(RuntimeError, match=name):
        _C().conv3x3_bn_act(x, wt, n, h, w, cin, cout, *vec, 1e-5, True)


def _forward(monkeypatch, net, x, mode, key):
    monkeypatch.setenv("RLA_CONV3X3_BN_EVAL", mode)
    before = C.stats[key]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = net(x)
    return y, C.stats[key] - before


def test_block_eval(monkeypatch):
    """An identity Bottleneck in eval mode: the switch at 1 fuses conv2, at 0 or with a forward hook
    on conv2 it does not, and those two agree bitwise.  The fused route drops a rounding: its rms
    error against float64 may not exceed the split route's by more than FACTOR."""
    FACTOR = 1.044  # measured 0.994, + 0.05 for another library build of the split route's convolution
    monkeypatch.setenv("RLA_CONV1X1", "gemm")
    monkeypatch.setenv("RLA_CONV1X1_BN_EVAL", "1")  # the 1x1 layers on one untimed route in every run
    blk = _block(False)
    x = torch.randn(2, 256, 14, 14, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
    x = x.contiguous(memory_format=torch.channels_last)
    ref = _block_fp64(blk.double(), x.double()).cpu()
    blk.float()
    fused, n1 = _forward(monkeypatch, blk, x, "1", "bn_eval_fused_3x3")
    split, n0 = _forward(monkeypatch, blk, x, "0", "bn_eval_fused_3x3")
    hook = blk.conv2.register_forward_hook(lambda *a: None)
    hooked, nh = _forward(monkeypatch, blk, x, "1", "bn_eval_fused_3x3")
    hook.remove()
    assert (n1, n0, nh) == (1, 0, 0)
    assert torch.equal(split, hooked) and fused.dtype == split.dtype == torch.bfloat16
    rms = lambda y: ((y.double().cpu() - ref) ** 2).mean().sqrt().item()
    print(f"bottleneck conv2: rms error fused {rms(fused):.3e}, split {rms(split):.3e}, "
          f"ratio {rms(fused) / rms(split):.3f}, factor {FACTOR}")
    assert rms(fused) <= FACTOR * rms(split)


def test_stem_route(monkeypatch):
    """The eval-mode stem of a small ResNet under ``no_grad``: bitwise the max pool of ``bn_apply``
    of the stem kernel's output, built from the bindings; switched off, the modules' own route."""
    from ray_lightning_accelerators_amd.models.resnet import ResNet
    from ray_lightning_accelerators_amd.ops.bn import eval_scale_shift

    monkeypatch.setenv("RLA_CONV1X1_BN_EVAL", "0")  # nothing timed
    torch.manual_seed(3)
    net = ResNet([1, 1, 1, 1], num_classes=8, fused_bn=True).cuda().to(memory_format=torch.channels_last).eval()
    net.bn1.running_mean.normal_(0, 0.5)
    net.bn1.running_var.uniform_(0.25, 4.0)
    net.bn1.weight.data.uniform_(-1.5, 1.5)
    x = torch.randn(2, 3, 64, 64, device="cuda").contiguous(memory_format=torch.channels_last)
    seen = []
    net.layer1.register_forward_pre_hook(lambda m, a: seen.append(a[0]))  # what the stem hands on
    n1, n0 = (_forward(monkeypatch, net, x, mode, "bn_eval_stem")[1] for mode in "10")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        lib = net.maxpool(net.bn1(net.conv1(x)))
    y = C.stem_hip(x.to(torch.bfloat16), net.conv1.weight.detach().to(torch.bfloat16))
    a = torch.empty_like(y)
    _C().bn_apply(y.permute(0, 2, 3, 1), *eval_scale_shift(net.bn1), None, True, a.permute(0, 2, 3, 1))
    want = _C().maxpool_fwd(a.permute(0, 2, 3, 1), 3, 2, 1)[0].permute(0, 3, 1, 2)
    assert (n1, n0) == (1, 0)
    assert torch.equal(seen[0], want) and torch.equal(seen[1], lib)
