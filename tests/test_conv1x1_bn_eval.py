"""csrc/conv1x1_bn_act.hip against float64: the 1x1 forward whose epilogue is an eval-mode
BatchNorm, the ReLU and the shortcut add,

    out = bf16(act(fma(x . w^T, scale, shift) + res)),  scale = gamma / sqrt(var + eps),
    shift = beta - mean * scale,

in its three epilogues (affine, relu, relu + residual) and both K regimes, through the binding,
and through ``Bottleneck`` in eval mode.  Shapes: M one row / one exact tile / a one-row last
tile / six tiles; K one stage / two stages (the short residual wait) / the weight-resident
limit / the first streaming K / more stages than the ring holds; N one and three columns.
Every M = 677 case runs again with the plan pinned to two CUs (a workgroup then walks several
tiles: ring and residual hand-over across tile boundaries) and must agree bitwise.

Worst error / bound ratios on an MI355X: profiles/r30_conv1x1_bn_eval/test_ratios.log.
"""
import functools

import pytest
import torch

from bn_reference import HALF_BF16, U, same_bf16, to_bf16
from ray_lightning_accelerators_amd.ops import conv as C

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 64), (128, 128, 192), (129, 160, 64), (129, 512, 64), (677, 32, 192), (677, 64, 64),
          (677, 128, 64), (677, 160, 192), (677, 512, 192)]
EPILOGUES = {"affine": (False, False), "relu": (True, False), "relu_res": (True, True)}


def _C():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


@functools.lru_cache(maxsize=None)
def _data(shape, kind):
    """CPU operands of one shape, made once.  ``int``: every fp32 intermediate of the kernel
    is exact (|acc| <= 16 K, scale in {+-0.5, +-1, +-2} as var = 1 and eps = 0, integer mean,
    beta and residual: multiples of 0.5 below 2^15)."""
    m, k, n = shape
    g = torch.Generator().manual_seed(m + 3 * k + 7 * n)
    sign = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
    if kind == "int":
        x = torch.randint(1, 5, (m, k), generator=g) * sign(m, k)
        w = torch.randint(1, 5, (n, k), generator=g) * sign(n, k)
        res = torch.randint(-64, 65, (m, n), generator=g).float()
        mean, beta = (torch.randint(-8, 9, (n,), generator=g).float() for _ in range(2))
        gamma = 2.0 ** torch.randint(-1, 2, (n,), generator=g).float() * sign(n)
        var, eps = torch.ones(n), 0.0
    else:
        x, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5
        res, mean, beta = torch.randn(m, n, generator=g), 0.5 * torch.randn(n, generator=g), torch.randn(n, generator=g)
        gamma = (0.5 + torch.rand(n, generator=g)) * sign(n)
        var, eps = 0.25 + 3.75 * torch.rand(n, generator=g), 1e-5
    return {"x": x.to(torch.bfloat16), "w": w.to(torch.bfloat16), "res": res.to(torch.bfloat16), "mean": mean,
            "var": var, "gamma": gamma, "beta": beta, "eps": eps}


def _reference(d, relu, with_res):
    """(out float64, bound): the formula in float64, and the element-wise bound of an fp32
    evaluation stored as bf16.  With u = 2^-24, A = sum_k |x||w| >= |acc|:
      * acc: K fp32 accumulations of exact products               -> K u A, times |scale|;
      * scale: var + eps, sqrt, division = 3 roundings            -> 3 u |acc scale|;
      * shift = fma(-mean, scale, beta): scale's 3 and its own    -> 4 u (|beta| + |mean scale|);
      * the fma and the residual add, one rounding each           -> 2 u (|acc scale| + |shift| + |res|);
    the ReLU does not grow an error, and the bf16 store adds half an ulp of the fp32 value,
    2^-8 (|out| + the above)."""
    s = lambda t: t.double()
    eps = float(torch.tensor(d["eps"], dtype=torch.float32))
    acc, absdot = s(d["x"]) @ s(d["w"]).T, s(d["x"]).abs() @ s(d["w"]).abs().T
    scale = s(d["gamma"]) / torch.sqrt(s(d["var"]) + eps)
    shift = s(d["beta"]) - s(d["mean"]) * scale
    res = s(d["res"]) if with_res else torch.zeros_like(acc)
    out = acc * scale + shift + res
    k = d["x"].size(1)
    err = U * (scale.abs() * k * absdot + 3 * (acc * scale).abs() + 4 * (s(d["beta"]).abs() + (s(d["mean"]) * scale).abs())
               + 2 * ((acc * scale).abs() + shift.abs() + res.abs()))
    out = torch.clamp(out, min=0.0) if relu else out
    return out, HALF_BF16 * out.abs() + (1 + HALF_BF16) * err


def _run(d, relu, with_res):
    dev = lambda t: t.cuda()
    return _C().conv1x1_bn_act(dev(d["x"]), dev(d["w"]), dev(d["mean"]), dev(d["var"]), dev(d["gamma"]),
                               dev(d["beta"]), d["eps"], relu, dev(d["res"]) if with_res else None)


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_fp64(shape, epi, kind):
    m, k, n = shape
    relu, with_res = EPILOGUES[epi]
    d = _data(shape, kind)
    out = _run(d, relu, with_res)
    assert out.shape == (m, n) and out.dtype == torch.bfloat16
    if m == 677:  # several tiles per workgroup: the same bits
        was = _C().plan_cus()
        _C().set_plan_cus(2)
        try:
            assert _C().conv1x1_bn_act_plan(m, k, n)["tiles_per_blk"] > 1
            pinned = _run(d, relu, with_res)
        finally:
            _C().set_plan_cus(0)
        assert _C().plan_cus() == was and torch.equal(pinned, out)
    ref, bound = _reference(d, relu, with_res)
    if kind == "int":
        assert bool(same_bf16(out.cpu(), to_bf16(ref)).all())
    else:
        ratio = ((out.double().cpu() - ref).abs() / bound).max().item()
        print(f"conv1x1_bn_act {shape} {epi}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("case", ["K=48", "N=96", "fp32_x", "short_res", "long_var", "res_no_relu"])
def test_refused_before_launch(case):
    m, k, n = 129, (48 if case == "K=48" else 64), (96 if case == "N=96" else 64)
    assert _C().conv1x1_bn_act_ok(m, k, n) == (case not in ("K=48", "N=96"))
    x = torch.zeros(m, k, device="cuda", dtype=torch.float32 if case == "fp32_x" else torch.bfloat16)
    w = torch.zeros(n, k, device="cuda", dtype=torch.bfloat16)
    vec = [torch.ones(n + (case == "long_var" and i == 1), device="cuda") for i in range(4)]
    res = torch.zeros(m - (case == "short_res"), n, device="cuda", dtype=torch.bfloat16)
    name = {"K=48": "unsupported shape", "N=96": "unsupported shape", "fp32_x": "conv1x1_bn_act: x",
            "short_res": "conv1x1_bn_act: res", "long_var": "conv1x1_bn_act: var", "res_no_relu": "residual"}[case]
    with pytest.raises(RuntimeError, match=name):
        _C().conv1x1_bn_act(x, w, *vec, 1e-5, case != "res_no_relu", res if "res" in case else None)


def _block(down):
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck, _bn, _conv1x1

    torch.manual_seed(5 + down)
    ds = torch.nn.Sequential(_conv1x1(256, 256, 1, fused=True), _bn(256, True, act=None)) if down else None
    blk = Bottleneck(256, 64, 1, ds, fused_bn=True).cuda().eval()
    for mod in blk.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.5)
            mod.running_var.uniform_(0.25, 4.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.5)
    return blk


def _block_fp64(blk, x):
    """The block in float64 from the bf16 weights, nothing rounded on the way."""
    F = torch.nn.functional

    def cb(conv, bn, t, relu):
        t = F.conv2d(t, conv.weight.detach().to(torch.bfloat16).double(), None, conv.stride, conv.padding)
        t = F.batch_norm(t, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(),
                         False, 0.0, bn.eps)
        return F.relu(t) if relu else t

    idt = x if blk.downsample is None else cb(blk.downsample[0], blk.downsample[1], x, False)
    t = cb(blk.conv2, blk.bn2, cb(blk.conv1, blk.bn1, x, True), True)
    return F.relu(cb(blk.conv3, blk.bn3, t, False) + idt)


@pytest.mark.parametrize("down", [True, False])
def test_block_eval(monkeypatch, down):
    """A Bottleneck in eval mode: the switch at 1 takes the fused route at every stride-1 1x1
    layer (3 with a stride-1 downsample conv, 2 without), at 0 or with a forward hook none,
    and those two agree bitwise (both run the modules' own forwards).  The fused route drops a
    rounding per layer: its rms error against float64 may not exceed the split route's by more
    than FACTOR.  Measured rms errors (MI355X): profiles/r30_conv1x1_bn_eval/test_ratios.log."""
    FACTOR = 1.05  # measured 0.92 (downsample) and 0.97 (identity): the margin is for another GEMM library build
    monkeypatch.setenv("RLA_CONV1X1", "gemm")  # one 1x1 backend for every run
    blk = _block(down)
    x = torch.randn(2, 256, 14, 14, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
    x = x.contiguous(memory_format=torch.channels_last)
    ref = _block_fp64(blk.double(), x.double()).cpu()
    blk.float()

    def run(mode):
        monkeypatch.setenv("RLA_CONV1X1_BN_EVAL", mode)
        before = C.stats["bn_eval_fused"]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y = blk(x)
        return y, C.stats["bn_eval_fused"] - before

    fused, n1 = run("1")
    split, n0 = run("0")
    hooks = [m.register_forward_hook(lambda *a: None) for m in blk.modules() if isinstance(m, C.Conv1x1NHWC)]
    hooked, nh = run("1")
    for h in hooks:
        h.remove()
    assert (n1, n0, nh) == (3 if down else 2, 0, 0)
    assert torch.equal(split, hooked) and fused.dtype == split.dtype == torch.bfloat16
    rms = lambda y: ((y.double().cpu() - ref) ** 2).mean().sqrt().item()
    print(f"bottleneck down={down}: rms error fused {rms(fused):.3e}, split {rms(split):.3e}, factor {FACTOR}")
    assert rms(fused) <= FACTOR * rms(split)
