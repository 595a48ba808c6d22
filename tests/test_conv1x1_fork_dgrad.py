"""The fused input gradient of a forked 1x1 pair (csrc/conv1x1_fork_dgrad.hip) on the raw binding
``conv1x1_fork_dgrad`` and through ``GradFork``, element by element against

  dx[n, h, w, :] = dy1[n, h, w, :] . w1  +  [h % s == 0 and w % s == 0] dyd[n, h/s, w/s, :] . wd

in float64 on the CPU (two matmuls and a strided add).

  * integer operands in {-2 .. 2}: 4 (C1 + Cd) < 2^24, so every fp32 sum is exact in any order
    and dx is the bf16 rounding of the float64 result bit for bit;
  * bf16 ``randn`` operands: no element past 2^-8 |ref| (one bf16 rounding) plus
    (C1 + Cd) 2^-24 A (1 + 2^-8), A = |dy1| . |w1| + strided(|dyd| . |wd|) (fp32 accumulation
    in any order), the form tests/test_conv1x1s2.py uses.
Worst error / bound ratio of the random cases on an MI355X: profiles/r29_fork_dgrad/test_ratios.log.
"""
import functools

import pytest
import torch

from ray_lightning_accelerators_amd.ops import conv as C

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, C1, Cd, s): one tile, one chunk per GEMM; 27 quads = a short tile that crosses two
# image boundaries; odd size (quads past the image), two column blocks, five wd chunks; 144 quads =
# more than one tile and a short last one; the stride-1 instance at M = 50; the same with three
# column blocks; and nine units (3 tiles x 3 column blocks), so that two workgroups each walk
# several units, one of them across a column-block change (test_plan_independent)
SHAPES = [(1, 4, 4, 64, 32, 32, 2), (3, 6, 6, 64, 64, 96, 2), (2, 7, 7, 128, 32, 160, 2), (1, 24, 24, 64, 96, 64, 2),
          (2, 5, 5, 64, 64, 256, 1), (1, 16, 16, 192, 128, 512, 1), (2, 24, 24, 192, 32, 64, 2)]


def _C():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


def _ref(dy1, w1, dyd, wd, s):
    out = dy1.double() @ w1.double()
    out[:, ::s, ::s] += dyd.double() @ wd.double()
    return out


@functools.lru_cache(maxsize=None)
def _data(shape, kind):
    """The four NHWC / [C, Cin] operands on the device, the float64 result and A; made once."""
    n, h, w, cin, c1, cd, s = shape
    g = torch.Generator().manual_seed(sum(shape))
    dims = [(n, h, w, c1), (c1, cin), (n, (h - 1) // s + 1, (w - 1) // s + 1, cd), (cd, cin)]
    if kind == "int":
        ops = [torch.randint(-2, 3, d, generator=g).to(torch.bfloat16) for d in dims]
    else:
        ops = [torch.randn(d, generator=g).to(torch.bfloat16) for d in dims]
    return [t.cuda() for t in ops], _ref(*ops, s), _ref(*[t.abs() for t in ops], s)


def _ratio(dx, shape, ref, absdot):
    c = shape[4] + shape[5]
    bound = 2.0 ** -8 * ref.abs() + c * 2.0 ** -24 * absdot * (1 + 2.0 ** -8)
    return ((dx.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_fp64(shape, kind):
    ops, ref, absdot = _data(shape, kind)
    dx = _C().conv1x1_fork_dgrad(*ops, shape[6])
    assert dx.shape == ref.shape and dx.dtype == torch.bfloat16
    if kind == "int":
        assert 4 * (shape[4] + shape[5]) < 2 ** 24
        assert torch.equal(dx.cpu(), ref.to(torch.bfloat16))
    else:
        ratio = _ratio(dx, shape, ref, absdot)
        print(f"conv1x1_fork_dgrad {shape}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("shape", SHAPES)
def test_plan_independent(shape):
    ops, _, _ = _data(shape, "randn")
    dx0 = _C().conv1x1_fork_dgrad(*ops, shape[6])
    assert torch.equal(_C().conv1x1_fork_dgrad(*ops, shape[6]), dx0)
    _C().set_plan_cus(2)
    try:
        plan = _C().conv1x1_fork_dgrad_plan(*shape)
        dx2 = _C().conv1x1_fork_dgrad(*ops, shape[6])
    finally:
        _C().set_plan_cus(0)
    assert plan["grid"] == min(2, plan["units"]) and plan["units"] == plan["tiles"] * plan["cols"]
    if shape == SHAPES[-1]:  # the others have at most three units
        assert plan["units"] // plan["grid"] >= 4
    assert torch.equal(dx2, dx0)


# channel counts in multiples of 64, which the pinned weight-gradient kernel needs
@pytest.mark.parametrize("shape", [(3, 6, 6, 64, 64, 128, 2), SHAPES[4]])
def test_through_grad_fork(monkeypatch, shape):
    n, h, w, cin, c1, cd, s = shape
    (dy1, w1, dyd, wd), ref, absdot = _data(shape, "randn")
    monkeypatch.setenv("RLA_CONV_WGRAD", "hip")  # fixed-order weight gradients for the bitwise comparison
    conv1 = C.Conv1x1NHWC(cin, c1).cuda()
    convd = (torch.nn.Conv2d(cin, cd, 1, 2, bias=False) if s == 2 else C.Conv1x1NHWC(cin, cd)).cuda()
    with torch.no_grad():
        conv1.weight.copy_(w1.view(c1, cin, 1, 1))
        convd.weight.copy_(wd.view(cd, cin, 1, 1))
    xh = torch.randn(n, h, w, cin, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()

    def run(mode):
        monkeypatch.setenv("RLA_FORK_DGRAD", mode)
        x = xh.permute(0, 3, 1, 2).detach().requires_grad_(True)
        conv1.weight.grad = convd.weight.grad = None
        fork, before = C.GradFork(), C.stats["fork_dgrad_fused"]
        if s == 2:
            wb = convd.weight.detach().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            yd = C.conv_nhwc(x, convd, wb, fork=fork)
        else:
            yd = convd(x, fork=fork)
        y1 = conv1(x, fork=fork)
        loss = (y1.float() * dy1.permute(0, 3, 1, 2).float()).sum() + (yd.float() * dyd.permute(0, 3, 1, 2).float()).sum()
        loss.backward()
        return x.grad.permute(0, 2, 3, 1), conv1.weight.grad, convd.weight.grad, C.stats["fork_dgrad_fused"] - before

    gx, g1, gd, used = run("1")
    assert used == 1 and _ratio(gx, shape, ref, absdot) <= 1.0
    assert torch.equal(gx, _C().conv1x1_fork_dgrad(dy1, w1, dyd, wd, s))
    gx0, g10, gd0, used0 = run("0")
    assert used0 == 0 and torch.equal(g1, g10) and torch.equal(gd, gd0)
    assert gx0.shape == gx.shape


@pytest.mark.parametrize("case", ["fp32", "noncontiguous", "wd_cin", "dyd_oh", "s3"])
def test_refused_before_launch(case):
    n, h, w, cin, c1, cd = 2, 6, 6, 64, 32, 64
    z = lambda *d, dt=torch.bfloat16: torch.zeros(*d, device="cuda", dtype=dt)
    dy1, w1, dyd, wd, s = z(n, h, w, c1), z(c1, cin), z(n, 3, 3, cd), z(cd, cin), 2
    if case == "fp32":
        dyd = z(n, 3, 3, cd, dt=torch.float32)
    elif case == "noncontiguous":
        dy1 = z(n, c1, h, w).permute(0, 2, 3, 1)
    elif case == "wd_cin":
        wd = z(cd, 128)
    elif case == "dyd_oh":
        dyd = z(n, 4, 3, cd)
    else:
        s = 3
    name = {"fp32": "dyd has dtype", "noncontiguous": "dy1 must be contiguous", "wd_cin": "wd has 128 input channels",
            "dyd_oh": "dyd must be", "s3": "stride must be 1 or 2"}[case]
    with pytest.raises(RuntimeError, match="conv1x1_fork_dgrad: " + name):
        _C().conv1x1_fork_dgrad(dy1, w1, dyd, wd, s)
