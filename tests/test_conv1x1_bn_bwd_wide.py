"""conv1x1_bn_bwd_wide (csrc/conv1x1_bn_bwd_wide.hip): the 1x1 input gradient at 128 < K <= 512
fused with the previous BatchNorm's backward partial pass, against fp64:

    da = bf16(dy1 . w),  d = bf16(yb > 0 ? da + dy2 : 0),  part[row] = (sum d, sum d * xb)

Exact cases use dyadic operands for which every intermediate is exact (bit-for-bit equality);
random cases are held to a bound derived from the formats alone: bf16 rounds to nearest with
relative error 2^-8, fp32 with 2^-24, the MFMA sum of K terms is within K 2^-24 sum|dy1||w|.
Worst error / bound ratio of the random cases on an MI355X:
profiles/r28_conv1x1_bn_bwd_wide/test_ratios.log."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U8, U24 = 2.0 ** -8, 2.0 ** -24
# one short tile, K % 64 != 0, one column block | several tiles, short last, ragged group |
# maximum K, two groups, the second ragged | the production (K, N) at two images
SMALL = [(77, 160, 64), (1000, 256, 192), (300, 512, 320)]
EXACT = [(s, 0) for s in SMALL] + [((392, 256, 1024), 0), ((98, 512, 2048), 0), ((659, 256, 512), 2)]


def _ops():
    from ray_lightning_accelerators_amd.ops import require

    return require()


def _reference(dy1, w, dy2, yb):
    da = dy1.double() @ w.double()
    return da, torch.where(yb > 0, da + dy2.double(), torch.zeros_like(da))


def _row_sums(d, xb, plan):
    dd, xx = d.double(), xb.double()
    return torch.stack([torch.stack([dd[lo:hi].sum(0), (dd[lo:hi] * xx[lo:hi]).sum(0)]) for lo, hi in plan["row_ranges"]])


@pytest.mark.parametrize("shape,cus", EXACT)
def test_exact(shape, cus):
    m, k, n = shape
    mod, dev = _ops(), torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(m + k + n)
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    dy1 = bf(torch.randint(-1, 2, (m, k), generator=g))
    nz = torch.rand(k, n, generator=g).argsort(0).argsort(0) < 64  # 64 non-zeros of +-1 per column
    w = bf(nz * (2 * torch.randint(0, 2, (k, n), generator=g) - 1))
    dy2 = bf(torch.randint(-64, 65, (m, n), generator=g))
    yb = bf(torch.randint(-2, 3, (m, n), generator=g))
    xb = bf(torch.randint(-4, 5, (m, n), generator=g))
    try:
        mod.set_plan_cus(cus)
        plan = mod.conv1x1_bn_bwd_wide_plan(m, k, n)
        d, part = mod.conv1x1_bn_bwd_wide(dy1, w, dy2, yb, xb)
        torch.cuda.synchronize()
    finally:
        mod.set_plan_cus(0)
    if cus:
        assert plan["units"] > plan["grid"]  # workgroups walk several units
    assert plan["row_ranges"][0][0] == 0 and plan["row_ranges"][-1][1] == m and len(plan["row_ranges"]) == plan["rows"]
    _, ref = _reference(dy1, w, dy2, yb)
    assert d.dtype == torch.bfloat16 and part.dtype == torch.float32 and tuple(part.shape) == (plan["rows"], 2, n)
    assert torch.equal(d.double(), ref)
    assert torch.equal(part.double(), _row_sums(ref, xb, plan))


@pytest.mark.parametrize("shape", SMALL)
def test_random_within_format_bounds(shape):
    m, k, n = shape
    mod, dev = _ops(), torch.device("cuda", 0)
    torch.manual_seed(k + n)
    dy1, w = (torch.randn(s, device=dev).to(torch.bfloat16) for s in ((m, k), (k, n)))
    dy2, yb, xb = (torch.randn(m, n, device=dev).to(torch.bfloat16) for _ in range(3))
    plan = mod.conv1x1_bn_bwd_wide_plan(m, k, n)
    d, part = mod.conv1x1_bn_bwd_wide(dy1, w, dy2, yb, xb)
    d2, part2 = mod.conv1x1_bn_bwd_wide(dy1, w, dy2, yb, xb)
    assert torch.equal(d, d2) and torch.equal(part, part2)
    assert bool(torch.isfinite(d.float()).all()) and bool(torch.isfinite(part).all())
    da, ref = _reference(dy1, w, dy2, yb)
    # s = the fp32 sum, da' = bf16(s), a = fp32(da' + dy2), d = bf16(a)
    e_s = k * U24 * (dy1.double().abs() @ w.double().abs())
    e_da = e_s + U8 * (da.abs() + e_s)
    a_mag = (da + dy2.double()).abs() + e_da
    bound = e_da + (U8 + U24) * a_mag * (1 + U24)
    err = (d.double() - ref).abs()
    assert bool((d[yb <= 0] == 0).all())
    assert bool((err[yb <= 0] == 0).all())
    r_d = float((err / bound.clamp_min(1e-300)).max())
    # part against fp64 sums of the kernel's own d: fp32 adds of `rows` terms per channel
    dd, xx = d.double(), xb.double()
    terms = torch.stack([torch.stack([dd[lo:hi].abs().sum(0), (dd[lo:hi] * xx[lo:hi]).abs().sum(0)]) * (hi - lo)
                         for lo, hi in plan["row_ranges"]])
    perr = (part.double() - _row_sums(d, xb, plan)).abs()
    r_p = float(torch.where(perr > 0, perr / (U24 * terms).clamp_min(1e-300), torch.zeros_like(perr)).max())
    print(f"[bound ratio] conv1x1_bn_bwd_wide {shape}: d {r_d:.3f} part {r_p:.3f}")
    assert r_d < 1.0 and r_p < 1.0, (r_d, r_p)


@pytest.mark.parametrize("k,n", [(128, 256), (200, 256), (544, 256), (256, 96)])
def test_refused_shapes(k, n):
    mod, dev = _ops(), torch.device("cuda", 0)
    assert not mod.conv1x1_bn_bwd_wide_ok(256, k, n)
    t = lambda *s: torch.zeros(s, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        mod.conv1x1_bn_bwd_wide(t(256, k), t(k, n), t(256, n), t(256, n), t(256, n))
    with pytest.raises(RuntimeError):
        mod.conv1x1_bn_bwd_wide_plan(256, k, n)


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("fault", ["strided", "fp32", "shape"])
def test_refused_operands(which, fault):
    mod, dev = _ops(), torch.device("cuda", 0)
    m, k, n = 130, 256, 128
    assert mod.conv1x1_bn_bwd_wide_ok(m, k, n)
    ops = [torch.zeros(s, device=dev, dtype=torch.bfloat16) for s in ((m, k), (k, n), (m, n), (m, n), (m, n))]
    t = ops[which]
    if fault == "strided":
        t = torch.zeros(t.size(0), 2 * t.size(1), device=dev, dtype=torch.bfloat16)[:, ::2]
    elif fault == "fp32":
        t = t.float()
    else:
        t = torch.zeros(t.size(0) + 1, t.size(1), device=dev, dtype=torch.bfloat16)
    ops[which] = t
    with pytest.raises(RuntimeError):
        mod.conv1x1_bn_bwd_wide(*ops)


def _step(blocks, x0):
    blocks.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = blocks(x)
    y.float().square().mean().backward()
    return y.detach().float(), x.grad.float(), [p.grad.detach().float().clone() for p in blocks.parameters()]


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def block_runs():
    """ResNet-50 layer3[1:3], two identity blocks (1024 -> 256 at 14 x 14): the first one's output
    carries the fold that the second one's conv1 absorbs on the wide kernel (the first one's own input
    is a plain tensor: nothing to absorb).  The weights are read from the arena's bf16 shadow, as
    in training, and the 3x3 forward is pinned to the in-tree kernel, so every forward has a fixed
    summation order: the library's convolutions (stock conv2d without the shadow, or layer3[0]'s
    stride-2 candidates) are not repeatable run to run at this batch, which would hide what the
    bitwise check is for.  One step with RLA_FUSE_BN_DGRAD_WIDE=0 and one with 1: (outputs, counter
    advance, folds) of each."""
    from ray_lightning_accelerators_amd.models.resnet import resnet50
    from ray_lightning_accelerators_amd.ops import bn as B
    from ray_lightning_accelerators_amd.ops import conv as C

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    blocks = resnet50(num_classes=10, fused_bn=True).to(dev).to(memory_format=torch.channels_last).layer3[1:3]
    x0 = torch.randn(4, 1024, 14, 14, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    from ray_lightning_accelerators_amd.parallel.arena import ParamArena

    blocks.arena = ParamArena(blocks)  # kept alive with the blocks: the shadow registry holds it weakly
    blocks.arena.enable_bf16_shadow(blocks)
    runs = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RLA_CONV3X3_PRE", "pre")
        for fuse in ("0", "1"):
            mp.setenv("RLA_FUSE_BN_DGRAD_WIDE", fuse)
            n0, f0 = C.stats["bn_dgrad_fused_wide"], B.fold_stats["folded"]
            out = _step(blocks, x0)
            runs.append((out, C.stats["bn_dgrad_fused_wide"] - n0, B.fold_stats["folded"] - f0))
    return blocks, x0, runs


def test_identity_block_forward_bitwise(block_runs):
    """The switch only changes the backward."""
    (y0, _, _), (y1, _, _) = block_runs[2][0][0], block_runs[2][1][0]
    assert torch.equal(y0, y1)


def test_identity_block_gradients_and_counters(block_runs):
    (out0, n0, f0), (out1, n1, f1) = block_runs[2]
    assert (n0, n1) == (0, 1)  # the one identity block whose input carries a fold
    assert f0 == f1
    assert _rel(out1[1], out0[1]) < 2e-2, _rel(out1[1], out0[1])
    for a, b in zip(out1[2], out0[2]):
        assert _rel(a, b) < 3e-2, _rel(a, b)


def test_identity_block_deterministic_mode(block_runs, monkeypatch):
    """Switch unset: the fixed-order kernel runs untimed and two backward passes are bitwise equal."""
    from ray_lightning_accelerators_amd.ops import conv as C

    blocks, x0, _ = block_runs
    monkeypatch.delenv("RLA_FUSE_BN_DGRAD_WIDE", raising=False)
    monkeypatch.setenv("RLA_CONV3X3_PRE", "pre")  # as in the fixture: not a timed pick
    picks, n0 = dict(C._choice), C.stats["bn_dgrad_fused_wide"]
    torch.use_deterministic_algorithms(True)
    try:
        a, b = _step(blocks, x0), _step(blocks, x0)
    finally:
        torch.use_deterministic_algorithms(False)
    assert C._choice == picks and C.stats["bn_dgrad_fused_wide"] - n0 == 2
    assert torch.equal(a[1], b[1]) and all(torch.equal(u, v) for u, v in zip(a[2], b[2]))
