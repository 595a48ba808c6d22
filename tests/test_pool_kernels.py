"""csrc/pool.hip and csrc/pool_gather.h against the float64 references of
tests/bn_reference.py: the pooled values, the argmax bytes and the gathering backward are
exact operations on bf16 data, so everything here is compared bitwise -- except the
pooled BatchNorm backward's fp32 sums and dx, which have the stage tests' bounds.

Geometries beyond k >= s (the launchers take any 1 <= k <= 15, s >= 1, 2 pad <= k), H != W,
trailing rows and columns no window covers (their gradient is exactly 0), ties inside and
across windows, a constant plane, NaN, -inf (windows of nothing else included), and for
the BN-folded form a negative scale: not monotone, with many ties at 0 after the ReLU."""
import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu
WORST = {}


def _mod():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


def _gpu(op):
    return {n: (v.cuda() if torch.is_tensor(v) else v) for n, v in op.items()}


def _ok(what, case, c):
    torch.cuda.synchronize()
    print(f"{what} {case}: {c.detail}")
    WORST[what] = max(WORST.get(what, 0.0), c.ratio)
    assert c.ok, f"{what} {case}: {c.detail}"


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("geo", R.POOL_GEOMETRIES, ids=str)
def test_maxpool_forward_and_backward(geo, C):
    k, s, pad = geo
    N, H, W = R.pool_shape(k, s, pad, C)
    OH, OW = R.pool_out(H, W, k, s, pad)
    assert H != W and (N * OH * OW * (C // 8)) % 256 and (N * H * W * (C // 8)) % 256
    x = R.make_pool_x(N, H, W, C, seed=10 * k + s).cuda()
    y, arg = _mod().maxpool_fwd(x, k, s, pad)
    want_y, want_arg = R.pool_expected(x, k, s, pad)
    _ok("maxpool_fwd y", (geo, C), R.cmp_exact(y, want_y))
    _ok("maxpool_fwd argmax", (geo, C), R.cmp_exact(arg, want_arg))
    dy = R.make_pool_dy((N, OH, OW, C), seed=k).cuda()
    dx = _mod().maxpool_bwd(dy, want_arg, H, W, k, s, pad)
    # sums of i / 64 are exact in fp32 and float64 alike: one rounding, the store's
    want_dx = R.to_bf16(R.ref_maxpool_bwd(dy, want_arg, H, W, k, s, pad))
    _ok("maxpool_bwd", (geo, C), R.cmp_exact(dx, want_dx))
    # rows / columns past the last window, and the gaps between windows when k < s
    eh, ew = (OH - 1) * s - pad + k, (OW - 1) * s - pad + k
    assert not bool(dx[:, eh:].any()) and not bool(dx[:, :, ew:].any())
    if k < s:
        gap = torch.tensor([(h + pad) % s >= k for h in range(H)], device="cuda")
        assert bool(gap.any()) and not bool(dx[:, gap].any())


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("geo", R.POOL_GEOMETRIES, ids=str)
def test_maxpool_bn_folded(geo, C):
    """bf16(relu(x * scale + shift)) pooled in one pass, for stats that make the map exact
    in fp32 (asserted): the values and the bytes have no rounding freedom."""
    k, s, pad = geo
    op = _gpu(R.pooled_operands(geo, C, R.pool_shape(k, s, pad, C)))
    R.assert_exact_affine(op["x"], op["ss"])
    assert bool((op["ss"][2] < 0).any()) and bool((op["ss"][2] > 0).any())
    nbt = torch.tensor([4], dtype=torch.int64, device="cuda")
    y, arg = _mod().maxpool_fwd(op["x"], k, s, pad, op["ss"].contiguous(), nbt)
    _ok("maxpool_fwd BN y", (geo, C), R.cmp_exact(y, op["y"]))
    _ok("maxpool_fwd BN argmax", (geo, C), R.cmp_exact(arg, op["arg"]))
    assert int(nbt) == 5


@pytest.mark.parametrize("geo,C,shape", R.POOLED_BN_CASES, ids=str)
def test_pooled_bn_backward(geo, C, shape):
    """The stem's BatchNorm backward, whose dy is gathered from the pooled gradient through
    the argmax bytes: bn_partial_kernel<1,true,false,true,false,true> and
    bn_bwd_apply_kernel<true,false,false,true,true> against the reference chain (float64
    scatter rounded to bf16, then the stage formulas)."""
    op = _gpu(R.pooled_operands(geo, C, shape))
    R.assert_exact_affine(op["x"], op["ss"])
    M = op["x"].numel() // C
    rpb, blocks = R.bn_plan(M, C)
    ss = op["ss"].contiguous()
    part = _mod().bn_partial(op["x"], None, op["dyp"], C, 1, True, None, None, ss, None, op["arg"], op["geo"])
    assert part.shape == (blocks, 2, C)
    S, A, n, coef, dx_ref, mag, _ = R.pooled_reference(op, rpb)
    _ok("bn_partial pooled", (geo, C, shape), R.cmp_part(part, S, A, n))
    dx = torch.full_like(op["x"], 7.0)
    _mod().bn_bwd_apply(op["x"], None, op["dyp"], coef.contiguous(), True, dx, None, None, ss, op["arg"], op["geo"])
    _ok("bn_bwd_apply pooled", (geo, C, shape), R.cmp_bf16(dx.reshape(-1, C), dx_ref, mag))


@pytest.mark.parametrize("N,C,HW", [(3, 8, 64), (5, 24, 16), (2, 2048, 4), (37, 136, 1)])
def test_gap_backward_power_of_two_is_exact(N, C, HW):
    g = torch.Generator().manual_seed(N + C)
    dy = torch.randn(N, C, generator=g).to(torch.bfloat16).cuda()
    dx = _mod().gap_bwd(dy, HW)
    _ok("gap_bwd", (N, C, HW), R.cmp_exact(dx, R.to_bf16(R.ref_gap_bwd(dy, HW))))


@pytest.mark.parametrize("N,C,HW", [(5, 24, 49), (3, 64, 7)])
def test_gap_backward(N, C, HW):
    g = torch.Generator().manual_seed(N + C)
    dy = torch.randn(N, C, generator=g).to(torch.bfloat16).cuda()
    dx = _mod().gap_bwd(dy, HW)
    ref = R.ref_gap_bwd(dy, HW)
    # dy * (float)(1 / HW): the reciprocal's rounding and the product's, k = 2 (+ 1 spare)
    _ok("gap_bwd", (N, C, HW), R.cmp_bf16(dx, ref, ref.abs(), k=3))


def test_zz_worst_ratios():
    for what, r in sorted(WORST.items()):
        print(f"WORST {what}: error / bound {r:.3g}")
    assert all(r <= 1.0 for r in WORST.values())
