"""The float64 references of tests/bn_reference.py are right, and the comparisons the GPU
stage tests make with them are sharp -- both shown without a GPU.

Right: the chained stage functions reproduce float64 autograd of F.batch_norm (+ residual,
ReLU, max pool), and the pool reference's argmax byte is F.max_pool2d's index.
Sharp: an fp32 emulation of each stage (torch float32 arithmetic, bf16 store) passes the
comparison functions on the GPU tests' inputs, and each deliberately wrong variant of it
-- biased running_var, a >= mask, a truncating bf16 store, Cc without / count, the last
maximum winning a tie, a dropped final row, nbt_pending ignored -- is rejected."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_reference as R

CPU_MAX = 600_000  # elements: the emulations of larger cases add minutes and no new path


def _rows(t):  # NCHW -> [M, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows, like):
    N, C, H, W = like.shape
    return rows.reshape(N, H, W, C).permute(0, 3, 1, 2)


# ------------------------------------------------------------------ the oracle is right
def test_round_bf16_is_direct_round_to_nearest_even():
    v = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8 + 2.0 ** -30),
                      3.4e38, 1e-40, 2.0 ** -134, 2.0 ** -134 * 1.01, math.inf, -0.0], dtype=torch.float64)
    want = torch.tensor([1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6, -(1 + 2.0 ** -7), math.inf, 2.0 ** -133, 0.0, 2.0 ** -133,
                         math.inf, -0.0], dtype=torch.float64)
    assert torch.equal(R.round_bf16(v), want)
    assert math.isnan(float(R.round_bf16(torch.tensor([math.nan], dtype=torch.float64))))
    # through fp32 the first value is double-rounded to 1.0: the reason for the explicit code
    assert float(v[:1].float().to(torch.bfloat16)) == 1.0
    g = torch.Generator().manual_seed(0)
    f = torch.randn(200_000, generator=g) * torch.logspace(-44, 38, 200_000)
    assert torch.equal(R.round_bf16(f.double()), f.to(torch.bfloat16).double())  # fp32 inputs: torch's own RNE
    t = R.round_bf16(f.double(), truncate=True)
    assert bool((t.abs() <= f.double().abs()).all()) and not torch.equal(t, R.round_bf16(f.double()))


@pytest.mark.parametrize("relu,with_res", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("momentum", [0.1, None])
def test_stage_chain_matches_float64_autograd(relu, with_res, momentum):
    g = torch.Generator().manual_seed(3)
    N, C, H, W = 3, 16, 5, 7
    x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_()
    res = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).requires_grad_() if with_res else None
    gamma = (torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_()
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    rm0, rv0 = torch.randn(C, generator=g, dtype=torch.float64), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    rm, rv, nbt, eps = rm0.clone(), rv0.clone(), 4, 1e-5
    # torch: num_batches_tracked += 1, then factor 1 / num_batches_tracked
    y = F.batch_norm(x, rm, rv, gamma, beta, True, 1.0 / nbt if momentum is None else momentum, eps)
    y = y + res if with_res else y
    y = F.relu(y) if relu else y
    dy = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    y.backward(dy)

    xr, count = _rows(x.detach()), float(N * H * W)
    S, _, _ = R.ref_partial_fwd(xr, rpb=17)
    st, nrm, nrv, _ = R.ref_finalize(S, count, gamma.detach(), beta.detach(), rm0, rv0, nbt,
                                     -1.0 if momentum is None else momentum, eps)
    eps32 = abs(float(torch.tensor(eps, dtype=torch.float32)) - eps)  # the kernel's eps is an fp32 value
    tol = 1e-10 + 10 * eps32
    yr, _ = R.ref_apply(xr, st[2], st[3], _rows(res.detach()) if with_res else None, relu)
    assert torch.allclose(_nchw(yr, x), y.detach(), atol=tol, rtol=0)
    if momentum is not None:  # fp32 momentum 0.1f differs from 0.1 by 1.5e-9
        assert torch.allclose(nrm, rm, atol=1e-7, rtol=0) and torch.allclose(nrv, rv, atol=1e-7, rtol=0)
    else:
        assert torch.allclose(nrm, rm, atol=tol, rtol=0) and torch.allclose(nrv, rv, atol=tol, rtol=0)

    d, Sb, _, _ = R.ref_partial_bwd(xr, _rows(dy), y=yr, relu=relu, rpb=17)
    coef, _ = R.ref_bwd_finalize(Sb, count, gamma.detach(), st[0], st[1])
    dx, _ = R.ref_bwd_apply(xr, d, coef)
    assert torch.allclose(_nchw(dx, x), x.grad, atol=tol, rtol=0)
    assert torch.allclose(coef[0], gamma.grad, atol=tol, rtol=0)
    assert torch.allclose(coef[1], beta.grad, atol=tol, rtol=0)
    if with_res:
        assert torch.allclose(_nchw(d, x), res.grad, atol=tol, rtol=0)


def test_finalize_reference_unbiased_count_one_and_pending():
    part = torch.tensor([[[2.0], [4.5]]], dtype=torch.float64)
    st, rm, rv, _ = R.ref_finalize(part, 1.0, None, None, torch.zeros(1), torch.ones(1), 1, -1.0, 1e-5, 1)
    assert float(st[0]) == 2.0 and abs(float(rv) - (0.5 * 1.0 + 0.5 * 0.5)) < 1e-15  # var 0.5 kept biased, 1 / (1 + 1)
    assert abs(float(rm) - 1.0) < 1e-15


@pytest.mark.parametrize("geo", [(3, 2, 1), (2, 3, 0), (5, 3, 2)])
def test_pooled_chain_matches_float64_autograd(geo):
    k, s, pad = geo
    g = torch.Generator().manual_seed(5)
    N, C, H, W = 2, 8, 11, 13
    x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_()
    gamma = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_()
    yp = F.max_pool2d(F.relu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, 1e-5)), k, s, pad)
    dyp = torch.randn(yp.shape, generator=g, dtype=torch.float64)
    yp.backward(dyp)
    xr, count = _rows(x.detach()), float(N * H * W)
    S, _, _ = R.ref_partial_fwd(xr)
    st, _, _, _ = R.ref_finalize(S, count, gamma.detach(), beta.detach(), None, None, None, 0.1, 1e-5)
    act, _ = R.ref_apply(xr, st[2], st[3], None, True)
    m, arg = R.ref_maxpool(act.reshape(N, H, W, C), k, s, pad)
    assert torch.allclose(m.permute(0, 3, 1, 2), yp.detach(), atol=1e-9, rtol=0)
    dfull = R.ref_maxpool_bwd(dyp.permute(0, 2, 3, 1), arg, H, W, k, s, pad).reshape(-1, C)
    d, Sb, _, _ = R.ref_partial_bwd(xr, dfull, ss=st, relu=True)
    coef, _ = R.ref_bwd_finalize(Sb, count, gamma.detach(), st[0], st[1])
    dx, _ = R.ref_bwd_apply(xr, d, coef)
    assert torch.allclose(_nchw(dx, x), x.grad, atol=1e-9, rtol=0)
    assert torch.allclose(coef[0], gamma.grad, atol=1e-9, rtol=0)
    assert torch.allclose(coef[1], beta.grad, atol=1e-9, rtol=0)


@pytest.mark.parametrize("geo", R.POOL_GEOMETRIES)
@pytest.mark.parametrize("C", [8, 24])
def test_pool_reference_byte_is_torch_index(geo, C):
    """On the GPU tests' own data: ties, a constant plane, NaN, windows of -inf only."""
    k, s, pad = geo
    N, H, W = R.pool_shape(k, s, pad, C)
    x = R.make_pool_x(N, H, W, C, seed=10 * k + s)
    m, arg = R.ref_maxpool(x, k, s, pad)
    xn = x.double().permute(0, 3, 1, 2).contiguous()
    want, _ = F.max_pool2d(xn, k, s, pad, return_indices=True)
    assert torch.equal(torch.nan_to_num(m.permute(0, 3, 1, 2), nan=123.0), torch.nan_to_num(want, nan=123.0))
    assert torch.equal(arg.permute(0, 3, 1, 2), R.torch_pool_bytes(xn, k, s, pad))
    # and the scatter is autograd's, on finite data
    xf = torch.nan_to_num(x.double(), nan=0.25, neginf=-9.0).permute(0, 3, 1, 2).contiguous().requires_grad_()
    yf = F.max_pool2d(xf, k, s, pad)
    dy = R.make_pool_dy(tuple(yf.permute(0, 2, 3, 1).shape), seed=k).double()
    yf.backward(dy.permute(0, 3, 1, 2))
    _, argf = R.ref_maxpool(xf.detach().permute(0, 2, 3, 1), k, s, pad)
    assert torch.equal(R.ref_maxpool_bwd(dy, argf, H, W, k, s, pad), xf.grad.permute(0, 2, 3, 1))


# ------------------------------------------------------------------ the comparisons are sharp
def _cpu(cases):
    return [c for c in cases if c[0] * c[1] <= CPU_MAX]


@pytest.mark.parametrize("C,M", _cpu(R.FWD_PARTIAL_CASES))
def test_forward_partial_comparison_rejects_dropped_row(C, M):
    x = R.make_rows(C, M, R.case_seed(C, M))["x"]
    rpb, _ = R.bn_plan(M, C)
    S, A, n = R.ref_partial_fwd(x, rpb)
    xf = x.float()
    good = R.cmp_part(R.emu_partial(xf, xf * xf, rpb), S, A, n)
    assert good.ok, good.detail
    assert not R.cmp_part(R.emu_partial(xf, xf * xf, rpb, drop_last=True), S, A, n).ok
    # block ranges unknown (another block count): the totals are compared instead
    one = R.emu_partial(xf, xf * xf, M)
    assert R.cmp_part(one, S, A, n).ok
    assert not R.cmp_part(R.emu_partial(xf, xf * xf, M, drop_last=True), S, A, n).ok


@pytest.mark.parametrize("variant", R.BWD_PARTIAL_VARIANTS, ids=str)
@pytest.mark.parametrize("C,M", _cpu(R.BWD_PARTIAL_CASES))
def test_backward_partial_comparison_rejects_ge_mask_and_dropped_row(C, M, variant):
    mask, dy2, wd = variant
    inp = R.bwd_operands(C, M, mask)
    if mask == "ss":
        R.assert_exact_affine(inp["x"], inp["ss"])
    s2 = inp["dy"].double() + inp["dy2"].double()
    assert torch.equal(s2.float().double(), s2)  # dy + dy2 is exact in fp32, so dout is bitwise
    rpb, _ = R.bn_plan(M, C)

    def emu(ge=False, drop=False, trunc=False):
        d = R.emu_masked_d(inp["x"], inp["dy"], inp["dy2"] if dy2 else None, inp["y"] if mask == "y" else None,
                           inp["ss"] if mask == "ss" else None, mask is not None, ge)
        dout = R.emu_store(d, trunc) if wd else None
        if wd:
            d = dout.float()
        return R.emu_partial(d, d * inp["x"].float(), rpb, drop), dout

    good = R.check_partial_bwd(*emu(), inp, variant, rpb)
    assert good.ok, good.detail
    assert not R.check_partial_bwd(*emu(drop=True), inp, variant, rpb).ok
    if mask is not None:
        act = inp["y"].double() if mask == "y" else inp["x"].double() * inp["ss"][2].double() + inp["ss"][3].double()
        if bool(((act == 0) & (s2 != 0)).any()):  # the inputs hold exact zeros of the activation
            assert not R.check_partial_bwd(*emu(ge=True), inp, variant, rpb).ok
    if wd and dy2:
        assert not R.check_partial_bwd(*emu(trunc=True), inp, variant, rpb).ok


def test_backward_inputs_hold_exact_zero_activations():
    """The >= mask is only distinguishable where the activation is exactly 0."""
    for mask in ("y", "ss"):
        inp = R.bwd_operands(64, 16 * 32 + 3, mask)
        act = inp["y"].double() if mask == "y" else inp["x"].double() * inp["ss"][2].double() + inp["ss"][3].double()
        assert int((act == 0).sum()) >= 8


@pytest.mark.parametrize("relu,with_res", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("C,M", _cpu(R.APPLY_CASES))
def test_apply_comparison_rejects_truncation_and_dropped_row(C, M, relu, with_res):
    inp = R.make_rows(C, M, R.case_seed(C, M))
    scale, shift = R.apply_coefficients(inp)
    res = inp["res"] if with_res else None
    ref, mag = R.ref_apply(inp["x"], scale, shift, res, relu)
    good = R.cmp_bf16(R.emu_apply(inp["x"], scale, shift, res, relu), ref, mag)
    assert good.ok, good.detail
    assert not R.cmp_bf16(R.emu_apply(inp["x"], scale, shift, res, relu, truncate=True), ref, mag).ok
    if bool((ref[-1] != 0).any()):
        assert not R.cmp_bf16(R.emu_apply(inp["x"], scale, shift, res, relu, drop_last=True), ref, mag).ok




@pytest.mark.parametrize("variant", R.BWD_APPLY_VARIANTS, ids=str)
@pytest.mark.parametrize("C,M", _cpu(R.APPLY_CASES))
def test_backward_apply_comparison_rejects_wrong_variants(C, M, variant):
    mask, dy2, dr = variant
    inp = R.bwd_operands(C, M, mask)
    coef = R.bwd_coefficients(inp, M, variant)

    def emu(ge=False, trunc=False):
        d = R.emu_masked_d(inp["x"], inp["dy"], inp["dy2"] if dy2 else None, inp["y"] if mask == "y" else None,
                           inp["ss"] if mask == "ss" else None, mask is not None, ge)
        return R.emu_bwd_apply(inp["x"], d, coef, trunc), (R.emu_store(d) if dr else None)

    good = R.check_bwd_apply(*emu(), inp, coef, variant)
    assert good.ok, good.detail
    assert not R.check_bwd_apply(*emu(trunc=True), inp, coef, variant).ok
    if mask is not None:
        act = inp["y"].double() if mask == "y" else inp["x"].double() * inp["ss"][2].double() + inp["ss"][3].double()
        d0 = inp["dy"].double() + (inp["dy2"].double() if dy2 else 0)
        if bool(((act == 0) & (d0 != 0)).any()):
            assert not R.check_bwd_apply(*emu(ge=True), inp, coef, variant).ok


@pytest.mark.parametrize("momentum,pending", R.FIN_MOMENTA)
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("nparts,C", R.FIN_CASES)
def test_finalize_comparison_rejects_biased_var_and_ignored_pending(nparts, C, affine, momentum, pending):
    for count in R.FIN_COUNTS:
        part, gamma, beta, rm, rv, nbt = R.finalize_operands(nparts, C, count, affine)
        args = (part, count, gamma, beta, rm, rv, nbt, momentum, 1e-5, pending)
        good = R.check_finalize(*R.emu_finalize(*args), *args)
        assert good.ok, good.detail
        clamped = R.ref_finalize(*args)[0][1][0]
        assert abs(float(clamped) - 1 / math.sqrt(float(torch.tensor(1e-5, dtype=torch.float32)))) < 1e-9  # channel 0
        if momentum != 0.0 and count > 1.0:
            assert not R.check_finalize(*R.emu_finalize(*args, biased=True), *args).ok
        if pending:
            assert not R.check_finalize(*R.emu_finalize(*args, ignore_pending=True), *args).ok



@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("nparts,C", R.FIN_CASES)
def test_backward_finalize_comparison_rejects_cc_without_count(nparts, C, affine):
    part, mean, invstd = R.make_bwd_parts(nparts, C, 17 * nparts + C)
    gamma = R.finalize_operands(nparts, C, 50.0, affine)[1]
    for count in (50.0, 100352.0):
        emu = R.emu_bwd_finalize(part, count, gamma, mean, invstd)
        good = R.check_bwd_finalize(emu, part, count, gamma, mean, invstd)
        assert good.ok, good.detail
        bad = R.emu_bwd_finalize(part, count, gamma, mean, invstd, cc_no_count=True)
        assert not R.check_bwd_finalize(bad, part, count, gamma, mean, invstd).ok
        one_percent = R.emu_bwd_finalize(part, count, gamma, mean, invstd)
        one_percent[3] *= 1.01
        assert not R.check_bwd_finalize(one_percent, part, count, gamma, mean, invstd).ok


@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("geo", R.POOL_GEOMETRIES)
def test_pool_comparison_rejects_last_maximum(geo, folded):
    k, s, pad = geo
    C = 24
    N, H, W = R.pool_shape(k, s, pad, C)
    x = R.make_pool_x(N, H, W, C, seed=10 * k + s, grid=folded)
    ss = R.exact_ss(C, 10 * k + s) if folded else None
    if folded:
        R.assert_exact_affine(x, ss)
        assert bool((ss[2] < 0).any()) and bool((ss[2] > 0).any())
    y, arg = R.pool_expected(x, k, s, pad, ss)
    act = x if ss is None else R.round_bf16(torch.clamp(x.double() * ss[2].double() + ss[3].double(), min=0.0))
    ye, ae = R.emu_maxpool(act, k, s, pad)
    assert R.cmp_exact(ye, y).ok and R.cmp_exact(ae, arg).ok
    yb, ab = R.emu_maxpool(act, k, s, pad, last_tie=True)
    if k > 1:
        assert not R.cmp_exact(ab, arg).ok  # the data holds ties in every geometry with a real window


def test_ambiguous_mask_share_is_small_for_real_statistics():
    """Where the stats are not exact (the rows' own batch statistics) the elements whose
    recomputed mask fp32 may decide either way must be rare: at most 1e-3 of them."""
    for C, M in [(64, 16 * 32 + 3), (24, 16 * 85 + 3), (2048, 19)]:
        inp = R.make_rows(C, M, R.case_seed(C, M))
        S, _, _ = R.ref_partial_fwd(inp["x"])
        st, _, _, _ = R.ref_finalize(S, float(M), inp["gamma"], inp["beta"], None, None, None, 0.1, 1e-5)
        assert float(R.ambiguous(inp["x"], st.float()).double().mean()) <= 1e-3


def test_gap_backward_reference():
    x = torch.randn(3, 16, 4, 4, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(3, 16, dtype=torch.float64)
    x.mean((2, 3)).backward(dy)
    assert torch.allclose(R.ref_gap_bwd(dy, 16), x.grad.permute(0, 2, 3, 1).reshape(3, 16, 16), atol=1e-15, rtol=0)


@pytest.mark.parametrize("geo,C,shape", R.POOLED_BN_CASES)
def test_pooled_backward_comparison_accepts_emulation(geo, C, shape):
    op = R.pooled_operands(geo, C, shape)
    R.assert_exact_affine(op["x"], op["ss"])
    M = op["x"].numel() // C
    rpb, _ = R.bn_plan(M, C)
    S, A, n, coef, dx, mag, d = R.pooled_reference(op, rpb)
    x32, d32 = op["x"].reshape(-1, C).float(), d.float()
    good = R.cmp_part(R.emu_partial(d32, d32 * x32, rpb), S, A, n)
    assert good.ok, good.detail
    assert not R.cmp_part(R.emu_partial(d32, d32 * x32, rpb, drop_last=True), S, A, n).ok or not bool(d[-1].any())
    good = R.cmp_bf16(R.emu_bwd_apply(x32, d32, coef), dx, mag)
    assert good.ok, good.detail
    assert not R.cmp_bf16(R.emu_bwd_apply(x32, d32, coef, truncate=True), dx, mag).ok


def test_some_pool_geometry_leaves_trailing_rows_and_columns_uncovered():
    """(H or W) - (last window's end): the GPU tests assert that gradient to be exactly 0."""
    left = []
    for g in R.POOL_GEOMETRIES:
        k, s, pad = g
        _, H, W = R.pool_shape(k, s, pad, 8)
        OH, OW = R.pool_out(H, W, k, s, pad)
        left.append((g, H - ((OH - 1) * s - pad + k), W - ((OW - 1) * s - pad + k)))
    assert any(h > 0 for _, h, _ in left) and any(w > 0 for _, _, w in left), left
