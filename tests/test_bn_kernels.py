"""Every stage of csrc/bn_act.hip, called through its binding on NHWC rows and compared
with the float64 reference of the same stage (tests/bn_reference.py, validated on the
CPU by tests/test_bn_reference.py).  The tolerances are derived there, next to each bound.

Template instances and the tests that launch them (ids abbreviated; every C-M of the
case lists runs each):

  bn_partial_kernel<0,false>                      test_forward_partial[*]
  bn_partial_kernel<1,false>                      test_backward_partial[(None, False, False)-*]
  bn_partial_kernel<1,false,false,false,true>     test_backward_partial[(None, False, True)-*]
  bn_partial_kernel<1,false,true>                 test_backward_partial[(None, True, False)-*]
  bn_partial_kernel<1,false,true,false,true>      test_backward_partial[(None, True, True)-*]
  bn_partial_kernel<1,true>                       test_backward_partial[('y', False, False)-*]
  bn_partial_kernel<1,true,false,false,true>      test_backward_partial[('y', False, True)-*]
  bn_partial_kernel<1,true,true>                  test_backward_partial[('y', True, False)-*]
  bn_partial_kernel<1,true,true,false,true>       test_backward_partial[('y', True, True)-*]
  bn_partial_kernel<1,true,false,true>            test_backward_partial[('ss', False, False)-*],
                                                  test_recomputed_mask_with_inexact_statistics
  bn_partial_kernel<1,true,true,true>             test_backward_partial[('ss', True, False)-*]
  bn_partial_kernel<1,true,false,true,false,true> test_pool_kernels.py::test_pooled_bn_backward[*]
  bn_finalize_kernel<false,float>                 test_finalize[*]
  bn_finalize_kernel<true,float>                  test_backward_finalize[*]
  bn_finalize_kernel<*,double>                    second reduction level only (off by default)
  bn_apply_kernel<relu,res>                       test_apply[relu-res-*], all four
  bn_bwd_apply_kernel<false,false>                test_backward_apply[(None, False, False)-*]
  bn_bwd_apply_kernel<false,true>                 test_backward_apply[(None, False, True)-*]
  bn_bwd_apply_kernel<false,false,true>           test_backward_apply[(None, True, False)-*]
  bn_bwd_apply_kernel<false,true,true>            test_backward_apply[(None, True, True)-*]
  bn_bwd_apply_kernel<true,false>                 test_backward_apply[('y', False, False)-*]
  bn_bwd_apply_kernel<true,true>                  test_backward_apply[('y', False, True)-*]
  bn_bwd_apply_kernel<true,false,true>            test_backward_apply[('y', True, False)-*]
  bn_bwd_apply_kernel<true,true,true>             test_backward_apply[('y', True, True)-*]
  bn_bwd_apply_kernel<true,false,false,true>      test_backward_apply[('ss', False, False)-*],
                                                  test_recomputed_mask_with_inexact_statistics
  bn_bwd_apply_kernel<true,false,true,true>       test_backward_apply[('ss', True, False)-*]
  bn_bwd_apply_kernel<true,false,false,true,true> test_pool_kernels.py::test_pooled_bn_backward[*]

Each test prints its worst error / bound; test_zz_worst_ratios prints the worst per stage."""
import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu
WORST = {}


def _mod():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


def _dev(t):
    return t.to("cuda") if torch.is_tensor(t) else t


def _gpu(inp):
    return {k: _dev(v) for k, v in inp.items()}


def _report(stage, case, c):
    torch.cuda.synchronize()
    print(f"{stage} {case}: {c.detail}")
    WORST[stage] = max(WORST.get(stage, 0.0), c.ratio)
    assert c.ok, f"{stage} {case}: {c.detail}"


def _check_part_blocks(part, M, C):
    rpb, blocks = R.bn_plan(M, C)
    assert part.shape == (blocks, 2, C) and part.dtype == torch.float32
    return rpb


def test_reference_rounds_on_the_device_as_on_the_cpu():
    """The references run where the operands live; their bf16 rounding must not depend on
    it, ties (sums of two bf16 values are full of them) included."""
    inp = R.make_rows(64, 515, 1)
    s = inp["dy"].double() + inp["dy2"].double()
    edge = torch.tensor([1e-40, 3.4e38, -0.0], dtype=torch.float64)
    v = torch.cat([s.flatten(), inp["x"].double().flatten() * 1.37, edge])
    assert int((s * 512 % 2 == 1).sum()) > 1000  # odd multiples of 2^-9: ties for 0.5 <= |s| < 1
    for trunc in (False, True):
        assert torch.equal(R.round_bf16(v.cuda(), trunc).cpu(), R.round_bf16(v, trunc))


@pytest.mark.parametrize("C,M", R.FWD_PARTIAL_CASES)
@pytest.mark.parametrize("with_nbt", [False, True])
def test_forward_partial(C, M, with_nbt):
    x = R.make_rows(C, M, R.case_seed(C, M))["x"].cuda()
    nbt = torch.tensor([5], dtype=torch.int64, device="cuda") if with_nbt else None
    part = _mod().bn_partial(x, None, None, C, 0, False, nbt)
    rpb = _check_part_blocks(part, M, C)
    _report("bn_partial fwd", (C, M), R.cmp_part(part, *R.ref_partial_fwd(x, rpb)))
    if with_nbt:
        assert int(nbt) == 6  # += 1 exactly, whatever the block count


@pytest.mark.parametrize("C,M", R.BWD_PARTIAL_CASES)
@pytest.mark.parametrize("variant", R.BWD_PARTIAL_VARIANTS, ids=str)
def test_backward_partial(variant, C, M):
    mask, dy2, wd = variant
    inp = _gpu(R.bwd_operands(C, M, mask))
    if mask == "ss":
        R.assert_exact_affine(inp["x"], inp["ss"])
    dout = torch.full_like(inp["x"], 7.0) if wd else None
    part = _mod().bn_partial(inp["x"], inp["y"] if mask == "y" else None, inp["dy"], C, 1, mask is not None, None,
                             inp["dy2"] if dy2 else None, inp["ss"] if mask == "ss" else None, dout)
    rpb = _check_part_blocks(part, M, C)
    _report("bn_partial bwd", (variant, C, M), R.check_partial_bwd(part, dout, inp, variant, rpb))


@pytest.mark.parametrize("C,M", R.APPLY_CASES)
@pytest.mark.parametrize("relu,with_res", [(False, False), (False, True), (True, False), (True, True)])
def test_apply(relu, with_res, C, M):
    inp = _gpu(R.make_rows(C, M, R.case_seed(C, M)))
    scale, shift = R.apply_coefficients(inp)
    res = inp["res"] if with_res else None
    nbt = torch.tensor([2], dtype=torch.int64, device="cuda") if (C + M) % 2 else None  # half the cases
    y = torch.full_like(inp["x"], 7.0)
    _mod().bn_apply(inp["x"], scale, shift, res, relu, y, nbt)
    ref, mag = R.ref_apply(inp["x"], scale, shift, res, relu)
    _report("bn_apply", (relu, with_res, C, M), R.cmp_bf16(y, ref, mag))
    if nbt is not None:
        assert int(nbt) == 3


@pytest.mark.parametrize("C,M", R.APPLY_CASES)
@pytest.mark.parametrize("variant", R.BWD_APPLY_VARIANTS, ids=str)
def test_backward_apply(variant, C, M):
    mask, dy2, dr = variant
    inp = _gpu(R.bwd_operands(C, M, mask))
    if mask == "ss":
        R.assert_exact_affine(inp["x"], inp["ss"])
    coef = R.bwd_coefficients(inp, M, variant).contiguous()
    dx = torch.full_like(inp["x"], 7.0)
    dres = torch.full_like(inp["x"], 7.0) if dr else None
    _mod().bn_bwd_apply(inp["x"], inp["y"] if mask == "y" else None, inp["dy"], coef, mask is not None, dx, dres,
                        inp["dy2"] if dy2 else None, inp["ss"] if mask == "ss" else None)
    _report("bn_bwd_apply", (variant, C, M), R.check_bwd_apply(dx, dres, inp, coef, variant))


def test_recomputed_mask_with_inexact_statistics():
    """The rows' own batch statistics: x * scale + shift rounds in fp32, so the elements
    within 4 u (|x scale| + |shift|) of zero may be masked either way.  They are left out
    of the elementwise comparison, their |d| and |d x| are added to the sums' bound, and
    they must be at most 1e-3 of all (a condition on the inputs, met by the reference
    alone: tests/test_bn_reference.py)."""
    C, M = 64, 16 * 32 + 3
    inp = _gpu(R.make_rows(C, M, R.case_seed(C, M)))
    S, _, _ = R.ref_partial_fwd(inp["x"])
    st, _, _, _ = R.ref_finalize(S, float(M), inp["gamma"], inp["beta"], None, None, None, 0.1, 1e-5)
    st = st.float().contiguous()
    amb = R.ambiguous(inp["x"], st)
    assert float(amb.double().mean()) <= 1e-3
    part = _mod().bn_partial(inp["x"], None, inp["dy"], C, 1, True, None, None, st)
    rpb = _check_part_blocks(part, M, C)
    d, Sb, A, n = R.ref_partial_bwd(inp["x"], inp["dy"], ss=st, relu=True, rpb=rpb)
    d0 = torch.where(amb, inp["dy"].double(), torch.zeros_like(d))
    extra = torch.stack([R.block_sums(d0.abs(), rpb), R.block_sums((d0 * inp["x"].double()).abs(), rpb)], 1)
    _report("bn_partial bwd", ("inexact ss", C, M), R.cmp_part(part, Sb, A, n, extra))
    coef, _ = R.ref_bwd_finalize(Sb, float(M), inp["gamma"], st[0], st[1])
    coef = coef.float().contiguous()
    dx = torch.full_like(inp["x"], 7.0)
    _mod().bn_bwd_apply(inp["x"], None, inp["dy"], coef, True, dx, None, None, st)
    ref, mag = R.ref_bwd_apply(inp["x"], d, coef)
    _report("bn_bwd_apply", ("inexact ss", C, M), R.cmp_bf16(dx, ref, mag, skip=amb))


@pytest.mark.parametrize("momentum,pending", R.FIN_MOMENTA)
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("nparts,C", R.FIN_CASES)
def test_finalize(nparts, C, affine, momentum, pending):
    for count in R.FIN_COUNTS:
        part, gamma, beta, rm, rv, nbt = (_dev(t) for t in R.finalize_operands(nparts, C, count, affine))
        new_rm, new_rv = rm.clone(), rv.clone()
        nbt_t = torch.tensor([nbt], dtype=torch.int64, device="cuda")
        stats = _mod().bn_finalize(part, count, gamma, beta, new_rm, new_rv, nbt_t, momentum, 1e-5, bool(pending))
        assert int(nbt_t) == nbt  # read, never written here
        c = R.check_finalize(stats, new_rm, new_rv, part, count, gamma, beta, rm, rv, nbt, momentum, 1e-5, pending)
        _report("bn_finalize", (nparts, C, affine, momentum, pending, count), c)
        # channel 0: b / count - mean^2 < 0 is clamped to 0, invstd = 1 / sqrt(eps)
        eps32 = float(torch.tensor(1e-5, dtype=torch.float32))
        assert abs(float(stats[1, 0]) - eps32 ** -0.5) <= 2 * R.U * eps32 ** -0.5
    # without running statistics
    stats = _mod().bn_finalize(part, count, gamma, beta, None, None, None, 0.1, 1e-5, False)
    c = R.check_finalize(stats, None, None, part, count, gamma, beta, None, None, None, 0.1, 1e-5, 0)
    _report("bn_finalize", (nparts, C, affine, "no running stats"), c)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("nparts,C", R.FIN_CASES)
def test_backward_finalize(nparts, C, affine):
    part, mean, invstd = (_dev(t) for t in R.make_bwd_parts(nparts, C, 17 * nparts + C))
    gamma = _dev(R.finalize_operands(nparts, C, 50.0, affine)[1])
    for count in (1.0, 50.0, 100352.0):
        coef = _mod().bn_bwd_finalize(part, count, gamma, mean, invstd)
        _report("bn_bwd_finalize", (nparts, C, affine, count),
                R.check_bwd_finalize(coef, part, count, gamma, mean, invstd))


def test_backward_apply_rejects_recomputed_mask_with_dres():
    """relu + ss + dres has no kernel (the y-masked one would be launched without y): the
    binding refuses it on the host, before any launch."""
    C, M = 8, 4
    x = torch.zeros(M, C, dtype=torch.bfloat16, device="cuda")
    coef = torch.zeros(5, C, device="cuda")
    ss = torch.zeros(4, C, device="cuda")
    with pytest.raises(RuntimeError, match="dres"):
        _mod().bn_bwd_apply(x, None, x.clone(), coef, True, x.clone(), x.clone(), None, ss)
    with pytest.raises(RuntimeError, match="dres"):  # a y given as well does not rescue it
        _mod().bn_bwd_apply(x, x.clone(), x.clone(), coef, True, x.clone(), x.clone(), None, ss)


def test_zz_worst_ratios():
    for stage, r in sorted(WORST.items()):
        print(f"WORST {stage}: error / bound {r:.3g}")
    assert all(r <= 1.0 for r in WORST.values())
