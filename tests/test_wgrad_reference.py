"""tests/wgrad_reference.py checked on the CPU, before anything runs on a GPU: the float64
weight-gradient reference agrees with ``torch.nn.grad.conv2d_weight`` in float64 over every
geometry tests/test_conv_wgrad_fp64.py runs (the asymmetric ones and the taps that lie wholly
in padding included), the integer operands are what the exact comparison needs, and both
comparisons reject a gradient with one row dropped, one row doubled or a padding pixel read."""
import pytest
import torch

import wgrad_reference as R

GEOMS = R.GENERIC_GEOMS + R.HALO_GEOMS
CHANNELS = [(4, 8), (8, 4), (5, 7)]   # (Cin, Cout)


def _conv2d_weight(dy, x, geo):
    """torch's own weight gradient in float64, as [Cout, KH, KW, Cin]."""
    cin, cout = x.size(3), dy.size(3)
    g = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (cout, cin, geo.kh, geo.kw),
                                    dy.double().permute(0, 3, 1, 2), stride=(geo.sh, geo.sw), padding=(geo.ph, geo.pw))
    return g.permute(0, 2, 3, 1)


@pytest.mark.parametrize("geo", GEOMS, ids=lambda g: g.tag)
def test_wgrad_ref_is_conv2d_weight_in_float64(geo):
    cin, cout = CHANNELS[sum(geo) % len(CHANNELS)]
    pads = R.padding_taps(geo)
    for kind in ("positive", "signed", "int"):
        dy, x = (R.int_operands if kind == "int" else R.randn_operands)(geo, cin, cout, dtype=torch.float64)
        if kind == "positive":
            dy, x = dy.abs(), x.abs()
        ref = R.geo_ref(dy, x, geo)
        want = _conv2d_weight(dy, x, geo)
        assert ref.dtype == torch.float64 and ref.shape == (cout, geo.kh, geo.kw, cin)
        if kind == "signed":
            # two float64 summation orders of sign-mixed terms: an element that cancels to 1e-4 of
            # its terms differs by more than 1e-12 of ITSELF between any two correct evaluations,
            # so the relative tolerance is taken of the sum of the terms' magnitudes
            assert bool(((ref - want).abs() <= 1e-12 * R.geo_amp(dy, x, geo)).all())
        else:
            torch.testing.assert_close(ref, want, rtol=1e-12, atol=0.0)   # integers: both are exact
        for r, s in pads:
            assert bool((ref[:, r, s, :] == 0).all()) and bool((want[:, r, s, :] == 0).all()), (r, s)
        live = [(r, s) for r in range(geo.kh) for s in range(geo.kw) if (r, s) not in pads]
        assert live and all(bool((ref[:, r, s, :] != 0).any()) for r, s in live)
        amp = R.geo_amp(dy, x, geo)
        assert bool((amp >= ref.abs()).all())
        torch.testing.assert_close(amp, _conv2d_weight(dy.abs(), x.abs(), geo), rtol=1e-12, atol=0.0)
    # integer operands: the float64 sums are the exact integers
    assert bool((ref == ref.round()).all())


def test_padding_taps_come_from_the_geometry():
    assert R.padding_taps(R.PADDING_GEOM) == [(r, s) for r in (0, 4) for s in range(5)]
    assert R.padding_taps(R.halo(1, 1, 1)) == [(r, s) for r in range(3) for s in range(3) if (r, s) != (1, 1)]
    assert R.padding_taps(R.halo(3, 1, 17)) == [(r, s) for r in (0, 2) for s in range(3)]
    for geo in R.GENERIC_GEOMS:
        assert bool(R.padding_taps(geo)) == (geo is R.PADDING_GEOM), geo


def test_geometry_lists_hold_what_the_gpu_tests_claim():
    for geo in R.GENERIC_GEOMS:
        assert geo.rows <= R.MAX_RANDOM_ROWS, geo
    assert any(g.kh != g.kw for g in R.GENERIC_GEOMS) and any(g.sh != g.sw for g in R.GENERIC_GEOMS)
    assert any(g.ph != g.pw for g in R.GENERIC_GEOMS)
    assert any(g.kh == 7 and g.sh == 2 and g.ph == 3 for g in R.GENERIC_GEOMS)
    # the halo list: every width at both sides of a class edge, an image shorter than a stage in
    # the two classes that have more than one row per stage (OW > 32 has R = 1: no image is
    # shorter, no OH leaves a remainder), OH % R != 0, stage totals 1, odd, even
    for cls, r in ((16, 4), (32, 2)):
        mine = [g for g in R.HALO_GEOMS if R.halo_owp(g.ow) == cls]
        assert any(g.oh < r for g in mine) and any(g.oh > r and g.oh % r for g in mine)
    totals = {R.halo_stages(g)[1] for g in R.HALO_GEOMS}
    assert 1 in totals and any(t % 2 for t in totals if t > 1) and any(t % 2 == 0 for t in totals)
    rows = [g.rows for g in R.HALO_GEOMS]
    assert max(rows) > R.MAX_RANDOM_ROWS >= min(rows)
    assert {R.halo_owp(w) for w in R.HALO_WIDTHS} == {16, 32, 64}


def test_integer_operands_are_exact_in_bf16_and_never_zero():
    geo = R.sq(3, 9, 9, 3, 1, 0)
    dy, x = R.int_operands(geo, 64, 64)
    for t in (dy, x):
        assert t.dtype == torch.bfloat16
        assert sorted(set(t.float().flatten().tolist())) == [-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0]
    assert 16 * R.MAX_EXACT_ROWS <= 2 ** 24


def _fp32_gradient(dy, x, geo, drop=None, double=None, read_pad=False):
    """An fp32 evaluation of the gradient with one output row's contribution dropped or
    counted twice, or with the zero padding replaced by ones."""
    dy = dy.float().clone()
    if drop is not None:
        dy.view(-1, dy.size(3))[drop] = 0
    if read_pad:
        xp = torch.nn.functional.pad(x.float(), (0, 0, geo.pw, geo.pw, geo.ph, geo.ph), value=1.0)
        out = R.wgrad_ref(dy, xp, geo.kh, geo.kw, geo.sh, geo.sw, 0, 0).float()
    else:
        out = (R.geo_ref(dy, x, geo)).float()
    if double is not None:
        one = torch.zeros_like(dy)
        one.view(-1, dy.size(3))[double] = dy.view(-1, dy.size(3))[double]
        out = out + R.geo_ref(one, x, geo).float()
    return out


@pytest.mark.parametrize("geo", [R.GENERIC_GEOMS[0], R.GENERIC_GEOMS[5], R.halo(3, 5, 33), R.halo(1, 5, 17)],
                         ids=lambda g: g.tag)
def test_comparisons_reject_a_dropped_or_doubled_row_and_a_read_padding_pixel(geo):
    cin, cout = 8, 8
    last = geo.rows - 1
    dy, x = R.int_operands(geo, cin, cout)
    ref = R.geo_ref(dy, x, geo)
    assert R.cmp_exact(_fp32_gradient(dy, x, geo), ref).ok
    for kw in ({"drop": last}, {"drop": 0}, {"double": last // 2}, {"read_pad": True}):
        c = R.cmp_exact(_fp32_gradient(dy, x, geo, **kw), ref)
        assert not c.ok and "taps" in c.detail, (kw, c.detail)
    dy, x = R.randn_operands(geo, cin, cout)
    ref, amp = R.geo_ref(dy, x, geo), R.geo_amp(dy, x, geo)
    assert geo.rows <= R.MAX_RANDOM_ROWS
    c = R.cmp_bound(_fp32_gradient(dy, x, geo), ref, amp, geo.rows)
    assert c.ok and c.ratio < 1.0, c.detail
    for kw in ({"drop": last}, {"drop": 0}, {"double": last // 2}, {"read_pad": True}):
        c = R.cmp_bound(_fp32_gradient(dy, x, geo, **kw), ref, amp, geo.rows)
        assert not c.ok and c.ratio > 10.0, (kw, c.detail)


def test_exact_comparison_needs_an_exact_reference():
    geo = R.sq(1, 3, 3, 1, 1, 0)
    dy, x = R.randn_operands(geo, 4, 4, dtype=torch.float64)
    with pytest.raises(AssertionError):
        R.cmp_exact(R.geo_ref(dy, x, geo).float(), R.geo_ref(dy, x, geo))
