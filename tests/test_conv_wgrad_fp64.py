"""The weight-gradient kernels (csrc/conv_wgrad.hip: the generic tap-GEMM ``wgrad_kernel``,
the 3x3 halo kernel ``wgrad3x3_kernel`` and ``wgrad_reduce_kernel``) element by element
against float64, on the raw bindings ``conv_wgrad`` / ``conv_wgrad_plan`` (NHWC memory).

tests/wgrad_reference.py holds the reference, the operands and the two comparisons
(tests/test_wgrad_reference.py checks those on the CPU):
  * integer operands in {+-1 .. +-4}: every partial sum is an integer below 2^24, fp32
    accumulation is exact in any order, and the result must be ``torch.equal`` to the
    float64 reference -- no tolerance.  Used wherever the question is which rows and taps
    went where: tile decode, split counts, the reduce kernel's loop boundaries, long
    reductions, stage counts;
  * ``randn`` bf16 operands at M = N OH OW <= 512: no element past ``2 M 2^-24 A`` (A the
    same sum over |dy| |x|), where one missing term is more than 30 bounds.
Every case first asserts its plan from ``conv_wgrad_plan`` (kernel kind, tile instance,
split count, rows or stages per split), so a case that stops reaching its path fails.

Groups: every tile instance and a non-power-of-two tile grid (XCD order with padding
blocks); generic geometry (stride 2 at even and odd H, asymmetric filters / strides / pads,
7x7 / 2 / 3, taps wholly in padding == 0.0, 3x3 too wide for the halo kernel); the halo
kernel at both sides of its width classes (OW 16 | 17, 32 | 33, 64), images shorter than a
stage, odd and single stage totals, each also through the generic kernel; ``plan.splits`` at
every boundary of the reduce kernel (16 thread groups, a 4-way unrolled loop from 49 splits
on) up to 258 splits with a last split of one partial stage; one long reduction per family
in a single workgroup; 1, 2, 3 stages per split on a 4-wave and a 2-wave reduction split;
two-run determinism; the plan's cover of [0, M) for ResNet-50's layers at real batch sizes;
a deferred BatchNorm + ReLU (``pre_ss``) on the strided generic and the halo kernel, with a
shift whose relu is positive so that a padding tap staged as relu(shift) fails.

Each random case prints its worst error / bound ratio.  Measured on an MI355X with the
factor 2 as stated (a worst-case bound: random errors largely cancel): generic geometry
0.001 - 0.021 (worst at the 5x5 on 2x3 images), halo kernel up to 0.151 (3x2x1 images, 6
rows) and the same cases through the generic kernel up to 0.104, pre_ss up to 0.002; no
element past the bound.  One dropped row at these sizes is 30 bounds or more.  Both files
of the weight gradient (this one and test_conv_wgrad.py) take about 9 s together.
"""
import functools

import pytest
import torch

import wgrad_reference as R

pytestmark = pytest.mark.gpu

# every ResNet-50 convolution but the stem: (input H = W, Cin, Cout, k, stride, pad)
RESNET50 = [
    (56, 64, 64, 1, 1, 0), (56, 64, 64, 3, 1, 1), (56, 64, 256, 1, 1, 0), (56, 256, 64, 1, 1, 0),
    (56, 256, 128, 1, 1, 0), (56, 128, 128, 3, 2, 1), (28, 128, 512, 1, 1, 0), (56, 256, 512, 1, 2, 0),
    (28, 512, 128, 1, 1, 0), (28, 128, 128, 3, 1, 1),
    (28, 512, 256, 1, 1, 0), (28, 256, 256, 3, 2, 1), (14, 256, 1024, 1, 1, 0), (28, 512, 1024, 1, 2, 0),
    (14, 1024, 256, 1, 1, 0), (14, 256, 256, 3, 1, 1),
    (14, 1024, 512, 1, 1, 0), (14, 512, 512, 3, 2, 1), (7, 512, 2048, 1, 1, 0), (14, 1024, 2048, 1, 2, 0),
    (7, 2048, 512, 1, 1, 0), (7, 512, 512, 3, 1, 1),
]
BATCHES = (1, 2, 3, 24, 32, 64, 256)


def _ops():
    from ray_lightning_accelerators_amd import ops

    return ops.require()


def _dev():
    return torch.device("cuda", 0)


def _args(geo, cin, cout):
    return (geo.n, geo.h, geo.w, cin, geo.oh, geo.ow, cout, geo.kh, geo.kw, geo.sh, geo.sw, geo.ph, geo.pw)


def _plan(geo, cin, cout, splits=0, algo=0):
    """(kind, wa, wb, splits, rows or stages per split)."""
    return tuple(_ops().conv_wgrad_plan(*_args(geo, cin, cout), splits, algo))


def _run(d, geo, cin, cout, splits=0, algo=0, pre=None, x=None):
    out = _ops().conv_wgrad(d["dy"], d["x"] if x is None else x, *_args(geo, cin, cout), splits, algo, pre)
    assert out.shape == (cout, geo.kh, geo.kw, cin) and out.dtype == torch.float32 and out.is_contiguous()
    return out


@functools.lru_cache(maxsize=None)
def _data(geo, cin, cout, kind):
    """Operands (NHWC, on the device) and their float64 references, computed once and never written again."""
    dy, x = (R.int_operands if kind == "int" else R.randn_operands)(geo, cin, cout)
    dy, x = dy.to(_dev()), x.to(_dev())
    d = {"dy": dy, "x": x, "ref": R.geo_ref(dy, x, geo)}
    if kind != "int":
        assert geo.rows <= R.MAX_RANDOM_ROWS, geo
        d["amp"] = R.geo_amp(dy, x, geo)
    return d


def _tile(cin, cout):
    """The generic kernel's workgroup tile (wa, wb) in 64-channel wave tiles and its rows per stage."""
    if cout % 128 == 0 and cin % 128 == 0:
        t = (2, 2)
    elif cout % 256 == 0:
        t = (4, 1)
    elif cin % 256 == 0:
        t = (1, 4)
    elif cout % 128 == 0:
        t = (2, 1)
    elif cin % 128 == 0:
        t = (1, 2)
    else:
        t = (1, 1)
    return t, (64 if t == (1, 1) else 32)


def _generic_split(m, s, kb):
    """(splits, rows per split) of ``s`` requested splits: whole stages of kb rows, no empty split."""
    rps = -(-(-(-m // s)) // kb) * kb
    return -(-m // rps), rps


def _halo_split(t, s):
    """(splits, stages per split) of ``s`` requested splits: stages in pairs, no empty split."""
    sps = -(-t // s)
    sps += sps & 1
    return -(-t // sps), sps


def _expect_generic(geo, cin, cout, splits, algo=0):
    """Asserts the plan of an explicit split request on the generic kernel; returns it."""
    (wa, wb), kb = _tile(cin, cout)
    plan = _plan(geo, cin, cout, splits, algo)
    assert plan == (0, wa, wb) + _generic_split(geo.rows, splits, kb), plan
    return plan


def _expect_halo(geo, cin, cout, splits):
    _, t = R.halo_stages(geo)
    plan = _plan(geo, cin, cout, splits)
    assert plan == (1, 1, 1) + _halo_split(t, splits), plan
    return plan


def _check_cover(plan, geo, cin, cout):
    """What any plan must satisfy for the kernels to sum every row exactly once and for the
    reduce kernel to read only partial slices that were written."""
    kind, wa, wb, s, per = plan
    assert s >= 1 and per >= 1
    if kind == 0:
        assert (wa, wb) == _tile(cin, cout)[0]
        kb, total = _tile(cin, cout)[1], geo.rows
        assert per % kb == 0, plan
        blocks = (cout // (64 * wa)) * (cin // (64 * wb)) * geo.kh * geo.kw * s
    else:
        assert kind == 1 and (wa, wb) == (1, 1) and per % 2 == 0, plan
        total = R.halo_stages(geo)[1]
        blocks = (cout // 64) * (cin // 64) * s
    assert (s - 1) * per < total <= s * per, (plan, total)   # the last split is not empty, none is missing
    # the grid index and the slices of the fp32 partials [splits][Cout][KH][KW][Cin] the binding allocates
    assert blocks + 7 < 2 ** 31 and s * cout * geo.kh * geo.kw * cin < 2 ** 40


def _exact(tag, got, d):
    c = R.cmp_exact(got, d["ref"])
    assert c.ok, f"{tag}: {c.detail}"


def _bound(tag, got, d, geo):
    c = R.cmp_bound(got, d["ref"], d["amp"], geo.rows)
    print(f"[bound ratio] {tag}: worst {c.ratio:.4f}")
    assert c.ok, f"{tag}: {c.detail}"


# ------------------------------------------------------------------ 2.1 tile instances, tile-grid decode
# (Cout, Cin) -> (wa, wb) and the tile grid (tiles along Cout, along Cin)
TILE_CASES = [
    ((64, 64), (1, 1), (1, 1)), ((128, 64), (2, 1), (1, 1)), ((64, 128), (1, 2), (1, 1)),
    ((128, 128), (2, 2), (1, 1)), ((256, 64), (4, 1), (1, 1)), ((64, 256), (1, 4), (1, 1)),
    ((192, 64), (1, 1), (3, 1)), ((64, 192), (1, 1), (1, 3)), ((192, 192), (1, 1), (3, 3)),
    ((320, 128), (1, 2), (5, 1)), ((256, 384), (2, 2), (2, 3)),
]
TILE_GEO = R.sq(2, 14, 13, 1, 1, 0)   # M = 364: not a multiple of the 32- or 64-row stage


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("case", TILE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_every_tile_instance_and_tile_grid(case, splits):
    """1x1 / stride 1 (the non-GEN instances), integer operands: every wave-tile layout, and
    tile grids of 3, 5, 6 and 9 tiles whose block total is no multiple of the 8 XCDs."""
    (cout, cin), tile, grid = case
    geo = TILE_GEO
    assert _tile(cin, cout)[0] == tile and (cout // (64 * tile[0]), cin // (64 * tile[1])) == grid
    plan = _expect_generic(geo, cin, cout, splits)
    assert plan[:4] == (0,) + tile + (splits,), plan
    _check_cover(plan, geo, cin, cout)
    d = _data(geo, cin, cout, "int")
    _exact(f"tiles {cout}x{cin} splits {splits}", _run(d, geo, cin, cout, splits), d)


def test_tile_cases_leave_padding_blocks_in_the_xcd_order():
    """Every block total above is no multiple of 8, so the last XCD's run ends in blocks that
    must return at once (the split-count cases below run totals of 16, 48 and 64: none)."""
    totals = {grid[0] * grid[1] * s for _, _, grid in TILE_CASES for s in (1, 3)}
    assert totals == {1, 3, 5, 6, 9, 15, 18, 27} and all(t % 8 for t in totals)
    assert {16, 48, 64} <= set(REDUCE_SPLITS)


# ------------------------------------------------------------------ 2.2 generic geometry
GEN_CH = (64, 128)   # (Cin, Cout): the (2, 1) tile, 32-row stages


@pytest.mark.parametrize("mode", ["random-s1", "random-s2", "int-s2"])
@pytest.mark.parametrize("geo", R.GENERIC_GEOMS, ids=lambda g: g.tag)
def test_generic_geometry(geo, mode):
    """The GEN instances of the tap-GEMM kernel: random operands under the element-wise bound
    at 1 and 2 splits, integer operands exactly; a tap wholly in padding is exactly 0.0."""
    cin, cout = GEN_CH
    kind, splits = mode.split("-s")
    splits = int(splits)
    plan = _expect_generic(geo, cin, cout, splits)
    assert plan[:4] == (0, 2, 1, splits), plan   # kind 0 also for the 3x3 / 1 / 1 at W = 65 and 70
    _check_cover(plan, geo, cin, cout)
    d = _data(geo, cin, cout, kind)
    got = _run(d, geo, cin, cout, splits)
    tag = f"generic {geo.tag} {mode}"
    if kind == "int":
        _exact(tag, got, d)
    else:
        _bound(tag, got, d, geo)
    pads = R.padding_taps(geo)
    assert bool(pads) == (geo is R.PADDING_GEOM)
    for r, s in pads:
        assert bool((got[:, r, s, :] == 0.0).all()), f"{tag}: padding tap ({r}, {s}) is not zero"


# ------------------------------------------------------------------ 2.3 halo kernel
HALO_CH = (64, 128)
HALO_SPLITS = (0, 1, 3)


@pytest.mark.parametrize("geo", R.HALO_GEOMS, ids=lambda g: g.tag)
def test_halo_kernel_width_classes(geo):
    """3x3 / 1 / 1 at both sides of every width class, OH % R != 0, OH < R, odd and single
    stage totals: the halo kernel (kind 1) and the generic kernel (algo 1), each against
    float64 -- integer operands exactly, random ones (M <= 512) under the bound -- at the
    automatic split, one split and three requested splits."""
    cin, cout = HALO_CH
    r, t = R.halo_stages(geo)
    kinds = ["int"] + (["random"] if geo.rows <= R.MAX_RANDOM_ROWS else [])
    for splits in HALO_SPLITS:
        if splits:
            ph = _expect_halo(geo, cin, cout, splits)
            pg = _expect_generic(geo, cin, cout, splits, algo=1)
            assert (ph[3] > 1) == (splits > 1 and t >= 3), (ph, t)
        else:
            ph, pg = _plan(geo, cin, cout, 0, 0), _plan(geo, cin, cout, 0, 1)
            assert ph[0] == 1 and pg[:3] == (0, 2, 1), (ph, pg)
        _check_cover(ph, geo, cin, cout)
        _check_cover(pg, geo, cin, cout)
        for kind in kinds:
            d = _data(geo, cin, cout, kind)
            for algo, name in ((0, "halo"), (1, "generic")):
                got = _run(d, geo, cin, cout, splits, algo)
                tag = f"{name} {geo.tag} (R {r}, T {t}) {kind} splits {splits}"
                if kind == "int":
                    _exact(tag, got, d)
                else:
                    _bound(tag, got, d, geo)
                for rr, ss in R.padding_taps(geo):   # H = 1 or W = 1: the outer taps see only padding
                    assert bool((got[:, rr, ss, :] == 0.0).all()), f"{tag}: padding tap ({rr}, {ss}) is not zero"


# ------------------------------------------------------------------ 2.4 split structure, reduce kernel
# wgrad_reduce_kernel: 16 thread groups take splits j, j + 16, ...; four loads at a time while
# k + 48 < S, then one at a time; the groups are combined through LDS
REDUCE_SPLITS = (2, 15, 16, 17, 47, 48, 49, 63, 64, 65, 130, 258)


def _generic_split_case(s):
    """64 -> 64 1x1 (64-row stages): s splits of one stage, the last one of 37 rows."""
    return R.pointwise((s - 1) * 64 + 37)


def _halo_split_case(s):
    """64 -> 64 3x3 on 3x7 images (OW < 16; R = 4 > OH: one stage per image): 2 s - 1 stages,
    s splits of a stage pair, the last one a single stage."""
    return R.halo(2 * s - 1, 3, 7)


@pytest.mark.parametrize("s", REDUCE_SPLITS)
def test_generic_kernel_split_counts(s):
    geo = _generic_split_case(s)
    plan = _expect_generic(geo, 64, 64, s)
    assert plan == (0, 1, 1, s, 64) and geo.rows - (s - 1) * 64 == 37, plan
    _check_cover(plan, geo, 64, 64)
    d = _data(geo, 64, 64, "int")
    _exact(f"generic {s} splits", _run(d, geo, 64, 64, s), d)


@pytest.mark.parametrize("s", REDUCE_SPLITS)
def test_halo_kernel_split_counts(s):
    geo = _halo_split_case(s)
    assert R.halo_stages(geo) == (4, 2 * s - 1)
    plan = _expect_halo(geo, 64, 64, s)
    assert plan == (1, 1, 1, s, 2), plan
    _check_cover(plan, geo, 64, 64)
    d = _data(geo, 64, 64, "int")
    _exact(f"halo {s} splits", _run(d, geo, 64, 64, s), d)


LONG_GENERIC = R.pointwise(9001)   # 141 stages of 64 rows in one workgroup
LONG_HALO = R.halo(11, 27, 29)     # 8613 rows: 154 stages of two 29-pixel rows, OH odd


def test_long_reduction_in_one_workgroup():
    """A production split's stage count (ResNet's 56x56 layers at batch 256 run about 100
    stages per split) through a single workgroup per tile, exact."""
    plan = _expect_generic(LONG_GENERIC, 64, 64, 1)
    assert plan == (0, 1, 1, 1, 9024), plan
    d = _data(LONG_GENERIC, 64, 64, "int")
    _exact("generic 9001 rows, 1 split", _run(d, LONG_GENERIC, 64, 64, 1), d)
    assert R.halo_stages(LONG_HALO) == (2, 154)
    plan = _expect_halo(LONG_HALO, 64, 64, 1)
    assert plan == (1, 1, 1, 1, 154), plan
    d = _data(LONG_HALO, 64, 64, "int")
    _exact("halo 8613 rows, 1 split", _run(d, LONG_HALO, 64, 64, 1), d)
    # the same rows through the generic kernel's GEN instance (nine taps, padding masks)
    plan = _expect_generic(LONG_HALO, 64, 64, 1, algo=1)
    assert plan == (0, 1, 1, 1, 8640), plan
    _exact("generic 3x3 8613 rows, 1 split", _run(d, LONG_HALO, 64, 64, 1, 1), d)


@pytest.mark.parametrize("stages", [1, 2, 3])
@pytest.mark.parametrize("cout", [64, 128], ids=["4-wave-split", "2-wave-split"])
def test_stage_counts_per_split(cout, stages):
    """1, 2 and 3 stages per split (the loop runs stages in pairs: an odd count runs one
    all-zero stage) where 4 waves (tile (1, 1)) or 2 waves (tile (2, 1)) share the reduction."""
    (wa, wb), kb = _tile(64, cout)
    assert (wa, wb, kb) == ((1, 1, 64) if cout == 64 else (2, 1, 32))
    for splits in (1, 2):
        geo = R.pointwise(splits * stages * kb - 5)   # the last stage is 5 rows short
        plan = _expect_generic(geo, 64, cout, splits)
        assert plan == (0, wa, wb, splits, stages * kb), plan
        d = _data(geo, 64, cout, "int")
        _exact(f"{stages} stages x {splits} splits, tile {wa}x{wb}", _run(d, geo, 64, cout, splits), d)


def test_many_splits_are_deterministic():
    """Random operands (their fp32 sums depend on the order): two runs of 130 generic splits
    and of 65 halo splits are bitwise equal."""
    for geo, s, algo, expect in ((R.pointwise(129 * 64 + 37), 130, 0, _expect_generic),
                                 (R.halo(129, 3, 7), 65, 0, _expect_halo)):
        assert expect(geo, 64, 64, s)[3] == s
        dy, x = (t.to(_dev()) for t in R.randn_operands(geo, 64, 64))
        d = {"dy": dy, "x": x}
        a = _run(d, geo, 64, 64, s, algo)
        b = _run(d, geo, 64, 64, s, algo)
        assert torch.equal(a, b), f"{int((a != b).sum())} elements differ between two runs"
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


# ------------------------------------------------------------------ 2.5 plan invariants
def test_resnet50_plans_cover_every_row_once():
    """No kernel launch: the automatic plan of every ResNet-50 layer but the stem at real
    batch sizes, on both algorithms."""
    seen = set()
    for n in BATCHES:
        for h, cin, cout, k, stride, pad in RESNET50:
            geo = R.sq(n, h, h, k, stride, pad)
            halo_layer = (k, stride, pad) == (3, 1, 1) and geo.ow <= 64
            for algo in (0, 1):
                plan = _plan(geo, cin, cout, 0, algo)
                assert plan[0] == (1 if halo_layer and algo == 0 else 0), (geo, cin, cout, algo, plan)
                _check_cover(plan, geo, cin, cout)
                seen.add((plan[0], plan[3] > 1))
    assert sum(1 for layer in RESNET50 if layer[3:] == (3, 1, 1)) == 4
    assert seen == {(0, False), (0, True), (1, False), (1, True)}   # both kernels, with and without the reduce


# ------------------------------------------------------------------ 2.6 deferred BatchNorm + ReLU
PRE_CASES = [(R.sq(4, 14, 14, 3, 2, 1), 0), (R.halo(3, 5, 17), 0), (R.halo(3, 5, 33), 0),
             (R.halo(3, 5, 17), 1), (R.halo(3, 5, 33), 1)]


def _stats(cin, kind):
    """bn_finalize's [4, C] layout (mean, invstd, scale, shift) with a shift whose relu is positive."""
    g = torch.Generator(device="cpu").manual_seed(77 + cin)
    st = torch.randn(4, cin, generator=g)
    st[1] = st[1].abs() + 0.5
    if kind == "int":
        st[2], st[3] = 1.0, 5.0        # relu(x + 5) in 1 .. 9 for x in +-1 .. +-4: exact, never zero
    else:
        st[3] = st[3].abs() + 0.5      # scales of both signs: the ReLU clips, a padding pixel would not be 0
    return st.to(_dev()).contiguous()


@pytest.mark.parametrize("kind", ["int", "random"])
@pytest.mark.parametrize("case", PRE_CASES, ids=lambda c: f"{c[0].tag}-algo{c[1]}")
def test_pre_ss_on_strided_and_halo_kernels(case, kind):
    """``pre_ss`` on a generic stride-2 3x3 plan and on the halo kernel at the new width
    edges: bitwise the run on the materialised activation, and element-wise the float64
    gradient of bf16(relu(x scale + shift)) with ZERO padding."""
    geo, algo = case
    cin, cout = 64, 128
    plan = _plan(geo, cin, cout, 2, algo)
    halo_kernel = geo.sh == 1 and algo == 0
    assert plan[0] == (1 if halo_kernel else 0) and plan[3] == 2, plan
    assert geo.rows <= R.MAX_RANDOM_ROWS and geo.ph > 0 and geo.pw > 0
    d = _data(geo, cin, cout, kind)
    st = _stats(cin, kind)
    assert float(torch.relu(st[3]).min()) > 0
    a = torch.empty_like(d["x"])
    _ops().bn_apply(d["x"], st[2].contiguous(), st[3].contiguous(), None, True, a)
    if kind == "int":
        assert torch.equal(a, torch.relu(d["x"].float() + 5.0).to(torch.bfloat16)) and float(a.float().min()) >= 1.0
    got = _run(d, geo, cin, cout, 2, algo, pre=st)
    mat = _run(d, geo, cin, cout, 2, algo, x=a)
    assert torch.equal(got, mat), f"differs from the materialised run at {int((got != mat).sum())} elements"
    ref = {"ref": R.geo_ref(d["dy"], a, geo)}
    tag = f"pre_ss {geo.tag} algo {algo} {kind}"
    if kind == "int":
        _exact(tag, got, ref)
    else:
        ref["amp"] = R.geo_amp(d["dy"], a, geo)
        _bound(tag, got, ref, geo)
