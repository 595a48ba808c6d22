"""The fused MNIST step (csrc/mlp_step3.hip) and ``mlp_eval`` (csrc/mlp_kernels.hip) held to
float64 element by element, stage by stage (tests/mlp_reference.py; checked on the CPU by
tests/test_mlp_reference.py).

Before every step the test snapshots what the launch will read (``params``, ``shadow``,
``h1pre``, ``xring``, ``yring``, ``counters``); after it, it reads what the head exported
(``act``: H1^T, H2^T, dH2^T, dZ^T; ``dh1t``), the stats row and the gradient.  Each stage is
compared with a float64 reference computed from the kernel's OWN output of the stage before:

  gather   xring / yring slot == bf16(u8_to_input(x[idx])); rows past the batch zero, label -1
  layer1   h1pre slot (copies summed) vs X . bf16(W1)^T: 49 2^-21 + sum_tiles 32 U24 amp_tile, or
           -- dyadic operands -- the int64 sum exactly; padded rows and the other slot zero.
           Checked at the start of EVERY step, so it is also the check of whoever wrote the
           slot during the step before from its freshly updated W1 tile.  An engine fed by
           ``set_data`` keeps both epochs' orders on the device, so there the slot found at an
           epoch's first step was written by the previous epoch's last tail (the STEP / ADAM /
           ACC / SGD tail or the one-launch tile waves: its switch of ``order`` buffer and ring
           slot at the wrap); an engine fed by ``begin_epoch`` (the short-batch cases) re-primes,
           so there an epoch's first slot is PRIME's and the tails are checked inside the epoch
  H1       == bf16(relu(float32(q) 2^-20 + b1)), every Bp column
  H2       U8 |ref| + 2 (L1 + 1) U24 amp   (dyadic operands: equal)
  dZ       U8 (|ref| + t) + t, t = (max ez / 2 + 2^-16) / rows; padded columns, classes 10..15 zero
  stats    loss within mean(2 max ez + 2^-16 (|m| + |lse| + |z_y|)); count, rows, step exact
  dH2 dH1  U8 |ref| + 2 K U24 amp (K = 16, L2), masks from the kernel's own H2 / H1; padding zero
  dW db    2 Bp U24 amp from the tail's own operands (act / dh1t / xring); amp = 0: exactly 0

The gradient is read three ways: the split route's ``grads`` (world 2, in the allreduce
callback); the fused tail's ``exp_avg`` of an engine with beta1 = 0 whose ``exp_avg`` the test
zeroes before each step, so that adam1's m = fmaf(1, g - 0, 0) is the gradient bit for bit
(with a nonzero m the difference g - m rounds first and m is the gradient only to an ulp of
|g - m|); and the one-launch step through its documented bitwise equality with that
two-launch twin.  A planted-integer tail (every act / dh1t / xring element in +-1..4) must
give the int64 products exactly, also when it accumulates.

Worst error / bound seen on an MI355X per stage, over every case of this file (each test
prints its own ``[bound ratio]`` lines and the last one the maxima): layer1 0.247, H2 0.994,
dZ 0.978, loss 0.008, dH2 0.996, dH1 0.988 (the three near 1 are the bf16 store: a result
just above a power of two rounds by up to 2^-8 of itself), dW1 0.036, dW2 0.029, dW3 0.077,
db1 0.013, db2 0.018, db3 0.028, Adam inside the fused tails 0.388, mlp_eval log-probs 0.010
and chunk sums 0.045; gather, labels, the zeroed slot, H1, every count, the planted-integer
gradients, every dyadic layer 1 / H2 and the one-launch and fused twins were equal.  No
element was past its bound.  The whole file (159 cases) takes about 8 s.
"""
import pytest
import torch

import mlp_reference as R
import optim_reference as OR
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices

pytestmark = pytest.mark.gpu

WIDTHS = sorted(fused_mlp.SUPPORTED)
NB = 3                       # batches per epoch (every case): 7 steps cross two epoch ends
STEPS = 2 * NB + 1
WORST = {}                   # per-stage maxima over the whole file (printed by the last test)


def _dev():
    return torch.device("cuda", 0)


def _seed(L1, L2, B, family):
    return 6000 + 7 * L1 + 3 * L2 + B + {"random": 0, "nozero": 50000, "prod": 90000}[family]


def make_case(L1, L2, B, family, world=1):
    """(x_u8, labels, params, normalize, lr) of one committed case: NB batches per rank and a few
    rows more (fewer than B, so that ``set_data`` makes exactly NB batches per epoch)."""
    seed = _seed(L1, L2, B, family)
    n = world * NB * B + min(5, B - 1)
    if family == "random":
        x, y = R.random_data(n, seed)
        return x, y, R.random_params(L1, L2, seed), None, 1e-2
    x, y = R.exact_data(n, seed, family)
    return x, y, R.exact_params(L1, L2, seed), (R.NORM_PM1 if family == "nozero" else None), 0.0


A_RANDOM_B = [(L1, L2, B) for L1, L2 in ((32, 64), (128, 256)) for B in (1, 17, 33, 48, 100, 256)] + [(64, 128, 1), (64, 128, 17)]
A_EXACT = [(L1, L2, B) for L1, L2 in ((32, 64), (64, 128), (128, 256)) for B in (17, 32, 100)]
SHORT = [(32, 64, 32, 24), (32, 64, 32, 1), (64, 128, 64, 33), (64, 128, 64, 7), (128, 256, 100, 99)]
SPLIT = [(32, 64, 32), (64, 128, 17), (128, 256, 100), (128, 64, 256), (32, 32, 1)]
E_SHAPES = [(32, 64, 1, 1), (64, 128, 17, 5), (128, 256, 32, 31), (32, 32, 33, 2), (128, 128, 100, 99)]


def committed_cases():
    """(L1, L2, B, family, world) of every engine case below (each names its data and weights
    through ``make_case``), for the CPU checks of tests/test_mlp_reference.py: no ambiguous row,
    and every dyadic operand certified."""
    out = [(L1, L2, 32, "random", 1) for L1, L2 in WIDTHS]
    out += [(L1, L2, B, "random", 1) for L1, L2, B in A_RANDOM_B]
    out += [(L1, L2, B, "random", 2) for L1, L2, B in SPLIT]
    out += [(64, 128, 32, "random", w) for w in (1, 2)]
    out += [(L1, L2, B, "nozero", 1) for L1, L2, B in A_EXACT]
    out += [(32, 64, 32, "prod", 1), (128, 256, 64, "prod", 1)]
    out += [(L1, L2, B, fam, 1) for L1, L2, B, _ in SHORT for fam in ("random", "nozero")]
    out += [(L1, L2, B, "nozero", w) for L1, L2, B, _ in E_SHAPES for w in (1, 2)]
    return sorted(set(out))


# ------------------------------------------------------------------ the per-step driver
def _engine(L1, L2, B, family, one_launch=False, host_order=None, last_rows=None, lr=None, **kw):
    x, y, params, norm, lr0 = make_case(L1, L2, B, family, kw.get("world_size", 1))
    kw.setdefault("betas", (0.0, 0.999))
    eng = FusedMLPEngine(L1, L2, B, lr=lr0 if lr is None else lr, device=_dev(), init_params=params, stats_ring=64,
                         **kw)
    eng.one_launch = eng.one_launch and one_launch
    if host_order is None:
        eng.set_data(x, y, normalize=norm)
    else:
        eng.attach_dataset(x, y, normalize=norm)
        eng.begin_epoch(host_order(0), NB, last_rows=last_rows)
    eng._case = (x, y, host_order, last_rows)
    return eng


def _host_order(n, B, last_rows):
    rows = (NB - 1) * B + (B if last_rows is None else last_rows)
    return lambda epoch: torch.randperm(n, generator=torch.Generator().manual_seed(77 + epoch))[:rows]


def _batch_idx(eng):
    """The sample indices the coming step must consume, from the host's own bookkeeping."""
    x, _, host_order, _ = eng._case
    B, cur = eng.B, eng.step_in_epoch
    rows = eng.last_rows if cur == eng.n_batches - 1 else B
    if host_order is not None:
        return host_order(eng.epoch)[cur * B: cur * B + rows]
    return shard_indices(x.size(0), eng.world_size, eng.rank, eng.epoch, eng.seed, True)[cur * B: cur * B + rows]


def _checked_step(eng, tag, exact=False, through_h2=False, act=True, grads="exp_avg", captured=None):
    """One engine step under the stage checks.  ``act``: the route exports act / dh1t (every
    route but the one-launch step, whose hand-off buffers are still checked).  ``grads``:
    "exp_avg" (beta1 = 0, exp_avg zeroed first), "capture" (the allreduce callback's copy) or
    None.  Returns the list of failures."""
    L1, L2, B, Bp = eng.L1, eng.L2, eng.B, R.bp_of(eng.B)
    x_u8, labels, host_order, last_rows = eng._case
    if host_order is not None and eng.step_in_epoch == 0 and eng.global_step > 0:
        eng.begin_epoch(host_order(eng.epoch), NB, last_rows=last_rows)
    if not eng._primed:
        eng.prime()
    if grads == "exp_avg":
        eng.exp_avg.zero_()
    torch.cuda.synchronize()
    snap = {k: getattr(eng, k).cpu().clone() for k in ("params", "shadow", "h1pre", "xring", "yring", "counters")}
    idx = _batch_idx(eng)
    rows, cur, step_want = idx.numel(), eng.step_in_epoch, eng.optimizer_steps + 1
    eng.step()
    torch.cuda.synchronize()
    c = snap["counters"]
    slot = int(c[3])
    assert torch.equal(c[0:5], c[5:10]) and int(c[1]) == cur and slot in (0, 1), (tag, c)
    assert R.shadow_invariants(snap["params"], snap["shadow"], L1, L2), tag
    hs = R.h1pre_slots(snap["h1pre"], L1, Bp)
    obs = R.act_dense(eng.act, eng.dh1t, L1, L2, Bp)
    obs.update(x=R.xring_dense(snap["xring"], Bp)[slot], y=R.yring_dense(snap["yring"], Bp)[slot],
               q=R.h1pre_dense(hs[slot], L1, Bp), q_other=R.h1pre_dense(hs[slot ^ 1], L1, Bp),
               stats=eng.recent_stats(1)[0])
    obs["x_want"], obs["y_want"] = R.ref_gather(x_u8, labels, idx, Bp, eng.x_scale, eng.x_shift)
    wt = R.weights_of(snap["params"], snap["shadow"], L1, L2)
    res = R.head_checks(obs, wt, rows, step_want, exact=exact, exact_through_h2=through_h2, handoff_only=not act)
    if act and grads is not None:
        g = eng.exp_avg if grads == "exp_avg" else captured[-1][: snap["params"].numel()]
        res += R.grad_checks(g, obs, L1, L2)
    return R.report(f"{tag} step {eng.global_step} rows {rows}", res, WORST)


def _run(eng, tag, steps=STEPS, **kw):
    bad = []
    for _ in range(steps):
        bad += _checked_step(eng, tag, **kw)
    eng.check()
    h = eng.health()
    assert h["saturated"] == 0 and h["nonfinite"] == 0, (tag, h)
    assert not bad, (tag, bad[:6])


_TWIN_KEYS = ("params", "exp_avg", "exp_avg_sq", "shadow", "h1pre", "xring", "yring", "stats")


def _twins_equal(a, b, tag):
    torch.cuda.synchronize()
    assert torch.equal(a.counters[:10].cpu(), b.counters[:10].cpu()), (tag, a.counters, b.counters)
    for k in _TWIN_KEYS:
        ta, tb = getattr(a, k), getattr(b, k)
        ne = ta.view(torch.int16) != tb.view(torch.int16) if ta.dtype == torch.bfloat16 else ta != tb
        assert not bool(ne.any()), (tag, k, int(ne.sum()), ne.nonzero().flatten()[:6].tolist())


def _run_with_one_launch_twin(L1, L2, B, family, tag, **kw):
    """The two-launch engine under the stage checks, the one-launch engine beside it under the
    hand-off checks; after every step the two hold the same bits."""
    two = _engine(L1, L2, B, family)
    one = _engine(L1, L2, B, family, one_launch=True)
    assert one.one_launch and not two.one_launch
    bad = []
    for _ in range(STEPS):
        bad += _checked_step(two, tag, **kw)
        bad += _checked_step(one, tag + " one-launch", act=False, exact=kw.get("exact", False))
        _twins_equal(one, two, tag)
    one.check()
    assert int(one.counters[10]) == STEPS  # every step of the twin was one launch
    assert not bad, (tag, bad[:6])


# ------------------------------------------------------------------ A + C: head stages, fused and one-launch gradients
@pytest.mark.parametrize("L1,L2", WIDTHS)
def test_head_stages_and_gradients_every_width(L1, L2):
    """All ten width pairs at B = 32 (every KG3 / KG1 K-split instance), random operands: the
    two-launch route stage by stage, its fused tail's gradient, and the one-launch twin."""
    _run_with_one_launch_twin(L1, L2, 32, "random", f"A {L1}/{L2} B=32")


@pytest.mark.parametrize("L1,L2,B", A_RANDOM_B)
def test_head_stages_and_gradients_every_batch_shape(L1, L2, B):
    """A partial head block, 2, 4 and 8 head blocks, Bp != B."""
    if B <= 17:
        _run_with_one_launch_twin(L1, L2, B, "random", f"A {L1}/{L2} B={B}")
    else:
        _run(_engine(L1, L2, B, "random"), f"A {L1}/{L2} B={B}")


@pytest.mark.parametrize("L1,L2,B", A_EXACT)
def test_head_stages_exact_operands(L1, L2, B):
    """Pixels +-1, dyadic weights, lr = 0: layer 1, H1 and H2 are ``torch.equal``, the logits are
    certified exact, so dZ, the loss and the count carry the 2^-16 allowance alone."""
    tag = f"A exact {L1}/{L2} B={B}"
    if B <= 32:
        _run_with_one_launch_twin(L1, L2, B, "nozero", tag, exact=True)
    else:
        _run(_engine(L1, L2, B, "nozero"), tag, exact=True)


@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 64)])
def test_head_stages_production_map_exact_through_h2(L1, L2, B):
    """The default pixel map on bytes 128..255 with the dyadic weights: certified through H2."""
    _run(_engine(L1, L2, B, "prod"), f"A prod {L1}/{L2} B={B}", through_h2=True)


# ------------------------------------------------------------------ B: the short last batch
@pytest.mark.parametrize("family", ["random", "nozero"])
@pytest.mark.parametrize("L1,L2,B,r", SHORT)
def test_short_last_batch_stage_by_stage(L1, L2, B, r, family):
    """Two epochs of a drop_last=False loader: the step that gathers the short batch, the one
    that consumes it (1 / last_rows in dZ and the loss, ``last_rows`` in the stats row, zero
    pixels / label -1 / zero deltas past it) and every full step around them."""
    x = make_case(L1, L2, B, family)[0]
    eng = _engine(L1, L2, B, family, host_order=_host_order(x.size(0), B, r), last_rows=r)  # re-primes per epoch
    _run(eng, f"B {family} {L1}/{L2} B={B} r={r}", steps=2 * NB, exact=family == "nozero")
    assert int(eng.recent_stats(1)[0, 2]) == r


# ------------------------------------------------------------------ C: the split route's gradients
@pytest.mark.parametrize("L1,L2,B", SPLIT)
def test_split_route_gradients(L1, L2, B):
    """head -> TAIL_GRAD -> allreduce -> TAIL_ADAM at world size 2 (two identical ranks):
    ``grads`` as the allreduce sees it, and a fused twin that must end on the same bits --
    adam1 writes the same bits on every route (csrc/mlp_common.h)."""
    captured = []

    def allreduce(g):
        captured.append(g.detach().cpu().clone())
        g.mul_(2)

    # ``set_data`` at world size 2: the orders of both epochs live on the device, so the slot an
    # epoch starts from is the one TAIL_ADAM wrote at the wrap.  The fused twin is fed rank 0's
    # shard by ``begin_epoch`` (it re-primes: PRIME and the tails write the same h1pre bits)
    split = _engine(L1, L2, B, "random", world_size=2, allreduce=allreduce)
    n = split._case[0].size(0)

    def order(epoch):
        return shard_indices(n, 2, 0, epoch, split.seed, True)[: NB * B]

    fused = FusedMLPEngine(L1, L2, B, lr=1e-2, betas=(0.0, 0.999), device=_dev(), stats_ring=64,
                           init_params=make_case(L1, L2, B, "random", 2)[2])
    fused.one_launch = False
    fused.attach_dataset(*split._case[:2])
    fused.begin_epoch(order(0), NB)
    assert split.n_batches == NB
    bad = []
    for _ in range(STEPS):
        bad += _checked_step(split, f"C split {L1}/{L2} B={B}", grads="capture", captured=captured)
        if fused.step_in_epoch == 0 and fused.global_step > 0:
            fused.begin_epoch(order(fused.epoch), NB)
        fused.step()
    assert not bad, bad[:6]
    torch.cuda.synchronize()
    for k in ("params", "exp_avg", "exp_avg_sq", "shadow"):
        assert torch.equal(getattr(split, k), getattr(fused, k)), k


# ------------------------------------------------------------------ D: planted integers through the gradient tail
@pytest.mark.parametrize("L1,L2,B", [(a, b, 32) for a, b in WIDTHS] +
                         [(a, b, B) for a, b in ((32, 64), (128, 256)) for B in (1, 17, 100, 256)])
def test_tail_grad_planted_integers_exact(L1, L2, B):
    """A real HEAD launch (so the counters are consistent), then act / dh1t / both xring slots
    overwritten with integers in +-1..4 (no zeros in valid columns, zeros in the padding, as in
    production): TAIL_GRAD's gradients are the int64 products and row sums exactly (at most
    16 * 256 < 2^24), and so is the accumulating tail's sum with planted integer ``grads``."""
    eng = _engine(L1, L2, B, "random")
    eng.prime()
    kw = eng._kw3()
    slot = int(eng.counters[3])
    fused_mlp.mlp3_launch(fused_mlp.MLP3_HEAD, stats=eng.stats, **kw)
    torch.cuda.synchronize()
    Bp, seed = R.bp_of(B), L1 + L2 + B
    valid = (torch.arange(Bp) < B).double().view(-1, 1)
    d = {k: R.int_plant((Bp, n), seed + i) * valid
         for i, (k, n) in enumerate((("h1", L1), ("h2", L2), ("dh2", L2), ("dz", 16), ("dh1", L1)))}
    d["dz"][:, R.NC:] = 0
    xs = torch.stack([R.int_plant((Bp, 784), seed + 10) * valid, R.int_plant((Bp, 784), seed + 11) * valid])
    act, dh1t = R.act_pack(d, L1, L2)
    assert act.numel() == eng.act.numel() and dh1t.numel() == eng.dh1t.numel()
    eng.act.copy_(act)
    eng.dh1t.copy_(dh1t)
    eng.xring.copy_(R.xring_pack(xs))
    fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_GRAD, stats=eng.stats, **kw)
    torch.cuda.synchronize()
    obs = dict(d, x=xs[slot])
    tag = f"D {L1}/{L2} B={B}"
    bad = R.report(tag, R.grad_checks(eng.grads, obs, L1, L2, exact=True), WORST)
    g0 = R.int_plant((eng.grads.numel(),), seed + 20)
    eng.grads.copy_(g0)
    fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_GRAD, stats=eng.stats, acc_add=True, **kw)
    torch.cuda.synchronize()
    want = g0 + R.flat_grads(R.ref_grads(obs))[0]
    bad += R.report(tag + " accumulate", [("acc", R.cmp_equal(eng.grads.cpu(), want))], WORST)
    assert not bad, bad


# ------------------------------------------------------------------ E: the layer-1 look-ahead of every route
ROUTES = {
    "step": dict(),                                   # PRIME, then the fused STEP tail
    "one_launch": dict(one_launch=True),              # the STEP1 tile waves
    "split": dict(world_size=2, allreduce=lambda g: g.mul_(2)),   # TAIL_ADAM after TAIL_GRAD
    "accumulate": dict(accumulate=2),                 # TAIL_ACC inside the window, TAIL_ADAM at its end
    "sgd": dict(optimizer="sgd", betas=(0.9, 0.999)),  # the SGD tail
}


def _route_engine(route, L1, L2, B, r, family, feed, lr=None):
    """``feed``: "set_data" (full batches; both epochs' orders on the device, the tail's
    look-ahead is live across the epoch end) or "begin_epoch" (a host order per epoch with a
    last batch of ``r`` rows; every epoch starts from PRIME)."""
    kw = dict(ROUTES[route])
    if feed == "set_data":
        eng = _engine(L1, L2, B, family, lr=lr, **kw)
        assert eng.n_batches == NB and not eng._host_epochs
    else:
        x = make_case(L1, L2, B, family, kw.get("world_size", 1))[0]
        last = r if r != B else None
        eng = _engine(L1, L2, B, family, host_order=_host_order(x.size(0), B, last), last_rows=last, lr=lr, **kw)
    assert eng.one_launch == (route == "one_launch" and B <= 32)
    return eng


def _run_route(eng, route, tag, **kw):
    bad, primes = [], 0
    for _ in range(2 * NB + 1):
        # a one-launch engine runs the two steps that touch the short batch as head + tail
        one = eng.one_launch and not eng._short_pos(eng.step_in_epoch)
        primes += not eng._primed
        bad += _checked_step(eng, tag, act=not one,
                             grads="exp_avg" if route in ("step", "one_launch") and not one else None, **kw)
    eng.check()
    assert eng.epoch == 2 and eng.step_in_epoch == 1   # two epoch ends behind it
    # set_data: PRIME ran once, before the first step -- every later slot is a tail's
    assert eng._host_epochs or primes == 1, primes
    assert not bad, bad[:6]


# the one-launch step exists for B <= 32; every other route runs every shape
E_CASES = [(route, *shape) for route in ROUTES for shape in E_SHAPES if route != "one_launch" or shape[2] <= 32]


@pytest.mark.parametrize("feed", ["set_data", "begin_epoch"])
@pytest.mark.parametrize("route,L1,L2,B,r", E_CASES)
def test_look_ahead_exact_on_every_route(route, L1, L2, B, r, feed):
    """Dyadic operands, lr = 0: at the start of every step the slot found there is the int64
    layer-1 sum of THIS batch exactly, the other slot all zero, padded rows zero, xring / yring
    bitwise right.  ``set_data`` (full batches): the slot at each of the two epoch starts was
    written by the route's own tail across the wrap (other ``order`` buffer, ring slot flipped).
    ``begin_epoch`` (last batch of ``r`` rows): the tails gather and consume the short batch
    inside the epoch; each epoch's first slot is PRIME's."""
    eng = _route_engine(route, L1, L2, B, r, "nozero", feed)
    _run_route(eng, route, f"E {route} {feed} {L1}/{L2} B={B} r={r if feed == 'begin_epoch' else B}", exact=True)


@pytest.mark.parametrize("feed", ["set_data", "begin_epoch"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_look_ahead_uses_the_updated_weights(route, feed):
    """Random operands, lr = 1e-2: every weight moves by about lr each step (Adam) or by
    lr g (SGD, lr = 0.1), and the next slot must match bf16(params AFTER the step) under the
    layer-1 bound -- a look-ahead from the tile as it was before the update is far outside.
    ``set_data``: also for the slot a tail writes across an epoch end."""
    L1, L2, B, r = 64, 128, 32, 19
    eng = _route_engine(route, L1, L2, B, r, "random", feed, lr=0.1 if route == "sgd" else 1e-2)
    p_init = eng.params.clone()
    _run_route(eng, route, f"E updated {route} {feed}")
    moved = (eng.params - p_init)[: L1 * 784].abs()   # the premise: W1 did move
    assert float(moved.max()) > 1e-4 and (route == "sgd" or float(moved.median()) > 1e-3), float(moved.median())


# ------------------------------------------------------------------ F: Adam inside the fused tails
@pytest.mark.parametrize("one_launch", [False, True], ids=["STEP", "STEP1"])
@pytest.mark.parametrize("L1,L2,adamw", [(32, 32, False), (64, 128, False), (128, 256, False), (64, 128, True)])
def test_adam_inside_the_fused_tails(L1, L2, adamw, one_launch):
    """beta1 = 0, exp_avg zeroed before the step: exp_avg afterwards is the gradient the tail
    applied, and the new exp_avg_sq, params and the three bf16 shadows are within
    optim_reference's bounds of float64 Adam / AdamW on that gradient."""
    kw = dict(optimizer="adamw", weight_decay=0.01) if adamw else {}
    eng = _engine(L1, L2, 32, "random", one_launch=one_launch, **kw)
    assert eng.one_launch == one_launch
    cfg = OR.adam_cfg("fused", lr=1e-2, betas=(0.0, 0.999), wd=0.01 if adamw else 0.0, adamw=adamw)
    lay = fused_mlp.mlp_shadow_layout(L1, L2)
    for t in (1, 2, 3):
        eng.exp_avg.zero_()
        st = {"p": eng.params.cpu().clone(), "m": eng.exp_avg.cpu().clone(), "v": eng.exp_avg_sq.cpu().clone()}
        eng.step()
        torch.cuda.synchronize()
        st["g"] = eng.exp_avg.cpu().clone()
        ref = OR.ref_mlp_adam(st, cfg, L1, L2, t=t)
        sh = eng.shadow.cpu()
        out = {"p": eng.params.cpu(), "m": eng.exp_avg.cpu(), "v": eng.exp_avg_sq.cpu(), "np": sh[: lay["np"]],
               "w2t": sh[lay["w2t"]:lay["w3t"]], "w3t": sh[lay["w3t"]:lay["total"]]}
        c = OR.check_mlp_adam(out, ref, L1, L2)
        print(f"[bound ratio] F {L1}/{L2} {'adamw ' if adamw else ''}{'STEP1' if one_launch else 'STEP'} t={t}: "
              f"worst {c.ratio:.3f}")
        WORST["adam"] = max(WORST.get("adam", 0.0), c.ratio)
        assert c.ok, c.detail
        assert int(eng.counters[0]) == t


# ------------------------------------------------------------------ G: mlp_eval per row
EVAL_N = [1, 31, 32, 33, 77, 96]
EVAL_WIDTHS = [(32, 64), (128, 256)]
EVAL_PROD = [(32, 64, 33), (128, 256, 77)]


def eval_operands(L1, L2, n, mode, family="nozero"):
    """(params, X [n, 784] float64, labels [n], x_u8, idx, affine) of one mlp_eval case, on the CPU
    (tests/test_mlp_reference.py certifies them there).  ``mode`` "f32": X holds +-1 and +-2."""
    seed = _seed(L1, L2, n, family) + 7
    params = R.exact_params(L1, L2, seed)
    x, y = R.exact_data(n + 9, seed, family)
    idx = torch.randperm(n + 9, generator=torch.Generator().manual_seed(seed))[:n]
    aff = fused_mlp.input_affine(R.NORM_PM1 if family == "nozero" else None)
    if mode == "u8":
        X = R.ref_gather(x, y, idx, n, *aff)[0]
    else:
        g = torch.Generator().manual_seed(seed)
        X = (torch.randint(1, 3, (n, 784), generator=g) * (torch.randint(0, 2, (n, 784), generator=g) * 2 - 1)).double()
    return params, X, y[idx], x, y, idx, aff


def _eval_case(L1, L2, n, mode, family="nozero"):
    params, X, yb, x, y, idx, aff = eval_operands(L1, L2, n, mode, family)
    if mode == "u8":
        kw = dict(x_u8=x.to(_dev()), index=idx.to(_dev()), labels=y.to(_dev()), x_scale=aff[0], x_shift=aff[1])
    else:
        kw = dict(x_f32=X.float().to(_dev()), labels=yb.to(_dev()))
    return params, X, yb, kw


@pytest.mark.parametrize("mode", ["u8", "f32"])
@pytest.mark.parametrize("n", EVAL_N)
@pytest.mark.parametrize("L1,L2", EVAL_WIDTHS)
def test_mlp_eval_per_row(L1, L2, n, mode):
    """Dyadic operands (u8 mode: the NORM instances on +-1 pixels; x_f32 mode: +-1 and +-2),
    every GEMM certified exact: each log-prob within 2^-16 (|z| + |lse|) of float64 z - lse,
    rows past n untouched, every 32-row chunk's (sum NLL, #correct) against the kernel's own
    log-probs (32 U24 sum |lp|; the count exact), partials and accumulate mode."""
    params, X, y, kw = _eval_case(L1, L2, n, mode)
    p = fused_mlp.mlp_unpack(params.to(torch.bfloat16).double(), L1, L2)
    b = fused_mlp.mlp_unpack(params.double(), L1, L2)
    W1, W2, W3 = p["layer_1.weight"], p["layer_2.weight"], p["layer_3.weight"]
    b1, b2, b3 = b["layer_1.bias"], b["layer_2.bias"], b["layer_3.bias"]
    assert torch.equal(W1, b["layer_1.weight"])   # the dyadic weights are bf16 numbers
    c1 = R.exact_certificate(X, W1, b1)
    H1 = torch.relu(X @ W1.t() + b1).to(torch.bfloat16).double()
    c2 = R.exact_certificate(H1, W2, b2)
    H2 = torch.relu(H1 @ W2.t() + b2).to(torch.bfloat16).double()
    c3 = R.exact_certificate(H2, W3, b3)
    assert c1.ok and c2.ok and c3.ok, (c1, c2, c3)
    Z = H2 @ W3.t() + b3
    st = R.ref_stats(Z, torch.zeros_like(Z), y)
    assert st.ambiguous == 0
    m = Z.max(1, keepdim=True).values
    lse = m + torch.log(torch.exp(Z - m).sum(1, keepdim=True))
    dev, nch = _dev(), (n + 31) // 32
    logits = torch.full((nch * 32 + 32, 10), -7777.0, device=dev)
    out = torch.full((nch, 2), -5.0, device=dev)
    fused_mlp.mlp_eval(params.to(dev), L1=L1, L2=L2, B=n, out=out, logits=logits, **kw)
    acc = torch.tensor([3.0, 4.0], device=dev)
    fused_mlp.mlp_eval(params.to(dev), L1=L1, L2=L2, B=n, out=acc, **kw)
    torch.cuda.synchronize()
    lp = logits.cpu().double()
    tag = f"G {mode} {L1}/{L2} n={n}"
    res = [("logp", R.cmp_bound(lp[:n], Z - lse, R.SOFT * (Z.abs() + lse.abs()))),
           ("untouched", R.cmp_equal(lp[n:], torch.full_like(lp[n:], -7777.0)))]
    nll = torch.zeros(nch * 32, dtype=torch.float64)
    nll[:n] = -lp[:n].gather(1, y.view(-1, 1)).squeeze(1)
    hit = torch.zeros(nch * 32, dtype=torch.float64)
    pred = torch.where(Z == m, torch.arange(10).expand_as(Z), torch.full_like(Z, 10, dtype=torch.long)).min(1).values
    hit[:n] = (pred == y).double()
    o = out.cpu().double()
    per = nll.view(nch, 32)
    res.append(("chunk_nll", R.cmp_bound(o[:, 0], per.sum(1), 32 * R.U24 * per.abs().sum(1))))
    res.append(("chunk_count", R.cmp_equal(o[:, 1], hit.view(nch, 32).sum(1))))
    a = acc.cpu().double()
    # accumulate mode: out += the chunks' sums (atomics in any order, onto the 3.0 that was there)
    res.append(("acc_nll", R.cmp_bound(a[0:1] - 3.0, nll.sum().view(1),
                                       (nch * 32 * R.U24 * (nll.abs().sum() + 3.0)).view(1))))
    res.append(("acc_count", R.cmp_equal(a[1:2] - 4.0, hit.sum().view(1))))
    bad = R.report(tag, res, WORST)
    assert not bad, bad


@pytest.mark.parametrize("L1,L2,n", EVAL_PROD)
def test_mlp_eval_production_map(L1, L2, n):
    """The default pixel map (bytes 128..255) with the dyadic weights: layers 1 and 2 certified,
    layer 3 by its certificate's verdict -- ez = 0 where it passes, the accumulation bound where
    it does not (decided from the operands, never from the output)."""
    params, X, y, kw = _eval_case(L1, L2, n, "u8", family="prod")
    p = fused_mlp.mlp_unpack(params.double(), L1, L2)
    W1, b1, W2, b2, W3, b3 = p.values()
    assert R.exact_certificate(X, W1, b1).ok
    H1 = torch.relu(X @ W1.t() + b1).to(torch.bfloat16).double()
    assert R.exact_certificate(H1, W2, b2).ok
    H2 = torch.relu(H1 @ W2.t() + b2).to(torch.bfloat16).double()
    Z, ez = R.ref_logits(H2, W3, b3)
    c3 = R.exact_certificate(H2, W3, b3)
    if c3.ok:
        ez = torch.zeros_like(ez)
    emax = ez.max(1, keepdim=True).values
    m = Z.max(1, keepdim=True).values
    lse = m + torch.log(torch.exp(Z - m).sum(1, keepdim=True))
    logits = torch.full((n, 10), -7777.0, device=_dev())
    out = torch.zeros((n + 31) // 32, 2, device=_dev())
    fused_mlp.mlp_eval(params.to(_dev()), L1=L1, L2=L2, B=n, out=out, logits=logits, **kw)
    torch.cuda.synchronize()
    # |d(z - lse)| <= 2 max ez, plus the allowance
    c = R.cmp_bound(logits.cpu().double(), Z - lse, 2.0 * emax + R.SOFT * (Z.abs() + lse.abs()))
    bad = R.report(f"G prod {L1}/{L2} n={n} (layer 3 certified: {c3.ok})", [("logp", c)], WORST)
    assert not bad, bad


def test_zz_worst_ratios_of_this_file():
    """Prints the per-stage maxima the tests above collected (the figures of the docstring)."""
    print("[bound ratio] worst per stage: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values()), WORST
