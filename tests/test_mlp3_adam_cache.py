"""The one-launch step's cache of Adam's bias corrections (csrc/mlp_step3.hip).

Block 0 of every one-launch step parks 1 - beta1^t and sqrt(1 - beta2^t) for the NEXT
step in four spare words of ``hand``, keyed by (t, bits(beta1), bits(beta2)); the other
blocks of the next launch take them from there instead of evaluating two f64 pow()
each, and compute them as before when the key does not match.  The learning rate is
never cached.

Oracle throughout: a second engine running the unchanged two-launch step
(``one_launch = False``), given the same treatment; ``params``, ``exp_avg``,
``exp_avg_sq`` and ``shadow`` are compared bit for bit.  A cached value that differed
in one bit from what the two pow() give would show in the first step that uses it.
"""
import struct

import pytest
import torch

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

gpu = pytest.mark.gpu

SHAPES = [(32, 64, 32), (128, 64, 17)]
LAY = fused_mlp.ADAM_CACHE_LAYOUT
NAN64 = 0x7FF8000000000000


def _dev():
    return torch.device("cuda", 0)


def _data(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = 3 * B + B // 2 + 3  # three batches per epoch: every test crosses an epoch switch
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _pair(L1, L2, B, seed=0, **kw):
    """(one-launch engine, two-launch oracle) on the same data from the same weights."""
    kw.setdefault("lr", 1e-2)
    x, y = _data(B, seed)
    a = FusedMLPEngine(L1, L2, B, device=_dev(), **kw)
    b = FusedMLPEngine(L1, L2, B, device=_dev(), **kw)
    assert a.one_launch
    b.one_launch = False
    a.set_data(x, y)
    b.set_data(x, y)
    return a, b


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _assert_same(a, b):
    torch.cuda.synchronize()
    a.check()
    assert int(a.counters[0]) == int(b.counters[0])
    for k in ("params", "exp_avg", "exp_avg_sq", "shadow"):
        pa, pb = _bits(getattr(a, k)), _bits(getattr(b, k))
        assert torch.equal(pa, pb), (k, int((pa != pb).sum()))


def _betas_key(betas):
    b1, b2 = (struct.unpack("<I", struct.pack("<f", float(v)))[0] for v in betas)
    return b1 | (b2 << 32)


def _cache(e):
    w = [int(v) & (2 ** 64 - 1) for v in e.hand[LAY["step"]:LAY["bc2_sqrt"] + 1].tolist()]
    return dict(zip(("step", "betas", "bc1", "bc2_sqrt"), w))


def _assert_key(e, msg=""):
    """The entry is for the step the next launch will take, under this engine's betas,
    and holds two finite doubles in (0, 1]."""
    c = _cache(e)
    assert c["step"] == int(e.counters[0]) + 1, (msg, c, int(e.counters[0]))
    assert c["betas"] == _betas_key(e.betas), (msg, c)
    for k in ("bc1", "bc2_sqrt"):
        v = struct.unpack("<d", struct.pack("<Q", c[k]))[0]
        assert 0.0 < v <= 1.0, (msg, k, v)
    return c


def _poke(e, **words):
    for k, v in words.items():
        v &= 2 ** 64 - 1
        e.hand[LAY[k]] = v - 2 ** 64 if v >= 2 ** 63 else v


# ------------------------------------------------------------------ CPU
def test_adam_cache_layout_python_mirror():
    """The cache occupies spare words 20..23 of ``hand``, as csrc/mlp_step3.hip documents
    (kHandAdamStep / Betas / Bc1 / Bc2); the pinned hand layout is unchanged."""
    assert fused_mlp.mlp3_adam_cache_layout(native=False) == {"step": 20, "betas": 21, "bc1": 22, "bc2_sqrt": 23}
    assert fused_mlp.HAND_LAYOUT == {"ack": 0, "err": 16, "sat": 17, "nonfinite": 18, "last_step": 19, "words": 32}
    assert fused_mlp.mlp3_hand_layout(native=False) == fused_mlp.HAND_LAYOUT
    used = set(fused_mlp.HAND_LAYOUT.values()) - {fused_mlp.HAND_LAYOUT["words"]}
    mine = set(fused_mlp.ADAM_CACHE_LAYOUT.values())
    assert len(mine) == 4 and not (mine & used) and max(mine) < fused_mlp.mlp3_hand_words(32, 64)


@gpu
def test_adam_cache_layout_from_the_extension():
    from ray_lightning_accelerators_amd import ops

    assert dict(ops.require().mlp3_adam_cache_layout()) == fused_mlp.ADAM_CACHE_LAYOUT
    assert fused_mlp.mlp3_adam_cache_layout() == fused_mlp.ADAM_CACHE_LAYOUT


# ------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("L1,L2,B,wd", [(32, 64, 32, 0.0), (128, 64, 17, 0.0), (32, 64, 32, 0.01)])
def test_hits_every_step(L1, L2, B, wd):
    """A fresh ``hand`` has no entry (key 0); after every one-launch step the key names
    the next step, and the steps that consume the entries stay on the oracle's bits.  The
    same step's entry is the same words on every engine and differs from step to step."""
    a, b = _pair(L1, L2, B, weight_decay=wd)
    assert _cache(a) == {"step": 0, "betas": 0, "bc1": 0, "bc2_sqrt": 0}
    seen = []
    for s in range(8):
        a.step()
        b.step()
        seen.append(_assert_key(a, s))
        _assert_same(a, b)
    assert [c["step"] for c in seen] == list(range(2, 10))
    assert len({c["bc1"] for c in seen}) == 8 and len({c["bc2_sqrt"] for c in seen}) == 8
    assert _cache(b)["step"] == 0  # the two-launch step neither reads nor writes the cache
    a2, _ = _pair(L1, L2, B, seed=1, weight_decay=wd)
    a2.run(3)
    torch.cuda.synchronize()
    assert _cache(a2) == seen[2]  # other data, same (step, betas): the same entry


@gpu
def test_matching_entry_is_what_the_step_uses():
    """The hit path is live: other values under a MATCHING key change the step (the
    counterpart of the poisoned-entry test below, where the key does not match)."""
    a, b = _pair(32, 64, 32)
    a.run(2)
    b.run(2)
    one = struct.unpack("<Q", struct.pack("<d", 1.0))[0]
    _assert_key(a)
    _poke(a, bc1=one, bc2_sqrt=one)  # "no bias correction" for step 3
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert not torch.equal(a.params, b.params)
    assert bool(torch.isfinite(a.params).all())


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_set_step_misses_once(L1, L2, B):
    a, b = _pair(L1, L2, B)
    a.run(3)
    b.run(3)
    for e in (a, b):
        e.set_step(40)
    assert _cache(a)["step"] == 4  # stale: the next launch needs step 41
    a.step()
    b.step()
    _assert_same(a, b)
    assert _assert_key(a)["step"] == 42
    a.run(3)
    b.run(3)
    _assert_same(a, b)
    _assert_key(a)


def _continue_fresh(src, one_launch, x, y, betas=None, copy_cache_from=None):
    """A fresh engine holding ``src``'s checkpoint: weights through ``state_dict``, Adam
    state and step through ``optimizer_state_dict``."""
    sd, od = src.state_dict(), src.optimizer_state_dict()
    flat = torch.cat([v.reshape(-1) for v in sd.values()])
    e = FusedMLPEngine(src.L1, src.L2, src.B, lr=src.lr, betas=betas or src.betas, weight_decay=src.wd,
                       device=_dev(), init_params=flat)
    e.exp_avg.copy_(torch.cat([od["state"][i]["exp_avg"].reshape(-1) for i in range(len(sd))]))
    e.exp_avg_sq.copy_(torch.cat([od["state"][i]["exp_avg_sq"].reshape(-1) for i in range(len(sd))]))
    e.one_launch = one_launch
    e.set_data(x, y)
    e.set_step(int(od["state"][0]["step"].item()))
    if copy_cache_from is not None:
        lo, hi = LAY["step"], LAY["bc2_sqrt"] + 1
        e.hand[lo:hi].copy_(copy_cache_from.hand[lo:hi])
    return e


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_checkpoint_into_a_fresh_engine(L1, L2, B):
    a, b = _pair(L1, L2, B)
    a.run(4)
    b.run(4)
    _assert_same(a, b)
    x, y = _data(B, seed=2)
    a2, b2 = _continue_fresh(a, True, x, y), _continue_fresh(b, False, x, y)
    assert _cache(a2)["step"] == 0 and int(a2.counters[0]) == 4
    a2.step()
    b2.step()
    _assert_same(a2, b2)
    assert _assert_key(a2)["step"] == 6
    a2.run(3)
    b2.run(3)
    _assert_same(a2, b2)


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_alternating_with_the_two_launch_step(L1, L2, B):
    """A two-launch step in between leaves an entry for a step that has passed: the next
    one-launch step misses, and leaves the entry for its successor."""
    a, b = _pair(L1, L2, B)
    for s in range(10):
        a.one_launch = s % 3 != 1
        before = _cache(a)
        a.step()
        b.step()
        if a.one_launch:
            _assert_key(a, s)
        else:
            assert _cache(a) == before  # the two-launch step leaves the words alone
        _assert_same(a, b)


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_other_betas_continue_another_engines_state(L1, L2, B):
    """The entry a run with betas (0.9, 0.999) left -- right step, other betas -- in the
    ``hand`` of an engine that continues with (0.8, 0.99): ignored."""
    a, b = _pair(L1, L2, B)
    a.run(3)
    b.run(3)
    x, y = _data(B, seed=3)
    a2 = _continue_fresh(a, True, x, y, betas=(0.8, 0.99), copy_cache_from=a)
    b2 = _continue_fresh(b, False, x, y, betas=(0.8, 0.99))
    c = _cache(a2)
    assert c["step"] == 4 and c["betas"] == _betas_key((0.9, 0.999)) != _betas_key(a2.betas)
    for s in range(4):
        a2.step()
        b2.step()
        _assert_key(a2, s)
        _assert_same(a2, b2)


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_lr_is_not_cached_eager(L1, L2, B):
    a, b = _pair(L1, L2, B)
    for s, lr in enumerate((1e-2, 3e-3, 3e-3, 5e-2, 1e-4, 2e-2)):
        for e in (a, b):
            e.set_lr(lr)
        a.step()
        b.step()
        _assert_key(a, s)
        _assert_same(a, b)


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_lr_is_not_cached_in_a_graph(L1, L2, B):
    """``set_lr`` between replays of a captured 3-step graph reaches the replayed kernels
    through ``lr_tensor`` (one epoch is three batches: a replay is one epoch)."""
    a, b = _pair(L1, L2, B)
    a.run(2)
    b.run(2)
    assert a.capture(3, remainders=False)  # runs one real step: the epoch ends here
    b.run(1)
    for lr in (4e-3, 3e-2, 1e-3):
        for e in (a, b):
            e.set_lr(lr)
        assert a._graph_ok(3)
        a.run(3)
        b.run(3)
        _assert_key(a, lr)
        _assert_same(a, b)
    assert a.global_step == b.global_step == 12


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_poisoned_entry_under_another_key_is_ignored(L1, L2, B):
    a, b = _pair(L1, L2, B)
    a.run(3)
    b.run(3)
    _poke(a, step=int(a.counters[0]) + 7, bc1=NAN64, bc2_sqrt=NAN64 | 1)
    a.step()
    b.step()
    _assert_same(a, b)
    assert bool(torch.isfinite(a.params).all())
    assert _assert_key(a)["step"] == 5
    # and a zero step never matches, whatever the rest says
    _poke(a, step=0, bc1=NAN64, bc2_sqrt=NAN64)
    a.run(2)
    b.run(2)
    _assert_same(a, b)
    _assert_key(a)


@gpu
@pytest.mark.parametrize("L1,L2,B", SHAPES)
def test_graph_replay_hits_match_eager(L1, L2, B):
    """Four steps per graph: the second to fourth launch of a replay consume the entry
    their predecessor in the same graph wrote, the first the entry of the previous
    replay (or of the 1-step remainder graph).  The oracle steps eagerly."""
    a, b = _pair(L1, L2, B)
    x, y = _data(B, seed=4)
    g = torch.Generator().manual_seed(5)
    x = torch.cat([x, torch.randint(0, 256, (2 * B, 784), generator=g, dtype=torch.uint8)])
    y = torch.cat([y, torch.randint(0, 10, (2 * B,), generator=g)])
    for e in (a, b):
        e.set_data(x, y)  # five batches per epoch
    assert a.n_batches == 5
    assert a.capture(4)  # one real step, then the 4-step graph and its 1 / 2-step remainders
    b.run(1)
    for n in (4, 5, 1):  # a replay ends epoch 0; epoch 1: a replay + the 1-step graph; one more step
        assert n == 1 or a._graph_ok(n)  # the dispatch begins with a replay of the 4-step graph
        a.run(n)
        b.run(n)
        _assert_key(a, n)
        _assert_same(a, b)
    assert a.global_step == b.global_step == 11
