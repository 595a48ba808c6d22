"""The one-launch step's prologue (csrc/mlp_step3.hip): the kernel arguments fetched in one
batch, the step state (counters, launch sequence number, Adam cache entry, learning rate)
in a second one that is waited for behind the head pass's loads, and the phase stamps only
in the probe instances.  The Adam cache entry keeps its four words (the wider entry with
the learning rate was measured and not kept): the learning rate is never cached.

Oracle throughout: the two-launch step (``one_launch = False``) from the same weights on
the same data, compared with ``torch.equal`` on the bits of ``params``, both moments, the
bf16 shadows, both H1pre slots, the X and label rings and the stats rows.  Every case ends
with the hand-off's error word at 0 and its acknowledgement word at launches x grid.
"""
import struct

import numpy as np
import pytest
import torch

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

gpu = pytest.mark.gpu

WIDTHS = [(32, 64), (32, 128), (128, 256)]
BATCHES = [32, 17, 1]
BUFFERS = ("params", "exp_avg", "exp_avg_sq", "shadow", "h1pre", "xring", "yring", "stats")
LAY = fused_mlp.ADAM_CACHE_LAYOUT
HAND = fused_mlp.HAND_LAYOUT
# f64 pow() on the device against the host's: OpenCL allows pow 16 ulp, 1.8e-15 absolute
# for a power below 1; the smallest correction compared here is 1 - 0.999 = 1e-3, so the
# relative error of a correction stays below 1.8e-12 (its square root's below half of that)
BC_RTOL = 2e-12


def _dev():
    return torch.device("cuda", 0)


def _data(B, n_batches, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = n_batches * B + B // 2
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


def _pair(L1, L2, B, n_batches=5, oracle_one_launch=False, **kw):
    """(one-launch engine, oracle) on the same data from the same weights."""
    kw.setdefault("lr", 1e-2)
    x, y = _data(B, n_batches)
    a = FusedMLPEngine(L1, L2, B, device=_dev(), **kw)
    b = FusedMLPEngine(L1, L2, B, device=_dev(), **kw)
    assert a.one_launch
    b.one_launch = oracle_one_launch
    a.set_data(x, y)
    b.set_data(x, y)
    assert a.n_batches == n_batches
    return a, b


def _grid(L1, L2):
    """Blocks of the one-launch step: block 0, the 49 W1 tiles, 8 small tasks per block."""
    tn1, tn2 = L1 // 16, L2 // 16
    ntask = tn1 * tn2 + tn2 + (L1 + L2 + 10 + 63) // 64
    return 1 + fused_mlp.W1_TILES + (ntask + 7) // 8


def _bits(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(a, b, msg=""):
    torch.cuda.synchronize()
    assert int(a.counters[0]) == int(b.counters[0]), msg
    for k in BUFFERS:
        pa, pb = _bits(getattr(a, k)), _bits(getattr(b, k))
        assert torch.equal(pa, pb), (msg, k, int((pa != pb).sum()))


def _assert_healthy(e, launches):
    torch.cuda.synchronize()
    e.check()
    assert int(e.hand[HAND["err"]]) == 0
    assert int(e.hand[HAND["ack"]]) == launches * _grid(e.L1, e.L2), (launches, _grid(e.L1, e.L2))


def _f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def _betas_key(betas):
    return _f32_bits(betas[0]) | (_f32_bits(betas[1]) << 32)


def _cache(e):
    w = [int(v) & (2 ** 64 - 1) for v in e.hand[LAY["step"]:LAY["bc2_sqrt"] + 1].tolist()]
    return dict(zip(("step", "betas", "bc1", "bc2_sqrt"), w))


def _f64(word):
    return struct.unpack("<d", struct.pack("<Q", word))[0]


def _assert_entry(e, msg=""):
    """The entry is the one the NEXT launch looks for, its words are adam_scalars' evaluated
    on the host in float64 (1 - beta1^t, sqrt(1 - beta2^t)), and no other spare word of
    ``hand`` is written (the learning rate is not part of the entry)."""
    torch.cuda.synchronize()
    c = _cache(e)
    t = int(e.counters[0]) + 1
    assert c["step"] == t, (msg, c)
    assert c["betas"] == _betas_key(e.betas), (msg, c)
    b1, b2 = (float(np.float32(v)) for v in e.betas)
    bc1, bc2s = _f64(c["bc1"]), _f64(c["bc2_sqrt"])
    assert abs(bc1 - (1.0 - b1 ** t)) <= BC_RTOL * (1.0 - b1 ** t), (msg, bc1)
    assert abs(bc2s - (1.0 - b2 ** t) ** 0.5) <= BC_RTOL * (1.0 - b2 ** t) ** 0.5, (msg, bc2s)
    assert not bool(e.hand[LAY["bc2_sqrt"] + 1:HAND["words"]].any()), msg
    return c


# ------------------------------------------------------------------ CPU
def test_grid_of_the_flagship():
    """The acknowledgement target of the tests below: 1 + 49 + 2 blocks at 32-64."""
    assert _grid(32, 64) == 52 and fused_mlp.mlp3_adam_cache_layout(native=False) == LAY


# ------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L1,L2", WIDTHS)
def test_twelve_steps_bitwise(L1, L2, B):
    """From a fresh engine: the first step misses the cache, the rest hit it (17 rows: the
    padded rows and clamped addresses; 1 row: the smallest batch)."""
    a, b = _pair(L1, L2, B)
    assert _cache(a)["step"] == 0
    for s in range(12):
        a.step()
        b.step()
        _assert_same(a, b, s)
        _assert_entry(a, s)
    _assert_healthy(a, 12)


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (128, 256, 17)])
def test_device_learning_rate_changes_between_steps(L1, L2, B):
    """Written to ``lr_ptr`` on the device: steps 3 and 4 with two other values, step 5
    back.  Every step hits the cache (the key is the step and the betas) and divides the
    learning rate it reads itself: the learning rate is never cached."""
    a, b = _pair(L1, L2, B, n_batches=8)
    lrs = [1e-2, 1e-2, 3e-3, 5e-2, 1e-2, 1e-2, 1e-2]
    for s, lr in enumerate(lrs):
        for e in (a, b):
            e.lr_tensor.fill_(lr)
        a.step()
        b.step()
        _assert_same(a, b, s)
        _assert_entry(a, s)
    _assert_healthy(a, len(lrs))


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (32, 128, 17)])
def test_other_misses_then_hits(L1, L2, B):
    """A far step, other betas, a two-launch step in between: the next one-launch step
    finds an entry under another key, and leaves the one its successor finds."""
    a, b = _pair(L1, L2, B, n_batches=8)
    a.run(2)
    b.run(2)
    launches = 2
    _assert_same(a, b)
    # a far step
    for e in (a, b):
        e.set_step(1000)
    assert _cache(a)["step"] == 3
    for s in range(2):
        a.step()
        b.step()
        _assert_same(a, b, ("set_step", s))
        assert _assert_entry(a)["step"] == 1002 + s
    launches += 2
    # other betas
    for e in (a, b):
        e.betas = (0.8, 0.99)
    assert _cache(a)["betas"] == _betas_key((0.9, 0.999)) != _betas_key(a.betas)
    for s in range(2):
        a.step()
        b.step()
        _assert_same(a, b, ("betas", s))
        _assert_entry(a)
    launches += 2
    # a two-launch step in between
    a.one_launch = False
    before = _cache(a)
    a.step()
    b.step()
    _assert_same(a, b, "two-launch")
    assert _cache(a) == before and before["step"] == int(a.counters[0])  # for a step that has passed
    a.one_launch = True
    for s in range(2):
        a.step()
        b.step()
        _assert_same(a, b, ("after two-launch", s))
        _assert_entry(a)
    launches += 2
    _assert_healthy(a, launches)


@gpu
@pytest.mark.parametrize("L1,L2", [(32, 64), (128, 256)])
def test_probe_instance_computes_what_the_production_instance_does(L1, L2):
    """The same engine state stepped 4 times with ``stamps`` set (the probe instance: the
    only one with stamps compiled in) and with it null (the production instance)."""
    a, b = _pair(L1, L2, 32, n_batches=8, oracle_one_launch=True)
    a.run(2)
    b.run(2)
    st = torch.zeros(4, 16, dtype=torch.int64, device=_dev())
    for i in range(4):
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1, stamps=st[i], stats=a.stats, **a._kw3())
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1, stats=b.stats, **b._kw3())
    _assert_same(a, b)
    assert _cache(a) == _cache(b)
    assert bool((st[:, 0] > 0).all()) and bool((st[:, 11] > st[:, 0]).all())  # the probe did stamp
    _assert_healthy(a, 6)
    _assert_healthy(b, 6)


@gpu
def test_stamps_without_a_probe_instance_are_an_error():
    a, _ = _pair(64, 64, 32)
    a.run(1)
    st = torch.zeros(16, dtype=torch.int64, device=_dev())
    with pytest.raises(RuntimeError):
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1, stamps=st, stats=a.stats, **a._kw3())
    _assert_healthy(a, 1)


@gpu
def test_eager_against_graph_replay():
    """24 eager steps against 3 replays of an 8-step graph (one epoch is 25 batches:
    the step ``capture`` runs first, then exactly three replays)."""
    a, b = _pair(32, 64, 32, n_batches=25, oracle_one_launch=True)
    assert a.capture(8, remainders=False)
    b.run(1)
    for _ in range(3):
        assert a._graph_ok(8)
        a.run(8)
    b.run(24)
    assert a.global_step == b.global_step == 25
    _assert_same(a, b)
    assert _cache(a) == _cache(b)
    _assert_entry(a)
    _assert_healthy(a, 25)
    _assert_healthy(b, 25)
