"""The row-chain form of the one-launch step's replicated head pass (csrc/mlp_step3.hip,
``RowChain``): waves 0-3 own row tile 0 and waves 4-7 row tile 1; the block stages the bf16
shadow weights once in LDS instead of every wave loading its own fragments; every wave
computes its row tile's logits and runs the softmax of four rows on its own accumulators;
H2 / dH2 reach the next MFMA through the transposed LDS images; and the block's
acknowledgement goes out from an LDS arrival count instead of behind a barrier of its own.

Every tile is the same MFMA sequence over K, every bf16 rounding sits at the same point and
the softmax keeps its per-row arithmetic, so the oracle throughout is the two-launch step
(``one_launch = False``, whose head is not touched) from the same weights on the same data,
compared with ``torch.equal`` on the bits of ``params``, both moments, the bf16 shadows,
both H1pre slots, the X and label rings and the stats rows.

Widths: the form is compiled where ``RowChain::fits`` holds (mirrored by ``_admitted``
below): 32-32, 32-64 (the flagship) and 64-64.  128-256 stands for the widths that keep the
parent form.  Batch sizes: 32 (both row tiles full), 17 (one real row in row tile 1), 16
(row tile 1 pure padding), 1 (15 padded rows in row tile 0); padded rows carry label -1,
write zeros and are not counted (the stats row's count is the batch size).
"""
import pytest
import torch

from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

gpu = pytest.mark.gpu

BUFFERS = ("params", "exp_avg", "exp_avg_sq", "shadow", "h1pre", "xring", "yring", "stats")
HAND = fused_mlp.HAND_LAYOUT
LAY = fused_mlp.ADAM_CACHE_LAYOUT
ALL_WIDTHS = [(32, 32), (32, 64), (32, 128), (32, 256), (64, 64), (64, 128), (64, 256), (128, 64), (128, 128),
              (128, 256)]
BATCHES = [32, 17, 16, 1]


def _admitted(L1, L2):
    """``RowChain<L1, L2>::fits``: no K split (L2 < 128), a 4-wave row group has a wave for
    every column tile, and staging the four shadow matrices costs a thread no more 16-byte
    loads than the weight fragments of the parent form did."""
    tn1, tn2 = L1 // 16, L2 // 16
    parent_frags = L1 // 32 + 1 + L2 // 32 + L2 // 32
    chunks = L2 * L1 // 8 + 10 * L2 // 8 + L2 * 2 + L1 * L2 // 8
    loads = (chunks + 511) // 512
    return L2 < 128 and tn1 <= 4 and tn2 <= 4 and loads <= parent_frags


ADMITTED = [w for w in ALL_WIDTHS if _admitted(*w)]
WIDTHS = ADMITTED + [(128, 256)]


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
    """No hand-off timeout, and exactly one acknowledgement per block per launch: the
    arrival count elects one wave of every block."""
    torch.cuda.synchronize()
    e.check()
    assert int(e.hand[HAND["err"]]) == 0
    assert int(e.hand[HAND["ack"]]) == launches * _grid(e.L1, e.L2), (launches, _grid(e.L1, e.L2))


def _health(e):
    return [int(e.hand[HAND[k]]) for k in ("sat", "nonfinite", "last_step")]


def _cache(e):
    return [int(v) for v in e.hand[LAY["step"]:LAY["bc2_sqrt"] + 1].tolist()]


# ------------------------------------------------------------------ CPU
def test_admitted_widths():
    """The flagship is mandatory, 128-256 certainly out; the mirror of the predicate admits
    exactly the three narrow widths."""
    assert ADMITTED == [(32, 32), (32, 64), (64, 64)]


# ------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L1,L2", WIDTHS)
def test_twelve_steps_bitwise(L1, L2, B):
    a, b = _pair(L1, L2, B)
    for s in range(12):
        a.step()
        b.step()
        _assert_same(a, b, s)
        # labels -1 (rows >= B) count nothing
        assert float(a.stats[s % a.stats.size(0), 2]) == float(B), (s, a.stats[s % a.stats.size(0)])
    _assert_healthy(a, 12)


@gpu
@pytest.mark.parametrize("lr", [1e-2, 1e-1])
@pytest.mark.parametrize("L1,L2", ADMITTED)
def test_health_words_and_adam_cache_entry(L1, L2, lr):
    """The layer-1 health words against the two-launch step's (lr 0.1 is the benchmark's,
    where the clamp does fire in a longer run), every state buffer with them, and the Adam
    cache entry: keyed for the next step, no further word of ``hand`` written (the entry's
    values against the host's float64 are tests/test_mlp3_prologue.py's)."""
    a, b = _pair(L1, L2, 32, n_batches=8, lr=lr)
    a.run(12)
    b.run(12)
    _assert_same(a, b)
    assert _health(a) == _health(b)
    c = _cache(a)
    assert c[0] == int(a.counters[0]) + 1 == 13
    assert not bool(a.hand[LAY["bc2_sqrt"] + 1:HAND["words"]].any())
    _assert_healthy(a, 12)


@gpu
def test_probe_instance_computes_what_the_production_instance_does():
    """32-64 with ``stamps`` set (the probe instance) and with it null; the stamps of block
    0's wave 0 are ordered: first load < H1 in LDS < end of the forward part < end of the chain."""
    a, b = _pair(32, 64, 32, n_batches=8, oracle_one_launch=True)
    a.run(2)
    b.run(2)
    st = torch.zeros(4, 16, dtype=torch.int64, device=_dev())
    for i in range(4):
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1, stamps=st[i], stats=a.stats, **a._kw3())
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1, stats=b.stats, **b._kw3())
    _assert_same(a, b)
    assert _cache(a) == _cache(b)
    assert bool((st[:, 0] > 0).all())
    for k in range(3):
        assert bool((st[:, k + 1] > st[:, k]).all()), (k, st[:, :4])
    assert bool((st[:, 11] > st[:, 3]).all())
    _assert_healthy(a, 6)
    _assert_healthy(b, 6)


@gpu
@pytest.mark.parametrize("B", [32, 17])
def test_eager_against_graph_replay(B):
    """24 eager steps against 3 replays of an 8-step graph (one epoch is 25 batches)."""
    a, b = _pair(32, 64, B, n_batches=25, oracle_one_launch=True)
    assert a.capture(8, remainders=False)
    b.run(1)
    for _ in range(3):
        assert a._graph_ok(8)
        a.run(8)
    b.run(24)
    assert a.global_step == b.global_step == 25
    _assert_same(a, b)
    assert _cache(a) == _cache(b)
    _assert_healthy(a, 25)
    _assert_healthy(b, 25)


@gpu
@pytest.mark.parametrize("proto", ["packed", "owner"])
def test_loopback_exchange_at_world_one(proto):
    """The exchange instances share the head pass.  Loopback at world 1 (this process is the
    only rank: the exchanged sum is this rank's own gradient times 1): the parameters of the
    plain one-launch step, bit for bit, over eager steps and graph replays."""
    from test_mlp3 import _loopback_ctx

    x, y = _data(32, 12)
    c, ctx = _loopback_ctx(1)
    lb = FusedMLPEngine(32, 64, 32, lr=1e-2, device=_dev(), dp_context=ctx, dp_proto=proto, dp_loop=True)
    ref = FusedMLPEngine(32, 64, 32, lr=1e-2, device=_dev())
    assert lb.one_launch_dp and lb.dp_ctx[0] == 1 and ref.one_launch
    lb.set_data(x, y)
    ref.set_data(x, y)
    for s in range(3):
        lb.run(1)
        ref.run(1)
        torch.cuda.synchronize()
        d = (lb.params - ref.params).abs().max().item()
        print(f"loopback {proto} world 1, step {s}: max |dp - plain| {d:.3e}")
        assert torch.equal(_bits(lb.params), _bits(ref.params)), (proto, s, d)
    assert lb.capture(4, remainders=False)  # runs one step itself
    ref.run(1)
    lb.run(8)
    ref.run(8)
    torch.cuda.synchronize()
    assert lb.global_step == ref.global_step == 12
    assert c.error_state() == 0, c.error_message()
    lb.check()
    assert torch.equal(_bits(lb.params), _bits(ref.params)), proto
    assert torch.equal(_bits(lb.stats), _bits(ref.stats)), proto
