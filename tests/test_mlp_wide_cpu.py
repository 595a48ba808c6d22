"""Batches above 256 rows on the CPU reference path: the engine accepts them up to
``fused_mlp.WIDE_MAX_B`` and steps exactly as ``mlp_train_step``'s fp32 reference does."""
import pytest
import torch

import mlp_reference as R
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine


def test_cpu_engine_steps_batch_512_as_the_reference_op():
    L1, L2, B = 32, 64, 512
    x, y = R.random_data(2 * B, 3)
    p = R.random_params(L1, L2, 3)
    order = torch.randperm(2 * B, generator=torch.Generator().manual_seed(3))
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, device="cpu", init_params=p, stats_ring=4)
    eng.attach_dataset(x, y)
    eng.begin_epoch(order, 2)
    eng.run(2)
    q, g, m, v = p.clone(), torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    stats, counters = torch.zeros(4, 4), torch.zeros(2, dtype=torch.int64)
    for _ in range(2):
        fused_mlp.mlp_train_step(q, g, L1=L1, L2=L2, B=B, labels=y, x_u8=x, order=order, counters=counters,
                                 n_batches=2, exp_avg=m, exp_avg_sq=v, stats=stats, apply_adam=True, lr=1e-2)
    assert eng.wide and torch.equal(eng.params, q) and torch.equal(eng.exp_avg_sq, v) and torch.equal(eng.stats, stats)
    assert eng.counters[:2].tolist() == [2, 0] and eng.health()["saturated"] == 0


def test_batch_sizes_above_the_wide_limit_still_raise():
    assert fused_mlp.WIDE_MAX_B == 4096
    with pytest.raises(ValueError, match="4096"):
        FusedMLPEngine(32, 64, 4097, device="cpu")
    p = R.random_params(32, 64, 1)
    with pytest.raises(ValueError, match="4096"):
        fused_mlp.mlp_train_step(p, torch.zeros_like(p), L1=32, L2=64, B=4097, labels=torch.zeros(4097, dtype=torch.long),
                                 x_f32=torch.zeros(4097, 784))


def test_layout_matches_the_extension():
    from ray_lightning_accelerators_amd import _C as ext
    for (L1, L2), B in ((w, b) for w in sorted(fused_mlp.SUPPORTED) for b in (257, 320, 513, 4096)):
        lay = fused_mlp.mlp_wide_layout(L1, L2, B)
        assert {k: lay[k] for k in ext.mlp_wide_layout(L1, L2, B)} == dict(ext.mlp_wide_layout(L1, L2, B)), (L1, L2, B)
