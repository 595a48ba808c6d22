"""Ragged layer widths without a GPU: predicates, arena packings and the engine's reference path on an
aligned arena."""
import pytest
import torch

import mlp_reference as R
from ray_lightning_accelerators_amd import _C as ext
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.arena import ParamArena
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine


@pytest.mark.parametrize("L1,L2,general,supported", [
    (33, 64, True, True), (1, 1, True, True), (512, 511, True, True), (32, 64, False, True),
    (0, 64, False, False), (513, 64, False, False), (64, 513, False, False),
    (80, 64, False, False), (33, 496, False, False)])   # odd multiples of 16 have no kernel
def test_predicates(L1, L2, general, supported):
    assert fused_mlp.mlp_general(L1, L2) is general is ext.mlp_general_supported(L1, L2)
    assert fused_mlp.mlp_supported(L1, L2) is supported
    if not supported:
        with pytest.raises(ValueError, match="no fused"):
            FusedMLPEngine(L1, L2, 32, device="cpu")


@pytest.mark.parametrize("L1,L2,align", [(33, 31, 4), (300, 100, 1), (1, 1, 4), (96, 40, 1)])
def test_param_arena_packs_the_classifier_as_the_kernels_read_it(L1, L2, align):
    from ray_lightning_accelerators_amd.models.mnist import MNISTClassifier

    arena = ParamArena(MNISTClassifier({"layer_1": L1, "layer_2": L2, "lr": 1e-3, "batch_size": 32}))
    offs = fused_mlp.mlp_arena_offsets(L1, L2, align)
    assert [o for o, _ in arena.offsets] == list(offs[:6])
    assert (offs == fused_mlp.mlp_arena_offsets(L1, L2, 1)) is (align == 1)     # dense only for multiples of 4
    assert all(ext.mlp_general_param_count(L1, L2, al) == fused_mlp.mlp_param_count(L1, L2, al) for al in (1, 4))


def test_cpu_engine_on_an_aligned_arena_steps_as_on_the_dense_one(L1=33, L2=31, B=8):
    x, y = R.random_data(2 * B, 5)
    order, engines = torch.randperm(2 * B, generator=torch.Generator().manual_seed(5)), []
    for align in (1, 4):
        engines.append(FusedMLPEngine(L1, L2, B, lr=1e-2, device="cpu", stats_ring=4, seed=5, arena_align=align))
        engines[-1].attach_dataset(x, y)
        engines[-1].begin_epoch(order, 2)
        engines[-1].run(2)
    a, b = engines
    assert b.params.numel() == fused_mlp.mlp_param_count(L1, L2, 4) > a.params.numel()
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items()) and torch.equal(a.stats, b.stats)
