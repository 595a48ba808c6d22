"""General layer widths (``fused_mlp.mlp_general``: multiples of 32 up to 512 outside the table)
without a GPU: the predicates, the Python mirror of the workspace layout, and the engine on the
fp32 reference path."""
import pytest
import torch

import mlp_reference as R
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine


@pytest.mark.parametrize("L1,L2,general,supported", [
    (96, 160, True, True), (512, 512, True, True), (256, 32, True, True), (32, 512, True, True),
    (32, 64, False, True), (128, 256, False, True),            # table pairs stay the table's
    (0, 64, False, False), (16, 64, False, False), (48, 64, False, False), (64, 48, False, False),
    (544, 64, False, False), (64, 544, False, False), (-32, 64, False, False)])
def test_predicates_at_the_boundaries(L1, L2, general, supported):
    assert fused_mlp.mlp_general(L1, L2) is general and fused_mlp.mlp_supported(L1, L2) is supported


@pytest.mark.parametrize("L1,L2,B", [(96, 32, 1), (160, 96, 65), (512, 512, 4096), (64, 128, 320)])
def test_layout_is_disjoint_covers_the_park_and_matches_the_extension(L1, L2, B):
    lay = fused_mlp.mlp_general_layout(L1, L2, B)
    Bp = lay["Bp"]
    assert Bp == -(-B // 64) * 64 and lay["ncb"] == -(-L1 // 64) and lay["h1_elems"] == Bp * L1
    spans = sorted((lay[k], lay[k] + n * Bp) for k, n in (("xt", 784), ("h1t", L1), ("h2t", L2), ("dh2t", L2),
                                                          ("dzt", 16), ("dh1t", L1), ("h1", L1)))
    assert spans[0][0] == 0 and spans[-1][1] == lay["park_elems"]
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))            # back to back: disjoint, no gap
    assert lay["part_elems"] == lay["slices"] * lay["np_pad"] + lay["nslab"] * 4 and 1 <= lay["slices"] <= Bp // 32
    from ray_lightning_accelerators_amd import _C as ext
    assert {k: lay[k] for k in ext.mlp_general_layout(L1, L2, B)} == dict(ext.mlp_general_layout(L1, L2, B))
    assert ext.mlp_general_supported(L1, L2) is fused_mlp.mlp_general(L1, L2)


def test_cpu_engine_steps_general_widths_as_the_reference_op():
    L1, L2, B = 96, 160, 32
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
    assert eng.general and eng.wide and not eng.one_launch and eng.shadow is None
    assert torch.equal(eng.params, q) and torch.equal(eng.exp_avg_sq, v) and torch.equal(eng.stats, stats)
    assert eng.counters[:2].tolist() == [2, 0]


@pytest.mark.parametrize("kw", [dict(clip_norm=1.0), dict(accumulate=2), dict(optimizer="sgd"),
                                dict(dp_context=[1, 0, 0, 0, 0, 0, 0]), dict(lr_ring=4, world_size=2)],
                         ids=lambda k: next(iter(k)))
def test_engine_refuses_at_general_widths_what_the_wide_step_refuses(kw):
    with pytest.raises(ValueError, match="table widths only"):
        FusedMLPEngine(96, 160, 32, device="cpu", **kw)
    with pytest.raises(ValueError, match="no fused kernel"):
        FusedMLPEngine(96, 544, 32, device="cpu")
