"""Gradient clipping of the fused MNIST step on the CPU: ``ops.optim.clip_partials``'
torch form against float64 (bound derived in tests/clip_reference.py), and
``FusedMLPEngine(device="cpu", clip_norm=c)`` against torch's own
``clip_grad_norm_`` + ``torch.optim.Adam``."""
import pytest
import torch
import torch.nn.functional as F

import clip_reference as R
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.ops.optim import clip_partials, clip_slices
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices


@pytest.mark.parametrize("nblk", R.NBLKS)
@pytest.mark.parametrize("n", R.SIZES)
def test_clip_partials_fallback_vs_fp64(n, nblk):
    x = R.make_input(n)
    part = clip_partials(x, nblk)
    assert part.shape == (nblk,) and part.dtype == torch.float32
    ref_part, s, bound = R.ref_partials(x, nblk)
    assert clip_slices(n, nblk) == R.slices(n, nblk)
    err = abs(float(part.double().sum()) - s)
    assert err <= bound, (err, bound)
    # every block against its own slice (the total's bound is an upper bound of each), empty slices exactly 0
    assert bool(((part.double() - ref_part).abs() <= bound).all())
    for b, (lo, hi) in enumerate(R.slices(n, nblk)):
        assert hi > lo or float(part[b]) == 0.0
    assert torch.equal(part, clip_partials(x, nblk))
    out = torch.full((nblk,), 7.0)
    assert clip_partials(x, nblk, out=out) is out and torch.equal(out, part)
    # mutant: the scalar tail dropped (every size here but 4 has one) -- beyond the bound
    if n % 4:
        dropped = clip_partials(x[: 4 * (n // 4)], nblk)
        assert abs(float(dropped.double().sum()) - s) > bound


def test_clip_partials_refuses_bad_nblk():
    x = torch.ones(8)
    for nblk in (0, 65, -1):
        with pytest.raises(ValueError):
            clip_partials(x, nblk)
    with pytest.raises(ValueError):
        clip_partials(x, 4, out=torch.zeros(3))


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8), torch.randint(0, 10, (n,), generator=g)


_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def _torch_clipped(p_init, x, y, L1, L2, B, steps, c, lr, seed=0):
    """nn.Linear-shaped fp32 tensors + clip_grad_norm_ + torch.optim.Adam on the engine's batches."""
    ref = {k: v.clone().requires_grad_(True) for k, v in zip(_NAMES, fused_mlp.mlp_unpack(p_init.clone(), L1, L2).values())}
    opt = torch.optim.Adam(list(ref.values()), lr=lr)
    nb = x.size(0) // B
    norms = []
    for s in range(steps):
        epoch, cur = divmod(s, nb)
        idx = shard_indices(x.size(0), 1, 0, epoch, seed, True)[cur * B:(cur + 1) * B]
        h = torch.relu(F.linear(x[idx].float() / 255.0, ref["W1"], ref["b1"]))
        h = torch.relu(F.linear(h, ref["W2"], ref["b2"]))
        loss = F.nll_loss(torch.log_softmax(F.linear(h, ref["W3"], ref["b3"]), 1), y[idx])
        opt.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(ref.values()), c)))
        opt.step()
    return torch.cat([ref[k].detach().reshape(-1) for k in _NAMES]), norms


def test_engine_cpu_clips_like_torch():
    """A bound below every step's norm: all 6 steps clipped, parameters as torch's."""
    L1, L2, B, c = 32, 64, 32, 0.05
    x, y = _data(200, seed=3)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, device="cpu", clip_norm=c)
    eng.set_data(x, y)
    p0 = eng.params.clone()
    for _ in range(6):
        eng.step()
    want, norms = _torch_clipped(p0, x, y, L1, L2, B, 6, c, 1e-2)
    assert min(norms) > c
    assert torch.allclose(eng.params, want, atol=1e-6), (eng.params - want).abs().max()
    h = eng.health()
    assert h["clipped_steps"] == 6 and h["nonfinite_norm_steps"] == 0
    assert abs(h["clip_norm_last"] - norms[-1]) <= 1e-5 * norms[-1]
    assert abs(h["clip_coef_last"] - c / (norms[-1] + 1e-6)) <= 1e-5 * c / norms[-1]


def test_engine_cpu_inactive_clip_is_bitwise_noop():
    """A bound no norm reaches: the run equals the clip_norm=None engine bit for bit."""
    L1, L2, B = 32, 64, 32
    x, y = _data(200, seed=3)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, device="cpu")
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, device="cpu", clip_norm=1e30)
    a.set_data(x, y)
    b.set_data(x, y)
    for _ in range(6):
        a.step()
        b.step()
    for k in ("params", "exp_avg", "exp_avg_sq", "stats", "counters"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    h = b.health()
    assert h["clipped_steps"] == 0 and h["clip_coef_last"] == 1.0
    ha = a.health()
    assert "clipped_steps" not in ha and a.clip_out is None and a.clip_part is None  # an engine that does not clip


def test_engine_cpu_world2_clip_matches_world1():
    """The allreduce route: SUM of two identical ranks, averaged by grad_scale, clips to
    the same norm (x2 and x1/2 are exact, the coefficient's rounding aside)."""
    L1, L2, B, c = 32, 32, 16, 0.05
    x, y = _data(100, seed=5)
    a = FusedMLPEngine(L1, L2, B, lr=1e-2, device="cpu", clip_norm=c)
    b = FusedMLPEngine(L1, L2, B, lr=1e-2, device="cpu", clip_norm=c, allreduce=lambda g: g.mul_(2))
    a.set_data(x, y)
    b.set_data(x, y)
    b.world_size = 2  # after set_data: same shard (5 steps < 2 epochs)
    for _ in range(5):
        a.step()
        b.step()
    assert torch.allclose(a.params, b.params, atol=1e-6)
    assert a.health()["clipped_steps"] == b.health()["clipped_steps"] == 5


def test_engine_refuses_dp_context_with_clip_norm():
    with pytest.raises(ValueError, match="dp_context"):
        FusedMLPEngine(32, 64, 32, device="cpu", clip_norm=1.0, dp_context=[2, 0, 1 << 20, 1000, 0, 0, 0, 0])
    with pytest.raises(ValueError):
        FusedMLPEngine(32, 64, 32, device="cpu", clip_norm=-1.0)
