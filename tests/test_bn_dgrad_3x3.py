"""bn1's backward sums from conv2's input-gradient epilogue (``RLA_FUSE_BN_DGRAD_3X3``):
the route through ops/conv.py, ops/bn.py and models/resnet.py.

A stride-1 bottleneck's conv2 is the only reader of bn1's output, so its 3x3 input
gradient masks with bn1's recomputed ReLU mask and sums for bn1's backward
(csrc/conv3x3.hip BWD); bn1 then runs only its finalize and apply.  The kernel itself is
checked in tests/test_conv3x3_bn_bwd.py; here the layers with the switch on (``1``)
against off (``0``), at the bounds of test_fused_bn_dgrad_resnet_layer_matches: output
bitwise equal, input gradient within 2e-2, every parameter gradient within 3e-2 (relative
L2; the masked gradient is bitwise the same, only the fp32 summation order of bn1's two
sums differs).
"""
import pytest
import torch
from torch import nn

gpu = pytest.mark.gpu


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


def _arena(module):
    from ray_lightning_accelerators_amd.parallel.arena import ParamArena

    arena = ParamArena(module)
    arena.enable_bf16_shadow(module)
    return arena


def _step(module, x0, loss=None):
    """One forward + backward under bf16 autocast: (y, dx, parameter gradients)."""
    module.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = module(x)
    (loss(out) if loss is not None else out.float().square().mean()).backward()
    y = out[0] if isinstance(out, tuple) else out
    return y.detach().float(), x.grad.float(), [p.grad.detach().float().clone() for p in module.parameters()]


def _close(on, off):
    (y1, g1, p1), (y0, g0, p0) = on, off
    assert torch.equal(y1, y0)
    assert _rel(g1, g0) < 2e-2, _rel(g1, g0)
    for a, b in zip(p1, p0):
        assert _rel(a, b) < 3e-2, _rel(a, b)


def _x(n, c, h, w, dev):
    return torch.randn(n, c, h, w, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@gpu
@pytest.mark.parametrize("defer", ["0", "1"])
def test_identity_bottleneck_matches_unfused(monkeypatch, defer):
    """Identity Bottleneck(256, 64): conv2's saved input is bn1's activation (RLA_BN_DEFER=0)
    or bn1's raw input (deferred apply, the PRE forward pinned); either way the fused input
    gradient reads bn1's input from the fold slot."""
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck
    from ray_lightning_accelerators_amd.ops import conv as C

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    monkeypatch.setenv("RLA_BN_DEFER", defer)
    if defer == "1":
        monkeypatch.setenv("RLA_CONV3X3_PRE", "pre")
    blk = Bottleneck(256, 64, fused_bn=True).to(dev).to(memory_format=torch.channels_last)
    arena = _arena(blk)  # noqa: F841 (keeps the bf16 shadow alive)
    assert blk.conv2.fuse_bn_dgrad
    x0 = _x(4, 256, 20, 20, dev)
    outs = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("RLA_FUSE_BN_DGRAD_3X3", fuse)
        n0, pre0 = C.stats["bn_dgrad_fused_3x3"], C.stats["pre_applied"]
        outs[fuse] = _step(blk, x0)
        assert C.stats["bn_dgrad_fused_3x3"] - n0 == (1 if fuse == "1" else 0)
        # conv2 took the deferred-apply forward in the second run only (conv3 defers in both)
        assert (C.stats["pre_applied"] - pre0 >= 2) == (defer == "1")
    _close(outs["1"], outs["0"])


@gpu
def test_downsample_bottleneck_is_untouched(monkeypatch):
    """A stride-2 conv2's input gradient is the library's: no fold route."""
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck
    from ray_lightning_accelerators_amd.ops import conv as C
    from ray_lightning_accelerators_amd.ops.bn import BatchNormAct2d
    from ray_lightning_accelerators_amd.ops.shadow import ConvBF16

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    monkeypatch.setenv("RLA_FUSE_BN_DGRAD_3X3", "1")
    down = nn.Sequential(ConvBF16(256, 512, 1, 2, bias=False), BatchNormAct2d(512, act=None))
    blk = Bottleneck(256, 128, 2, down, fused_bn=True).to(dev).to(memory_format=torch.channels_last)
    arena = _arena(blk)  # noqa: F841
    assert not getattr(blk.conv2, "fuse_bn_dgrad", False)
    n0 = C.stats["bn_dgrad_fused_3x3"]
    _, dx, _ = _step(blk, _x(4, 256, 16, 16, dev))
    assert C.stats["bn_dgrad_fused_3x3"] == n0
    assert bool(torch.isfinite(dx).all())


class _Tapped(nn.Module):
    """BatchNormAct2d -> ConvBF16 marked for the fusion, with a SECOND consumer of the
    BatchNorm output (a feature tap): autograd then hands the BatchNorm d + the tap's gradient."""

    def __init__(self):
        super().__init__()
        from ray_lightning_accelerators_amd.ops.bn import BatchNormAct2d
        from ray_lightning_accelerators_amd.ops.shadow import ConvBF16

        self.bn = BatchNormAct2d(64)
        self.conv = ConvBF16(64, 64, 3, 1, 1, bias=False)
        self.conv.fuse_bn_dgrad = True

    def forward(self, x):
        h = self.bn(x)
        return self.conv(h), h.float().mean()


@gpu
def test_second_consumer_is_rejected(monkeypatch):
    from ray_lightning_accelerators_amd.ops import bn as B
    from ray_lightning_accelerators_amd.ops import conv as C

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = _Tapped().to(dev).to(memory_format=torch.channels_last)
    with torch.no_grad():
        net.bn.bias.uniform_(-0.5, 0.5)
    arena = _arena(net)  # noqa: F841
    x0 = _x(4, 64, 20, 20, dev)
    outs = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("RLA_FUSE_BN_DGRAD_3X3", fuse)
        r0, n0 = B.fold_stats["fused_rejected"], C.stats["bn_dgrad_fused_3x3"]
        y, dx, ps = _step(net, x0, loss=lambda out: out[0].float().square().mean() + 10.0 * out[1])
        if fuse == "1":
            assert C.stats["bn_dgrad_fused_3x3"] - n0 == 1  # the conv cannot know ...
            assert B.fold_stats["fused_rejected"] - r0 == 1  # ... the BatchNorm notices
        else:
            assert B.fold_stats["fused_rejected"] == r0 and C.stats["bn_dgrad_fused_3x3"] == n0
        outs[fuse] = (dx, ps)
    (g1, p1), (g0, p0) = outs["1"], outs["0"]
    assert _rel(g1, g0) < 2e-2, _rel(g1, g0)
    for a, b in zip(p1, p0):
        assert _rel(a, b) < 3e-2, _rel(a, b)


@gpu
def test_single_consumer_hand_built_pair_fuses(monkeypatch):
    """The same pair without the tap: accepted, and equal to the switch-off run."""
    from ray_lightning_accelerators_amd.ops import bn as B
    from ray_lightning_accelerators_amd.ops import conv as C

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = _Tapped().to(dev).to(memory_format=torch.channels_last)
    arena = _arena(net)  # noqa: F841
    x0 = _x(3, 64, 17, 19, dev)
    outs = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("RLA_FUSE_BN_DGRAD_3X3", fuse)
        r0, n0 = B.fold_stats["fused_rejected"], C.stats["bn_dgrad_fused_3x3"]
        y, dx, ps = _step(net, x0, loss=lambda out: out[0].float().square().mean())
        assert B.fold_stats["fused_rejected"] == r0
        assert C.stats["bn_dgrad_fused_3x3"] - n0 == (1 if fuse == "1" else 0)
        outs[fuse] = (y, dx, ps)
    _close(outs["1"], outs["0"])


@gpu
def test_resnet_layer1_counts(monkeypatch):
    """resnet50().layer1 over one step: the 1x1 route's counters are where they were (two
    identity blocks' conv1, no extra fold), and all three conv2 take the new route."""
    from ray_lightning_accelerators_amd.models.resnet import resnet50
    from ray_lightning_accelerators_amd.ops import bn as B
    from ray_lightning_accelerators_amd.ops import conv as C

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    layer = resnet50(num_classes=10, fused_bn=True).to(dev).to(memory_format=torch.channels_last).layer1
    arena = _arena(layer)  # noqa: F841
    x0 = _x(4, 64, 32, 32, dev)
    folded = {}
    outs = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("RLA_FUSE_BN_DGRAD_3X3", fuse)
        n0, m0, f0 = C.stats["bn_dgrad_fused"], C.stats["bn_dgrad_fused_3x3"], B.fold_stats["folded"]
        outs[fuse] = _step(layer, x0)
        assert C.stats["bn_dgrad_fused"] - n0 == 2
        assert C.stats["bn_dgrad_fused_3x3"] - m0 == (3 if fuse == "1" else 0)
        folded[fuse] = B.fold_stats["folded"] - f0
    assert folded["1"] == folded["0"]
    _close(outs["1"], outs["0"])


@gpu
def test_deterministic_mode_takes_fused_untimed(monkeypatch):
    """Both candidates are fixed-order: deterministic mode (switch on auto) takes the fused
    kernel without timing -- ``_choice`` is unchanged -- and two backward passes are
    bitwise equal.  (conv2's deferred-apply forward is pinned: its ``fwd_kxk_pre`` table
    times ``pre`` against ``apply``, two bitwise-equal forwards, in deterministic mode too.)"""
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck
    from ray_lightning_accelerators_amd.ops import conv as C

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    monkeypatch.delenv("RLA_FUSE_BN_DGRAD_3X3", raising=False)
    monkeypatch.setenv("RLA_CONV3X3_PRE", "pre")
    blk = Bottleneck(256, 64, fused_bn=True).to(dev).to(memory_format=torch.channels_last)
    arena = _arena(blk)  # noqa: F841
    x0 = _x(4, 256, 20, 20, dev)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        before = dict(C._choice)
        n0 = C.stats["bn_dgrad_fused_3x3"]
        a = _step(blk, x0)
        b = _step(blk, x0)
        assert C._choice == before
        assert C.stats["bn_dgrad_fused_3x3"] - n0 == 2
    finally:
        torch.use_deterministic_algorithms(was)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for p, q in zip(a[2], b[2]):
        assert torch.equal(p, q)


@gpu
def test_auto_picks_from_its_own_table(monkeypatch):
    """``auto``: the pick comes from the ``dgrad_kxk_bn`` table (``fused`` / ``split``),
    consulted only for a layer with a fold; an answer that names no candidate (``_pick``
    during a graph capture) means ``split``."""
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck
    from ray_lightning_accelerators_amd.ops import conv as C

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    monkeypatch.delenv("RLA_FUSE_BN_DGRAD_3X3", raising=False)
    blk = Bottleneck(256, 64, fused_bn=True).to(dev).to(memory_format=torch.channels_last)
    arena = _arena(blk)  # noqa: F841
    x0 = _x(4, 256, 20, 20, dev)
    real = C._pick
    seen = {}
    answer = {"v": "fused"}

    def pick(op, key, cands):
        if op == "dgrad_kxk_bn":
            seen[op] = tuple(cands)
            for fn in cands.values():  # both candidates run (what the timing would do)
                fn()
            return answer["v"]
        seen.setdefault(op, tuple(cands))
        return real(op, key, cands)

    monkeypatch.setattr(C, "_pick", pick)
    outs = {}
    for v, count in (("fused", 1), ("split", 0), ("miopen", 0)):
        answer["v"] = v
        n0 = C.stats["bn_dgrad_fused_3x3"]
        outs[v] = _step(blk, x0)
        assert C.stats["bn_dgrad_fused_3x3"] - n0 == count
    assert seen["dgrad_kxk_bn"] == ("fused", "split")
    assert "dgrad_kxk" in seen  # split went on to the plain input gradient's own table
    _close(outs["fused"], outs["split"])
    _close(outs["miopen"], outs["split"])


# ------------------------------------------------------------------------------ CPU
def test_switch_changes_nothing_on_cpu(monkeypatch):
    from ray_lightning_accelerators_amd.models.resnet import Bottleneck
    from ray_lightning_accelerators_amd.ops import conv as C

    torch.manual_seed(0)
    blk = Bottleneck(64, 16, fused_bn=True)
    assert blk.conv2.fuse_bn_dgrad
    x0 = torch.randn(2, 64, 8, 8)
    outs = {}
    n0 = C.stats["bn_dgrad_fused_3x3"]
    for fuse in ("0", "1"):
        monkeypatch.setenv("RLA_FUSE_BN_DGRAD_3X3", fuse)
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = blk(x)
        y.square().mean().backward()
        outs[fuse] = (y.detach(), x.grad, [p.grad.clone() for p in blk.parameters()])
    assert torch.equal(outs["0"][0], outs["1"][0]) and torch.equal(outs["0"][1], outs["1"][1])
    for a, b in zip(outs["0"][2], outs["1"][2]):
        assert torch.equal(a, b)
    assert C.stats["bn_dgrad_fused_3x3"] == n0  # (0 in a process without a GPU)


def test_stats_key_and_mode_parsing(monkeypatch):
    from ray_lightning_accelerators_amd.ops import conv as C
    from ray_lightning_accelerators_amd.ops.bn import _FoldSlot

    assert isinstance(C.stats["bn_dgrad_fused_3x3"], int) and "bn_dgrad_fused" in C.stats
    if not torch.cuda.is_available():
        assert C.stats["bn_dgrad_fused_3x3"] == 0
    for raw, want in (("0", "0"), ("1", "1"), ("auto", "auto"), ("yes", "auto")):
        monkeypatch.setenv("RLA_FUSE_BN_DGRAD_3X3", raw)
        assert C.fuse_bn_dgrad_3x3_mode() == want
    monkeypatch.delenv("RLA_FUSE_BN_DGRAD_3X3")
    assert C.fuse_bn_dgrad_3x3_mode() == "auto"
    s = _FoldSlot()
    assert s.xin is None and s.st is None and s.x3 is None  # a hand-off of its own, not x3
