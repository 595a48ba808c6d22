"""Backend dispatch of the NHWC convolutions (ops/conv.py): every operation builds one
table of candidates, ``_pick`` names one and that table's callable runs.

CPU: the stock candidates (GEMM, ``aten::convolution``) equal ``F.conv2d``'s autograd
exactly, and exactly the picked candidate runs, once.  GPU: every candidate of every
table that has a MIOpen candidate, forced in turn, matches that MIOpen candidate.
"""
import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import conv as C

COUT = 24
SHAPES = [(2, 16, 5, 3), (2, 16, 6, 5)]
GEOS = [(3, 1, 1), (1, 2, 0), (3, 2, 1)]  # kernel, stride, padding


def _operands(shape, k, s=1, p=0, cout=COUT, device="cpu", seed=0):
    """x bf16 channels_last, the fp32 master weight, its bf16 copy and an output gradient."""
    g = torch.Generator().manual_seed(seed)
    n, cin, h, w = shape
    x = torch.randn(n, cin, h, w, generator=g).to(torch.bfloat16)
    wt = torch.randn(cout, cin, k, k, generator=g) / (k * cin ** 0.5)
    dy = torch.randn(n, cout, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, generator=g).to(torch.bfloat16)
    x, wt, dy = (t.to(device).contiguous(memory_format=torch.channels_last) for t in (x, wt, dy))
    return x, wt, wt.to(torch.bfloat16), dy


def _conv1x1(x, wt, dy, **kw):
    x, wt = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = C._Conv1x1Fn.apply(x, wt, None, kw.get("fork"), kw.get("bn_stats"), False)
    y.backward(dy)
    return y.detach(), x.grad, wt.grad


def _convkxk(x, wt, wb, dy, s, p, **kw):
    x, wt = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y = C._ConvNHWCFn.apply(x, wt, wb, (s, s), (p, p), kw.get("fork"), kw.get("bn_stats"))
    y.backward(dy)
    return y.detach(), x.grad, wt.grad


def _autograd(x, wb, dy, s, p):
    """``F.conv2d``'s autograd on the bf16 weight; the weight gradient widened to fp32."""
    x, wb = x.clone().requires_grad_(True), wb.clone().requires_grad_(True)
    y = F.conv2d(x, wb, stride=s, padding=p)
    y.backward(dy)
    return y.detach(), x.grad, wb.grad.float()


def _same(got, ref):
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a, b), float((a.float() - b.float()).abs().max())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["gemm", "miopen"])
def test_stock_1x1_backends_equal_autograd(monkeypatch, shape, mode):
    # (the GEMM weight gradient is aten::mm.dtype, which has no CPU kernel: GPU tests)
    monkeypatch.setenv("RLA_CONV1X1", mode)
    monkeypatch.setenv("RLA_CONV_WGRAD", "miopen")
    x, wt, wb, dy = _operands(shape, 1)
    _same(_conv1x1(x, wt, dy), _autograd(x, wb, dy, 1, 0))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k,s,p", GEOS)
def test_stock_kxk_backend_equals_autograd(monkeypatch, shape, k, s, p):
    monkeypatch.setenv("RLA_CONV1X1", "miopen")
    monkeypatch.setenv("RLA_CONV_WGRAD", "miopen")
    x, wt, wb, dy = _operands(shape, k, s, p)
    _same(_convkxk(x, wt, wb, dy, s, p), _autograd(x, wb, dy, s, p))


# (op, key, candidate names in insertion order) of one 1x1 and the three KxK layers per
# shape, as the same recorder gave them on the commit before the tables were unified
PICKS = [
    ("fwd", (30, 16, 24), ("gemm", "miopen")),
    ("dgrad", (30, 16, 24), ("gemm", "miopen")),
    ("wgrad", (30, 16, 24), ("gemm", "miopen")),
    ("wgrad_kxk", (30, 16, 24, 3, 3, 1, 1), ("miopen", "hip", "hip_gen")),
    ("wgrad_kxk", (12, 16, 24, 1, 1, 2, 0), ("miopen", "hip")),
    ("wgrad_kxk", (12, 16, 24, 3, 3, 2, 1), ("miopen", "hip")),
    ("fwd", (60, 16, 24), ("gemm", "miopen")),
    ("dgrad", (60, 16, 24), ("gemm", "miopen")),
    ("wgrad", (60, 16, 24), ("gemm", "miopen")),
    ("wgrad_kxk", (60, 16, 24, 3, 3, 1, 1), ("miopen", "hip", "hip_gen")),
    ("wgrad_kxk", (18, 16, 24, 1, 1, 2, 0), ("miopen", "hip")),
    ("wgrad_kxk", (18, 16, 24, 3, 3, 2, 1), ("miopen", "hip")),
]
LIBRARY_CALLS = ("_miopen_fwd", "_miopen_bwd", "_gemm_fwd", "_gemm_dgrad", "_gemm_wgrad")


def _count_library_calls(monkeypatch):
    calls = []
    for name in LIBRARY_CALLS:
        def counting(*a, _name=name, _real=getattr(C, name)):
            # a MIOpen backward is told apart by what it was asked for: (need_dx, need_dw)
            calls.append((_name,) + tuple(a[5:]) if _name == "_miopen_bwd" else _name)
            return _real(*a)

        monkeypatch.setattr(C, name, counting)
    return calls


@pytest.mark.parametrize("stock", ["gemm", "miopen"])
def test_picked_candidate_is_the_one_that_runs(monkeypatch, stock):
    """``_pick`` replaced by a recorder (so nothing is timed): per operation exactly one
    library call, the picked backend's; dgrad and wgrad both from MIOpen are ONE call."""
    want = {"fwd": stock, "dgrad": stock, "wgrad": "miopen", "wgrad_kxk": "miopen"}
    seen = []

    def pick(op, key, cands):
        seen.append((op, key, tuple(cands)))
        return want[op]

    monkeypatch.setattr(C, "_pick", pick)
    calls = _count_library_calls(monkeypatch)
    both = ("_miopen_bwd", True, True)
    ran_1x1 = {"gemm": ["_gemm_fwd", "_gemm_dgrad", ("_miopen_bwd", False, True)], "miopen": ["_miopen_fwd", both]}
    for shape in SHAPES:
        x, wt, wb, dy = _operands(shape, 1)
        del calls[:]
        got = _conv1x1(x, wt, dy)
        assert calls == ran_1x1[stock]
        _same(got, _autograd(x, wb, dy, 1, 0))
        for k, s, p in GEOS:
            x, wt, wb, dy = _operands(shape, k, s, p)
            del calls[:]
            got = _convkxk(x, wt, wb, dy, s, p)
            assert calls == ["_miopen_fwd", both]
            _same(got, _autograd(x, wb, dy, s, p))
    assert seen == PICKS


# ---- GPU: every candidate of every table with a MIOpen candidate, forced in turn ----

def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))


def _forked_pair(ops1, ops2, strided_last):
    """A bottleneck's conv1 (1x1) and its strided downsample conv reading the same x
    through one GradFork: (y1, y2, dx of both, dw1, dw2).  The layer applied last runs
    its backward first and parks its input gradient; the other adds into it."""
    (x, w1, _, dy1), (_, w2, wb2, dy2) = ops1, ops2
    x, w1, w2 = (t.clone().requires_grad_(True) for t in (x, w1, w2))
    fork = C.GradFork()
    y1 = y2 = None
    for strided in (not strided_last, strided_last):
        if strided:
            y2 = C._ConvNHWCFn.apply(x, w2, wb2, (2, 2), (0, 0), fork)
        else:
            y1 = C._Conv1x1Fn.apply(x, w1, None, fork, None, False)
    torch.autograd.backward([y1, y2], [dy1, dy2])
    assert fork.dx is None
    return y1.detach(), y2.detach(), x.grad, w1.grad, w2.grad


def _layer_1x1(stats):
    ops = _operands((4, 64, 8, 8), 1, cout=64, device="cuda")
    return lambda: _conv1x1(ops[0], ops[1], ops[3], bn_stats=C.BNStats() if stats else None)


def _layer_3x3(stats):
    ops = _operands((4, 64, 8, 8), 3, 1, 1, cout=64, device="cuda")
    return lambda: _convkxk(*ops, 1, 1, bn_stats=C.BNStats() if stats else None)


def _layer_strided():
    ops = _operands((4, 64, 8, 8), 1, 2, 0, cout=128, device="cuda")
    return lambda: _convkxk(*ops, 2, 0)


def _layer_forked(strided_last):
    ops1 = _operands((4, 64, 8, 8), 1, cout=64, device="cuda")
    ops2 = _operands((4, 64, 8, 8), 1, 2, 0, cout=128, device="cuda", seed=1)
    return lambda: _forked_pair(ops1, ops2, strided_last)


# layer -> its tables in pick order, and which results are input gradients (bound 2e-2;
# outputs and weight gradients 1e-2: the bounds of test_conv3x3.py / test_conv_wgrad.py)
LAYERS = {
    "1x1": (lambda: _layer_1x1(False), [("fwd", ("gemm", "miopen")), ("dgrad", ("gemm", "miopen")),
                                        ("wgrad", ("gemm", "miopen", "hip"))], (1,)),
    "1x1_stats": (lambda: _layer_1x1(True), [("fwd_st", ("hip", "gemm", "miopen")), ("dgrad", ("gemm", "miopen")),
                                             ("wgrad", ("gemm", "miopen", "hip"))], (1,)),
    "3x3": (lambda: _layer_3x3(False), [("fwd_kxk", ("miopen", "hip")), ("wgrad_kxk", ("miopen", "hip", "hip_gen")),
                                        ("dgrad_kxk", ("miopen", "hip"))], (1,)),
    "3x3_stats": (lambda: _layer_3x3(True), [("fwd_kxk_st", ("miopen", "hip_st")),
                                             ("wgrad_kxk", ("miopen", "hip", "hip_gen")),
                                             ("dgrad_kxk", ("miopen", "hip"))], (1,)),
    "strided_1x1": (_layer_strided, [("wgrad_kxk", ("miopen", "hip"))], (1,)),
    # the strided conv parks its gradient, the 1x1 adds in its GEMM (no dgrad table) ...
    "forked_strided_first": (lambda: _layer_forked(True), [("fwd", ("gemm", "miopen")),
                                                           ("wgrad", ("gemm", "miopen", "hip")),
                                                           ("wgrad_kxk", ("miopen", "hip"))], (2,)),
    # ... and the 1x1 parks, the strided conv adds into every second pixel
    "forked_1x1_first": (lambda: _layer_forked(False), [("fwd", ("gemm", "miopen")), ("dgrad", ("gemm", "miopen")),
                                                        ("wgrad", ("gemm", "miopen", "hip")),
                                                        ("wgrad_kxk", ("miopen", "hip"))], (2,)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("layer", list(LAYERS))
def test_every_candidate_matches_miopen(monkeypatch, layer):
    make, tables, dx_at = LAYERS[layer]
    run = make()
    want, seen = {}, {}

    def pick(op, key, cands):
        seen[op] = tuple(cands)
        return want.get(op, "miopen")

    monkeypatch.setattr(C, "_pick", pick)
    ref = run()
    assert seen == dict(tables)  # a new candidate or table must be forced here too
    for op, names in tables:
        for name in names:
            if name == "miopen":
                continue
            want.clear()
            want[op] = name
            for i, (a, b) in enumerate(zip(run(), ref)):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert _rel(a, b) < (2e-2 if i in dx_at else 1e-2), (op, name, i, _rel(a, b))
