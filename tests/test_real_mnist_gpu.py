"""Real MNIST files and ``Normalize`` on the resident path -- on the GPU.

The kernels' u8 -> bf16 conversion is ``bf16(fmaf(u8, x_scale, x_shift))``
(``ops.fused_mlp.input_affine``): every place that gathers a batch (PRIME, the head's gather
workgroups, the one-launch step's tile waves, the loader-free ``mlp_eval``) is checked
bitwise against that formula, the identity map against the kernels without the argument, the
gradients against the bf16 emulation and fp32 autograd on the normalised pixels, and the
Trainer is shown to keep an IDX dataset with a ``Normalize`` on the resident path.
"""
import json
import os
import struct

import pytest
import torch
import torch.nn.functional as F

from ray_lightning_accelerators_amd.ops import fused_mlp, require
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices
from helpers import update_worst

gpu = pytest.mark.gpu

MNIST_NORM = (0.1307, 0.3081)
_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
# tests/test_mlp3.py GRAD_BOUND: measured on un-normalised data
GRAD_BOUND = {"W1": 0.1, "b1": 0.15, "W2": 0.12, "b2": 0.12, "W3": 0.015, "b3": 0.015}
_STATE = ("params", "exp_avg", "exp_avg_sq", "shadow", "h1pre", "xring", "yring", "counters")


def _dev():
    return torch.device("cuda", 0)


def _rel(a, b):
    return (a.float() - b.float()).norm().item() / max(b.float().norm().item(), 1e-12)


def _bf(x):
    return x.to(torch.bfloat16).float()


def _ramp(B):
    """3B + B/2 rows, pixel (i * 784 + j) mod 256: every byte value occurs in every batch."""
    n = 3 * B + B // 2
    x = (torch.arange(n * 784) % 256).to(torch.uint8).view(n, 784)
    return x, (torch.arange(n) * 7 + 3) % 10


def _normed(x_u8, norm):
    """fp32 FMA semantics of the kernels' pixel map (they round this value to bf16)."""
    return fused_mlp.u8_to_input(x_u8, *fused_mlp.input_affine(norm))


def _engine(route, L1, L2, B, norm, x, y, captured=None, **kw):
    """one: the one-launch step; two: head + fused tail; split: head / tail(grad) / allreduce /
    tail(adam) at world size 2 with a doubling stub allreduce (two identical ranks)."""
    if route == "split":
        def allreduce(g):
            if captured is not None:
                captured.append(g.detach().cpu().clone())
            g.mul_(2)

        eng = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), world_size=2, rank=0, allreduce=allreduce, **kw)
    else:
        eng = FusedMLPEngine(L1, L2, B, lr=1e-2, device=_dev(), **kw)
        if route == "two":
            eng.one_launch = False
        assert eng.one_launch == (route == "one")
    eng.set_data(x, y, normalize=norm)
    return eng


ROUTES = [("one", 32), ("one", 20), ("two", 48), ("split", 48)]


# ------------------------------------------------------------------ 1: gather exactness
def _pending_rows(eng):
    """(pixels [Bp, 784] bf16, labels [Bp]) of the pending batch's ring slot."""
    Bp = (eng.B + 31) // 32 * 32
    slot = int(eng.counters[3])
    xr = eng.xring.view(2, 49, Bp, 16)[slot].permute(1, 0, 2).reshape(Bp, 784).cpu()
    return xr, eng.yring.view(2, Bp)[slot].cpu()


def _assert_gather(eng, x, y, norm, world, what):
    B = eng.B
    cur = eng.step_in_epoch
    idx = shard_indices(x.size(0), world, 0, eng.epoch, eng.seed, True)[cur * B:(cur + 1) * B]
    xr, yr = _pending_rows(eng)
    want = _normed(x[idx], norm).to(torch.bfloat16)
    bad = int((xr[:B].view(torch.int16) != want.view(torch.int16)).sum())
    assert bad == 0, (what, bad, xr[:B].float().flatten()[:4], want.float().flatten()[:4])
    assert bool((xr[B:].view(torch.int16) == 0).all()), what  # padded rows stay zero, not x_shift
    assert torch.equal(yr[:B].long(), y[idx]) and bool((yr[B:] == -1).all()), what


@gpu
@pytest.mark.parametrize("route,B", ROUTES)
def test_gather_is_bitwise_the_fma_formula(route, B):
    """After prime(), and again after a step, the pending batch's xring slot is
    bf16(fmaf(u8, x_scale, x_shift)) and yring its labels; padded rows 0 / -1."""
    x, y = _ramp(B)
    eng = _engine(route, 32, 64, B, MNIST_NORM, x, y)
    world = 2 if route == "split" else 1
    eng.prime()
    torch.cuda.synchronize()
    _assert_gather(eng, x, y, MNIST_NORM, world, "prime")
    for s in range(2):
        eng.step()
        torch.cuda.synchronize()
        _assert_gather(eng, x, y, MNIST_NORM, world, f"step {s}")
    eng.check()
    # the slot holds values no un-normalised batch can: below zero and above one
    xr, _ = _pending_rows(eng)
    assert float(xr.float().min()) < -0.4 and float(xr.float().max()) > 2.8


# ------------------------------------------------------------------ 2: identity
@gpu
@pytest.mark.parametrize("route,B", ROUTES)
def test_identity_normalize_is_bitwise_the_default(route, B):
    """``normalize=(0, 1)`` against ``None``: every state buffer bitwise equal.  ``input_affine``
    maps (0, 1) onto exactly the default pair, so both engines launch the default (constant
    1/255) instances: this pins the plumbing, not a NORM instance.  That the default instances
    compute what they did rests on the existing suite and the instruction-stream comparison
    with the parent (profiles/r17_real_mnist/resources.txt); the NORM instances are held to the
    formula bitwise by test_gather_is_bitwise_the_fma_formula and the tests below, and the
    last lines here run one a single ulp away from the identity."""
    x, y = _ramp(B)
    a = _engine(route, 32, 64, B, None, x, y)
    b = _engine(route, 32, 64, B, (0.0, 1.0), x, y)
    steps = 2 * a.n_batches + 2
    for _ in range(steps):
        a.step()
        b.step()
    torch.cuda.synchronize()
    a.check()
    b.check()
    assert int(a.counters[0]) == steps
    for k in _STATE:
        ta, tb = getattr(a, k), getattr(b, k)
        same = torch.equal(ta.view(torch.int16), tb.view(torch.int16)) if ta.dtype == torch.bfloat16 \
            else torch.equal(ta, tb)
        assert same, (route, k)
    n = x.size(0)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(_dev())
    pa, pb = (torch.empty((n + 31) // 32, 2, device=_dev()) for _ in range(2))
    fused_mlp.mlp_eval(a.params, L1=32, L2=64, B=n, labels=a.labels, out=pa, x_u8=a.x_u8, index=idx)
    fused_mlp.mlp_eval(a.params, L1=32, L2=64, B=n, labels=a.labels, out=pb, x_u8=a.x_u8, index=idx,
                       x_scale=b.x_scale, x_shift=b.x_shift)
    assert torch.equal(pa, pb)
    # a NORM instance next to the identity (x_scale one ulp up), against the fp32 forward on
    # its own formula, to tests/test_fused_validation.py's tolerance
    up = float(torch.nextafter(torch.tensor(b.x_scale, dtype=torch.float32), torch.tensor(1.0)))
    assert up != b.x_scale
    p0 = fused_mlp.init_mlp_params(32, 64, torch.Generator().manual_seed(0))
    pc = torch.empty_like(pa)
    fused_mlp.mlp_eval(p0.to(_dev()), L1=32, L2=64, B=n, labels=a.labels, out=pc, x_u8=a.x_u8, index=idx,
                       x_scale=up, x_shift=0.0)
    ref = torch.zeros(2)
    fused_mlp.mlp_eval(p0, L1=32, L2=64, B=n, labels=y, out=ref, x_u8=x, index=idx.cpu(), x_scale=up, x_shift=0.0)
    got = pc.sum(0).cpu()
    assert abs(float(got[0] - ref[0])) / n < 2e-2 and abs(float(got[1] - ref[1])) <= max(2, 0.01 * n), (got, ref)


# ------------------------------------------------------------------ 3: bf16 emulation
def _fixed_h1pre(X, W1b):
    """X . W1^T as the kernels sum it: 49 16-pixel tile partials, each rounded to the 12.20
    fixed point (saturating at +-32), added exactly (tests/test_mlp3.py)."""
    xt = X.double().view(X.size(0), 49, 16)
    wt = W1b.double().view(W1b.size(0), 49, 16)
    part = torch.einsum("bti,mti->tbm", xt, wt).float().double()
    q = torch.round(part * 2.0 ** 20).clamp(-(2.0 ** 25), 2.0 ** 25)
    return (q.sum(0) / 2.0 ** 20).float()


def _emulate_bf16_grads(params, x, y, L1, L2, B):
    p = fused_mlp.mlp_unpack(params.cpu(), L1, L2)
    W1, b1, W2, b2, W3, b3 = [p[k] for k in p]
    X = _bf(x)
    h1 = _bf(torch.relu(_fixed_h1pre(X, _bf(W1)) + b1))
    h2 = _bf(torch.relu(h1 @ _bf(W2).T + b2))
    z = h2 @ _bf(W3).T + b3
    pr = torch.softmax(z, 1)
    dz = _bf((pr - F.one_hot(y, 10).float()) / B)
    dh2 = _bf((dz @ _bf(W3)) * (h2 > 0))
    dh1 = _bf((dh2 @ _bf(W2)) * (h1 > 0))
    g = [dh1.T @ X, dh1.sum(0), dh2.T @ h1, dh2.sum(0), dz.T @ h2, dz.sum(0)]
    return torch.cat([t.reshape(-1) for t in g])


@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (64, 128, 64)])
def test_normalized_grads_vs_bf16_emulation(L1, L2, B):
    """Every step of 2+ epochs: the gradient handed to the allreduce is the bf16 emulation fed
    the normalised batch, relative error < 2e-2 (the project's bound for this comparison)."""
    n_data = 3 * B + B // 2
    g = torch.Generator().manual_seed(L1 + L2 + B)
    x = torch.randint(0, 256, (n_data, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n_data,), generator=g)
    captured = []
    eng = _engine("split", L1, L2, B, MNIST_NORM, x, y, captured=captured)
    steps = 2 * eng.n_batches + 2
    worst = 0.0
    for s in range(steps):
        epoch, cur = eng.epoch, eng.step_in_epoch
        p_before = eng.params.detach().cpu().clone()
        eng.step()
        torch.cuda.synchronize()
        idx = shard_indices(n_data, 2, 0, epoch, 0, True)[cur * B:(cur + 1) * B]
        emu = _emulate_bf16_grads(p_before, _normed(x[idx], MNIST_NORM), y[idx], L1, L2, B)
        err = _rel(captured[-1][: emu.numel()], emu)
        worst = max(worst, err)
        assert err < 2e-2, (s, err)
    print(f"normalised grads vs emulation {L1}/{L2}/{B}: max rel err {worst:.3g} over {steps} steps")
    assert int(eng.counters[0]) == steps


# ------------------------------------------------------------------ 4: fp32 autograd
def _grads_of(flat, x, y, L1, L2, dev=None, autocast=False):
    p = {k: v.detach().clone().to(dev or "cpu").requires_grad_(True) for k, v in
         zip(_NAMES, fused_mlp.mlp_unpack(flat.detach().float().cpu(), L1, L2).values())}
    x, y = x.to(dev or "cpu"), y.to(dev or "cpu")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        h = torch.relu(F.linear(x, p["W1"], p["b1"]))
        h = torch.relu(F.linear(h, p["W2"], p["b2"]))
        z = F.linear(h, p["W3"], p["b3"])
    F.nll_loss(torch.log_softmax(z.float(), 1), y).backward()
    return torch.cat([p[k].grad.reshape(-1) for k in _NAMES]).cpu()


def _per_tensor_rel(g, ref, L1, L2):
    a, b = fused_mlp.mlp_unpack(g.cpu(), L1, L2), fused_mlp.mlp_unpack(ref.cpu(), L1, L2)
    return {k: _rel(u, v) for k, u, v in zip(_NAMES, a.values(), b.values())}


@gpu
def test_one_launch_normalized_grads_vs_fp32_autograd():
    """The one-launch step on Normalize((0.1307,), (0.3081,)) data against fp32 autograd on the
    normalised pixels, every step of 2+ epochs: per tensor below 1.5 x stock bf16 autocast's
    own error on the same batches + 0.01, below the absolute ceilings of the un-normalised
    test, and no saturated or non-finite layer-1 partial.

    Measured on an MI355X (53 steps, max normwise relative error, kernel / stock autocast):
    W1 0.0866 / 0.0867, b1 0.0650 / 0.0642, W2 0.0951 / 0.0986, b2 0.0849 / 0.0931,
    W3 0.0085 / 0.0097, b3 0.0097 / 0.0107; 0 saturated, 0 non-finite
    (profiles/r17_real_mnist/).  The ceilings measured on un-normalised data hold."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    L1, L2, B, nb = 32, 64, 32, 24
    x, y = synthetic_mnist(B * nb + 7, seed=11)
    eng = FusedMLPEngine(L1, L2, B, lr=1e-3, device=_dev(), seed=1)
    eng.set_data(x, y, normalize=MNIST_NORM)
    assert eng.one_launch
    b1 = eng.betas[0]
    worst = {k: 0.0 for k in _NAMES}
    worst_ac = {k: 0.0 for k in _NAMES}
    steps = 2 * nb + 5
    for _ in range(steps):
        epoch, cur = eng.epoch, eng.step_in_epoch
        idx = shard_indices(x.size(0), 1, 0, epoch, eng.seed, True)[cur * B:(cur + 1) * B]
        p0, m0 = eng.params.clone(), eng.exp_avg.clone()
        eng.step()
        g = (eng.exp_avg - b1 * m0) / (1 - b1)  # the gradient Adam applied
        xn = _normed(x[idx], MNIST_NORM)
        ref = _grads_of(p0, xn, y[idx], L1, L2)
        update_worst(worst, _per_tensor_rel(g, ref, L1, L2))
        update_worst(worst_ac, _per_tensor_rel(_grads_of(p0, xn, y[idx], L1, L2, _dev(), autocast=True), ref, L1, L2))
    eng.check()
    health = eng.health()
    row = {"test": "one_launch_normalized_grads_32_64", "steps": steps, "normalize": MNIST_NORM,
           "max_rel_err": worst, "stock_bf16_autocast_max_rel_err": worst_ac,
           "saturated": health["saturated"], "nonfinite": health["nonfinite"]}
    print("FIDELITY " + json.dumps(row), flush=True)
    if os.environ.get("RLA_FIDELITY_LOG"):
        with open(os.environ["RLA_FIDELITY_LOG"], "a") as f:
            f.write(json.dumps(row) + "\n")
    for k in _NAMES:
        assert worst[k] < 1.5 * worst_ac[k] + 0.01, (k, worst, worst_ac)
        assert worst[k] < GRAD_BOUND[k], (k, worst)
    assert health["saturated"] == 0 and health["nonfinite"] == 0 and not health["timed_out"], health


# ------------------------------------------------------------------ 5: eval
@gpu
@pytest.mark.parametrize("n", [96, 77])
@pytest.mark.parametrize("norm", [MNIST_NORM, (0.5, 0.5)])
def test_eval_kernel_normalized_vs_fp32_forward(norm, n):
    """``mlp_eval`` with x_scale / x_shift over 96 samples (3 chunks), and over 77 (a short last
    chunk: its padded rows are staged as zeros, not x_shift, and count for nothing), against an
    fp32 torch forward on the normalised pixels, to tests/test_fused_validation.py's tolerance."""
    L1, L2 = 32, 64
    dev = _dev()
    g = torch.Generator().manual_seed(1)
    p = fused_mlp.init_mlp_params(L1, L2, g)
    x = torch.randint(0, 256, (n + 29, 784), dtype=torch.uint8, generator=g)
    y = torch.randint(0, 10, (n + 29,), generator=g)
    idx = torch.randperm(n + 29, generator=g)[:n]
    sc, sh = fused_mlp.input_affine(norm)
    v = fused_mlp.mlp_unpack(p, L1, L2)
    h = torch.relu(F.linear(_normed(x[idx], norm), v["layer_1.weight"], v["layer_1.bias"]))
    h = torch.relu(F.linear(h, v["layer_2.weight"], v["layer_2.bias"]))
    logp = F.log_softmax(F.linear(h, v["layer_3.weight"], v["layer_3.bias"]), 1)
    ref = torch.stack([F.nll_loss(logp, y[idx], reduction="sum"), (logp.argmax(1) == y[idx]).sum().float()])
    part = torch.empty(3, 2, device=dev)
    kw = dict(L1=L1, L2=L2, B=n, labels=y.to(dev), x_u8=x.to(dev), index=idx.to(dev), x_scale=sc, x_shift=sh)
    fused_mlp.mlp_eval(p.to(dev), out=part, **kw)
    got = part.sum(0).cpu()
    print(f"eval {norm}: mean NLL {float(got[0]) / n:.5f} vs {float(ref[0]) / n:.5f}, correct {got[1]} vs {ref[1]}")
    assert abs(float(got[0] - ref[0])) / n < 2e-2, (got, ref)
    assert abs(float(got[1] - ref[1])) <= max(2, 0.01 * n), (got, ref)
    # the CPU reference of the same call agrees with the plain forward too
    cpu = torch.zeros(2)
    fused_mlp.mlp_eval(p, L1=L1, L2=L2, B=n, labels=y, out=cpu, x_u8=x, index=idx, x_scale=sc, x_shift=sh)
    assert abs(float(cpu[0] - ref[0])) / n < 2e-2 and abs(float(cpu[1] - ref[1])) <= 2
    # and the un-normalised launch computes something else
    plain = torch.empty(3, 2, device=dev)
    fused_mlp.mlp_eval(p.to(dev), out=plain, **{**kw, "x_scale": fused_mlp.X_SCALE_DEFAULT, "x_shift": 0.0})
    assert not torch.equal(plain, part)
    # accumulate mode and log-probabilities take the same map
    acc = torch.zeros(2, device=dev)
    lp = torch.empty(n, 10, device=dev)
    fused_mlp.mlp_eval(p.to(dev), out=acc, logits=lp, **kw)
    assert abs(float(acc[0].cpu() - got[0])) < 1e-2 and float(acc[1]) == float(got[1])
    assert float((lp.cpu() - logp).abs().max()) < 0.15
    # per chunk: the short last chunk sums its real rows only
    nll = F.nll_loss(logp, y[idx], reduction="none")
    for c in range(3):
        rows = nll[32 * c:32 * (c + 1)]
        assert abs(float(part[c, 0].cpu() - rows.sum())) < 2e-2 * rows.numel(), (c, part, rows.sum())


# ------------------------------------------------------------------ 5b: the one-workgroup step, u8 mode
@gpu
@pytest.mark.parametrize("L1,L2,B", [(32, 64, 32), (32, 64, 48), (128, 256, 20)])
def test_train_step_u8_mode_normalized(L1, L2, B):
    """``mlp_train_step`` over a resident dataset (rows of 32 and, where LDS allows, 64 per
    chunk): gradients, loss and cursor under a Normalize against the bf16 emulation of the
    normalised batch (plain fp32 layer-1 sum: this kernel has no fixed point), relative error
    < 2e-2; the identity map leaves every output bitwise what the default gives."""
    dev = _dev()
    g = torch.Generator().manual_seed(B)
    n = 3 * B
    x = torch.randint(0, 256, (n, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (n,), generator=g)
    order = torch.randperm(n, generator=g)
    p = fused_mlp.init_mlp_params(L1, L2, g)

    def run(**aff):
        grads = torch.zeros_like(p, device=dev)
        cnt = torch.tensor([0, 1], dtype=torch.int64, device=dev)  # the second batch
        stats = torch.zeros(4, 4, device=dev)
        fused_mlp.mlp_train_step(p.to(dev), grads, L1=L1, L2=L2, B=B, labels=y.to(dev), x_u8=x.to(dev),
                                 order=order.to(dev), counters=cnt, n_batches=3, stats=stats, **aff)
        torch.cuda.synchronize()
        return grads.cpu(), cnt.cpu(), stats.cpu()

    sc, sh = fused_mlp.input_affine(MNIST_NORM)
    grads, cnt, stats = run(x_scale=sc, x_shift=sh)
    idx = order[B:2 * B]
    xn = _bf(_normed(x[idx], MNIST_NORM))
    v = fused_mlp.mlp_unpack(p, L1, L2)
    W1, b1, W2, b2, W3, b3 = [v[k] for k in v]
    h1 = _bf(torch.relu(xn @ _bf(W1).T + b1))
    h2 = _bf(torch.relu(h1 @ _bf(W2).T + b2))
    z = h2 @ _bf(W3).T + b3
    dz = _bf((torch.softmax(z, 1) - F.one_hot(y[idx], 10).float()) / B)
    dh2 = _bf((dz @ _bf(W3)) * (h2 > 0))
    dh1 = _bf((dh2 @ _bf(W2)) * (h1 > 0))
    emu = torch.cat([t.reshape(-1) for t in (dh1.T @ xn, dh1.sum(0), dh2.T @ h1, dh2.sum(0), dz.T @ h2, dz.sum(0))])
    err = _rel(grads, emu)
    loss = float(F.nll_loss(torch.log_softmax(z, 1), y[idx]))
    print(f"u8 train step {L1}/{L2}/{B}: grad rel err {err:.3g}, loss {float(stats[0, 0]):.5f} vs {loss:.5f}")
    assert err < 2e-2, err
    assert abs(float(stats[0, 0]) - loss) < 2e-2 * max(1.0, loss) and int(stats[0, 2]) == B
    assert cnt.tolist() == [1, 2]
    base, ident = run(), run(**dict(zip(("x_scale", "x_shift"), fused_mlp.input_affine((0.0, 1.0)))))
    for a, b in zip(base, ident):
        assert torch.equal(a, b)
    assert not torch.equal(base[0], grads)


# ------------------------------------------------------------------ 6: bindings
BAD_MAPS = [(float("nan"), 0.0), (float("inf"), 0.0), (0.0, 0.0), (-1.0 / 255.0, 0.0), (1.0 / 255.0, float("nan")),
            (1.0 / 255.0, float("inf")), (1.0 / 255.0, float("-inf"))]


def _raw_mlp3(kind, kw, stats, **extra):
    """``_C.mlp3`` without ops.fused_mlp.mlp3_launch's own argument checks."""
    b = kw["betas"]
    args = [int(kind), kw["x_u8"], kw["labels"], kw["order"], kw["counters"], kw["n_batches"], kw["B"], kw["L1"],
            kw["L2"], kw["params"], kw["grads"], kw["exp_avg"], kw["exp_avg_sq"], kw["shadow"], kw["dh1t"],
            kw["xring"], kw["h1pre"], kw["act"], kw["yring"], stats, True, kw["lr"], b[0], b[1], kw["eps"],
            kw["weight_decay"], 1.0, kw["lr_tensor"], False, None, [], kw["head_part"], kw["hand"], -1, False, 1]
    require().mlp3(*args, **extra)


@gpu
def test_bad_pixel_map_is_refused_before_any_launch():
    dev = _dev()
    x, y = _ramp(32)
    eng = _engine("one", 32, 64, 32, MNIST_NORM, x, y)
    eng.run(2)
    torch.cuda.synchronize()
    names = _STATE + ("hand", "grads", "stats", "dh1t", "act")
    before = {k: getattr(eng, k).clone() for k in names}
    kw = eng._kw3()
    kinds = (fused_mlp.MLP3_STEP, fused_mlp.MLP3_HEAD, fused_mlp.MLP3_TAIL_GRAD, fused_mlp.MLP3_TAIL_ADAM,
             fused_mlp.MLP3_PRIME, fused_mlp.MLP3_STEP1, fused_mlp.MLP3_TAIL_ACC)
    for sc, sh in BAD_MAPS:
        for kind in kinds:
            with pytest.raises(ValueError, match="x_scale"):  # the Python wrapper
                fused_mlp.mlp3_launch(kind, stats=eng.stats, **{**kw, "x_scale": sc, "x_shift": sh})
            with pytest.raises(ValueError, match="nothing was launched"):  # launch_mlp3's code, via the binding
                _raw_mlp3(kind, kw, eng.stats, x_scale=sc, x_shift=sh)
    torch.cuda.synchronize()
    for k, v in before.items():  # counters, hand (acknowledgements, sequence) and every buffer: nothing ran
        t = getattr(eng, k)
        bits = (lambda u: u.view(torch.int16)) if t.dtype == torch.bfloat16 else (lambda u: u)
        assert torch.equal(bits(t), bits(v)), k
    # the one-launch step with an exchange has no Normalize instance: the wrapper says so, and
    # launch_mlp3 answers -14 before it looks at the exchange context (never a launch)
    good = dict(zip(("x_scale", "x_shift"), fused_mlp.input_affine(MNIST_NORM)))
    with pytest.raises(ValueError, match="MLP3_STEP1_DP"):
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1_DP, stats=eng.stats, **{**kw, **good})
    b = kw["betas"]
    dp_args = [int(fused_mlp.MLP3_STEP1_DP), kw["x_u8"], kw["labels"], kw["order"], kw["counters"], kw["n_batches"],
               kw["B"], kw["L1"], kw["L2"], kw["params"], kw["grads"], kw["exp_avg"], kw["exp_avg_sq"], kw["shadow"],
               kw["dh1t"], kw["xring"], kw["h1pre"], kw["act"], kw["yring"], eng.stats, True, kw["lr"], b[0], b[1],
               kw["eps"], kw["weight_decay"], 0.5, kw["lr_tensor"], False, None, [2, 0, 1 << 20, 1000, 0, 0, 0, 0],
               kw["head_part"], kw["hand"], 1, False, 1]
    with pytest.raises(RuntimeError, match="code -14"):
        require().mlp3(*dp_args, **good)
    torch.cuda.synchronize()
    for k, v in before.items():
        t = getattr(eng, k)
        bits = (lambda u: u.view(torch.int16)) if t.dtype == torch.bfloat16 else (lambda u: u)
        assert torch.equal(bits(t), bits(v)), k
    # mlp_eval and the loader-free train step: sentinels stay
    p = eng.params
    idx = torch.arange(32, device=dev)
    C = require()
    for sc, sh in BAD_MAPS:
        out = torch.full((1, 2), -7.0, device=dev)
        with pytest.raises(ValueError, match="nothing was launched"):
            C.mlp_eval(eng.x_u8, None, eng.labels, idx, 32, 32, 64, p, None, out, sc, sh)
        with pytest.raises(ValueError):
            fused_mlp.mlp_eval(p, L1=32, L2=64, B=32, labels=eng.labels, out=out, x_u8=eng.x_u8, index=idx,
                               x_scale=sc, x_shift=sh)
        grads = torch.full_like(p, -7.0)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        with pytest.raises(ValueError, match="nothing was launched"):
            C.mlp_train_step(eng.x_u8, None, eng.labels, idx, cnt, 1, 32, 32, 64, p, grads, None, None, None, False,
                             False, True, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, False, None, sc, sh)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((grads == -7.0).all()) and cnt.tolist() == [0, 0]
    assert torch.equal(eng.params, before["params"])
    # the x_f32 modes ignore the pair
    xf = torch.rand(32, 784, device=dev)
    out = torch.zeros(2, device=dev)
    C.mlp_eval(None, xf, eng.labels[:32].contiguous(), None, 32, 32, 64, p, None, out, float("nan"), float("nan"))
    torch.cuda.synchronize()
    assert float(out[0]) > 0.0
    # the engine goes on from where it was
    eng.run(2)
    torch.cuda.synchronize()
    eng.check()


# ------------------------------------------------------------------ 7: Trainer
def _idx_bytes(t: torch.Tensor) -> bytes:
    return struct.pack(">I", 0x00000800 | t.dim()) + b"".join(struct.pack(">I", d) for d in t.shape) + \
        t.to(torch.uint8).contiguous().numpy().tobytes()


def _write_idx_mnist(root, n_train=256, n_val=64):
    """``n_train + n_val`` synthetic rows as MNIST's train files (torchvision's layout); the
    caller splits them.  Returns (images [n, 784] uint8, labels)."""
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    x, y = synthetic_mnist(n_train + n_val, seed=21)
    raw = root / "MNIST" / "raw"
    raw.mkdir(parents=True)
    (raw / "train-images-idx3-ubyte").write_bytes(_idx_bytes(x.view(-1, 28, 28)))
    (raw / "train-labels-idx1-ubyte").write_bytes(_idx_bytes(y))
    return x, y


def _fit_resident(tmp_path, monkeypatch, model, datamodule=None):
    """``Trainer.fit`` for 2 epochs with every route off the resident path instrumented."""
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    seen = {"x_f32": 0, "eval": 0, "eval_none": 0}
    orig_step, orig_eval = fused_mlp.mlp_train_step, FusedMNISTStep.eval_epoch

    def train_step(*a, **k):
        seen["x_f32"] += k.get("x_f32") is not None
        return orig_step(*a, **k)

    def eval_epoch(self, dl, n):
        res = orig_eval(self, dl, n)
        seen["eval"] += 1
        seen["eval_none"] += res is None
        return res

    monkeypatch.setattr(fused_mlp, "mlp_train_step", train_step)
    monkeypatch.setattr(FusedMNISTStep, "eval_epoch", eval_epoch)
    trainer = pl.Trainer(default_root_dir=str(tmp_path / "run"), gpus=1, max_epochs=2, checkpoint_callback=False,
                         progress_bar_refresh_rate=0, num_sanity_val_steps=0)
    assert trainer.fit(model, datamodule=datamodule) == 1
    torch.cuda.synchronize()
    return trainer, seen


def _val_loss_fp32(model, x_u8, y, norm, B):
    """Mean over the full batches of the batch-mean NLL: the stock validation_epoch_end, as an
    fp32 forward of the trained weights on the normalised pixels."""
    with torch.no_grad():
        xn = _normed(x_u8, norm)
        w = [p.detach().cpu().float() for p in model.parameters()]
        h = torch.relu(F.linear(xn, w[0], w[1]))
        h = torch.relu(F.linear(h, w[2], w[3]))
        logp = F.log_softmax(F.linear(h, w[4], w[5]), 1)
        nb = x_u8.size(0) // B
        return float(F.nll_loss(logp[: nb * B], y[: nb * B]))


def _assert_resident(trainer, seen, batches, norm):
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    f = trainer._fused
    assert isinstance(f, FusedMNISTStep) and f.eng is not None
    assert f.eng.normalize == norm and (f.eng.x_scale, f.eng.x_shift) == fused_mlp.input_affine(norm)
    assert f.eng.one_launch
    assert f.eng.global_step == batches == int(f.eng.counters[0]) == trainer.global_step  # every batch was resident
    assert seen["x_f32"] == 0  # ... and none went through the loader-fed kernel
    assert seen["eval"] == 2 and seen["eval_none"] == 0  # both validation passes: one launch each
    h = f.health()
    assert h["saturated"] == 0 and h["nonfinite"] == 0, h


@gpu
def test_trainer_keeps_idx_mnist_with_normalize_resident(tmp_path, monkeypatch):
    import ray_lightning_accelerators_amd.lightning as pl
    from torch.utils.data import DataLoader, Subset
    from ray_lightning_accelerators_amd.models.data import Compose, IdxMNIST, Normalize
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    x, y = _write_idx_mnist(tmp_path)
    B = 32

    class RealMNIST(LightningMNISTClassifier):
        def prepare_data(self):
            if not hasattr(self, "_train_set"):
                full = IdxMNIST(self.data_dir, train=True, transform=Compose([Normalize((0.1307,), (0.3081,))]))
                self._train_set, self._val_set = Subset(full, range(256)), Subset(full, range(256, 320))

        def train_dataloader(self):
            self.prepare_data()
            return DataLoader(self._train_set, batch_size=self.batch_size, shuffle=True, drop_last=True)

        def val_dataloader(self):
            self.prepare_data()
            return DataLoader(self._val_set, batch_size=self.batch_size, drop_last=True)

    pl.seed_everything(0)
    model = RealMNIST({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": B}, data_dir=str(tmp_path))
    trainer, seen = _fit_resident(tmp_path, monkeypatch, model)
    _assert_resident(trainer, seen, 2 * (256 // B), MNIST_NORM)
    got = float(trainer.callback_metrics["ptl/val_loss"])
    want = _val_loss_fp32(model, x[256:], y[256:], MNIST_NORM, B)
    print(f"ptl/val_loss {got:.5f} vs fp32 forward {want:.5f}")
    assert abs(got - want) < 2e-2, (got, want)
    # what the loader hands out is what the kernels computed on: same pixels, same labels
    xb, yb = model._val_set[3]
    assert torch.equal(xb.reshape(-1).to(torch.bfloat16), _normed(x[259], MNIST_NORM).to(torch.bfloat16))
    assert yb == int(y[259])


@gpu
def test_trainer_keeps_the_datamodule_normalize_resident(tmp_path, monkeypatch):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.data import IdxMNIST
    from ray_lightning_accelerators_amd.models.datamodules import MNISTDataModule
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    x, y = _write_idx_mnist(tmp_path)
    B = 32
    pl.seed_everything(0)
    model = LightningMNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": B})
    dm = MNISTDataModule(data_dir=str(tmp_path), val_split=64, batch_size=B, normalize=True)
    trainer, seen = _fit_resident(tmp_path, monkeypatch, model, datamodule=dm)
    assert isinstance(dm._train.dataset, IdxMNIST)
    _assert_resident(trainer, seen, 2 * (256 // B), (0.5, 0.5))
    vi = torch.as_tensor(dm._val.indices)
    got = float(trainer.callback_metrics["ptl/val_loss"])
    want = _val_loss_fp32(model, x[vi], y[vi], (0.5, 0.5), B)
    print(f"ptl/val_loss {got:.5f} vs fp32 forward {want:.5f}")
    assert abs(got - want) < 2e-2, (got, want)
