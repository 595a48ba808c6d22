"""The flat-arena kernels of csrc/optim_kernels.hip (adam_step, sgd_step, multi_copy, scale_,
sumsq) and csrc/mlp_adam.hip's arena Adam, run through the paths production takes -- the
grid-stride loop beyond 2048 blocks, the bf16 shadow, device step / learning-rate scalars
under graph replay, fuse_optimizer's param groups, a prebuilt copy table -- and compared
elementwise with the float64 single-step references of tests/optim_reference.py (validated on
the CPU by tests/test_optim_reference.py).  Every bound is derived there.

Each case prints ``[ratio] <kernel> <case>: worst error / bound``; test_zz_worst_ratios prints
the worst per kernel."""
import functools

import pytest
import torch

import optim_reference as R

pytestmark = pytest.mark.gpu
WORST = {}
SENTINEL = 7.0
DEV = "cuda"


def _ops():
    from ray_lightning_accelerators_amd import ops

    ops.require()
    return ops


def _report(kernel, case, c):
    print(f"[ratio] {kernel} {case}: {c.detail}")
    WORST[kernel] = max(WORST.get(kernel, 0.0), c.ratio)
    assert c.ok, f"{kernel} {case}: {c.detail}"


def _adam_kw(cfg):
    return dict(lr=cfg.lr, betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.wd, grad_scale=cfg.grad_scale,
                adamw=cfg.adamw, maximize=cfg.maximize)


def _sgd_kw(cfg):
    return dict(lr=cfg.lr, momentum=cfg.momentum, dampening=cfg.dampening, weight_decay=cfg.wd,
                grad_scale=cfg.grad_scale, nesterov=cfg.nesterov, maximize=cfg.maximize)


@functools.lru_cache(maxsize=2)
def _case(kind, cfg, n):
    """(state, reference) of one case, computed once for the runs with and without a shadow."""
    st = R.make_state(n, 21 if kind == "adam" else 22, cfg.state)
    return st, (R.ref_adam if kind == "adam" else R.ref_sgd)(st, cfg)


def _device_scalars(t, lr):
    return (torch.tensor([t], dtype=torch.int64, device=DEV),
            torch.tensor([lr], dtype=torch.float32, device=DEV))


def _run_adam(st, cfg, shadow, t=None, lr=None, device_scalars=False):
    d = {k: st[k].to(DEV) for k in ("p", "g", "m", "v")}
    bf = torch.full((st["p"].numel(),), SENTINEL, dtype=torch.bfloat16, device=DEV) if shadow else None
    kw = _adam_kw(cfg)
    step = cfg.t if t is None else t
    if device_scalars:   # the host lr must be ignored
        step, kw["lr_tensor"] = _device_scalars(step, cfg.lr if lr is None else lr)
        kw["lr"] = 123.0
    _ops().fused_adam_(d["p"], d["g"], d["m"], d["v"], step=step, p_bf16=bf, **kw)
    torch.cuda.synchronize()
    assert torch.equal(d["g"].cpu(), st["g"]) or bool(torch.isnan(st["g"]).any())
    return {k: d[k].cpu() for k in ("p", "m", "v")}, (bf.cpu() if shadow else None)


def _run_sgd(st, cfg, shadow, t=None, lr=None, device_scalars=False):
    d = {k: st[k].to(DEV) for k in ("p", "g", "buf")}
    has_buf = cfg.momentum != 0
    bf = torch.full((st["p"].numel(),), SENTINEL, dtype=torch.bfloat16, device=DEV) if shadow else None
    kw = _sgd_kw(cfg)
    step = cfg.t if t is None else t
    if device_scalars:
        step, kw["lr_tensor"] = _device_scalars(step, cfg.lr if lr is None else lr)
        kw["lr"] = 123.0
    _ops().fused_sgd_(d["p"], d["g"], d["buf"] if has_buf else None, step=step, p_bf16=bf, **kw)
    torch.cuda.synchronize()
    out = {"p": d["p"].cpu()}
    if has_buf:
        out["buf"] = d["buf"].cpu()
    return out, (bf.cpu() if shadow else None)


# ------------------------------------------------------------------ adam_step / sgd_step
@pytest.mark.parametrize("shadow", [False, True], ids=["noshadow", "shadow"])
@pytest.mark.parametrize("case", R.ADAM_CASES, ids=lambda c: f"{c[0].name}-{c[1]}")
def test_adam_step(case, shadow):
    cfg, n = case
    st, ref = _case("adam", cfg, n)
    out, bf = _run_adam(st, cfg, shadow)
    _report("adam_step", f"{cfg.name} n={n} shadow={shadow}", R.check_adam(out, ref, bf))


@pytest.mark.parametrize("shadow", [False, True], ids=["noshadow", "shadow"])
@pytest.mark.parametrize("case", R.SGD_CASES, ids=lambda c: f"{c[0].name}-{c[1]}")
def test_sgd_step(case, shadow):
    cfg, n = case
    st, ref = _case("sgd", cfg, n)
    out, bf = _run_sgd(st, cfg, shadow)
    _report("sgd_step", f"{cfg.name} n={n} shadow={shadow}", R.check_sgd(out, ref, bf))


def test_sgd_first_step_overwrites_the_buffer():
    """t = 1 against t = 2 from the same nonzero buffer: only t = 2 blends it."""
    cfg = next(c for c in R.SGD_CONFIGS if c.name == "t1")
    st = R.make_state(1025, 22)
    for t in (1, 2):
        out, bf = _run_sgd(st, cfg, True, t=t)
        _report("sgd_step", f"t={t} from a nonzero buf", R.check_sgd(out, R.ref_sgd(st, cfg, t=t), bf))
        assert not R.check_sgd(out, R.ref_sgd(st, cfg, t=3 - t), bf).ok
    out, _ = _run_sgd(st, cfg, False, t=1)
    assert torch.equal(out["buf"], st["g"])   # grad_scale 1, no decay: the gradient itself


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_arena_views_leave_their_neighbours_alone(kind):
    """Operands as views whose storage offset is a multiple of 4 elements, as the arena hands
    them out (the shadow at 4 elements: 8-byte, not 16-byte aligned)."""
    n, lo = 1027, 8
    cfg = R.ADAM_CONFIGS[1] if kind == "adam" else R.SGD_CONFIGS[4]
    st = R.make_state(n, 33)
    keys = ("p", "g", "m", "v") if kind == "adam" else ("p", "g", "buf")
    base = {k: torch.full((n + 2 * lo,), SENTINEL, device=DEV) for k in keys}
    base["bf"] = torch.full((n + 8,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    view = {k: base[k][lo:lo + n] for k in keys}
    view["bf"] = base["bf"][4:4 + n]
    for k in keys:
        view[k].copy_(st[k])
    ops = _ops()
    if kind == "adam":
        ops.fused_adam_(view["p"], view["g"], view["m"], view["v"], step=cfg.t, p_bf16=view["bf"], **_adam_kw(cfg))
        c = R.check_adam({k: view[k].cpu() for k in ("p", "m", "v")}, R.ref_adam(st, cfg), view["bf"].cpu())
    else:
        ops.fused_sgd_(view["p"], view["g"], view["buf"], step=cfg.t, p_bf16=view["bf"], **_sgd_kw(cfg))
        c = R.check_sgd({k: view[k].cpu() for k in ("p", "buf")}, R.ref_sgd(st, cfg), view["bf"].cpu())
    torch.cuda.synchronize()
    _report(f"{kind}_step", f"views at offset {lo}, n={n}", c)
    for k in keys:
        assert bool((base[k][:lo] == SENTINEL).all()) and bool((base[k][lo + n:] == SENTINEL).all()), k
    assert bool((base["bf"][:4] == SENTINEL).all()) and bool((base["bf"][4 + n:] == SENTINEL).all())
    assert torch.equal(view["g"].cpu(), st["g"])


# ------------------------------------------------------------------ device scalars, graph replay
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_device_step_and_lr_override_the_host_arguments(kind):
    n = 1025
    st = R.make_state(n, 34)
    if kind == "adam":
        cfg = R.ADAM_CONFIGS[1]
        for t, lr in ((1, 2e-3), (9, 5e-4)):
            out, bf = _run_adam(st, cfg, True, t=t, lr=lr, device_scalars=True)
            ref = R.ref_adam(st, cfg, t=t, lr=lr)
            _report("adam_step", f"device scalars t={t} lr={lr}", R.check_adam(out, ref, bf))
    else:
        cfg = R.SGD_CONFIGS[4]
        for t, lr in ((1, 0.02), (2, 0.3)):
            out, bf = _run_sgd(st, cfg, True, t=t, lr=lr, device_scalars=True)
            _report("sgd_step", f"device scalars t={t} lr={lr}", R.check_sgd(out, R.ref_sgd(st, cfg, t=t, lr=lr), bf))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_graph_replay_reads_step_and_lr_at_run_time(kind):
    """One captured step (the counter's add_ then the kernel, a linear graph) replayed four
    times with a new gradient and learning rate each: every replay is one reference step from the
    state it found.  Replay 1 takes SGD's first-step branch, the others must not."""
    n = 4099
    ops = _ops()
    cfg = R.ADAM_CONFIGS[1] if kind == "adam" else R.SGD_CONFIGS[4]
    keys = ("p", "m", "v") if kind == "adam" else ("p", "buf")
    st0 = R.make_state(n, 35)
    d = {k: st0[k].to(DEV) for k in keys}
    g_static = torch.zeros(n, device=DEV)
    bf = torch.full((n,), SENTINEL, dtype=torch.bfloat16, device=DEV) if kind == "sgd" else None
    step_t, lr_t = _device_scalars(0, cfg.lr)

    def body():
        step_t.add_(1)
        if kind == "adam":
            kw = dict(_adam_kw(cfg), lr=123.0)
            ops.fused_adam_(d["p"], g_static, d["m"], d["v"], step=step_t, lr_tensor=lr_t, **kw)
        else:
            kw = dict(_sgd_kw(cfg), lr=123.0)
            ops.fused_sgd_(d["p"], g_static, d["buf"], step=step_t, lr_tensor=lr_t, p_bf16=bf, **kw)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in keys:                                # the warm-up moved the state: put it back
        d[k].copy_(st0[k])
    step_t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    torch.cuda.synchronize()
    assert int(step_t) == 0 and torch.equal(d["p"].cpu(), st0["p"])   # a capture runs nothing
    for i, lr in enumerate((0.05, 0.02, 0.3, 1e-3), 1):
        lr = lr * (0.1 if kind == "adam" else 1.0)
        pre = {k: d[k].cpu() for k in keys}
        pre["g"] = R.make_state(n, 36 + i)["g"]
        g_static.copy_(pre["g"])
        lr_t.fill_(lr)
        graph.replay()
        torch.cuda.synchronize()
        assert int(step_t) == i
        out = {k: d[k].cpu() for k in keys}
        if kind == "adam":
            c = R.check_adam(out, R.ref_adam(pre, cfg, t=i, lr=lr))
        else:
            c = R.check_sgd(out, R.ref_sgd(pre, cfg, t=i, lr=lr), bf.cpu())
            other = R.ref_sgd(pre, cfg, t=2 if i == 1 else 1, lr=lr)     # the other branch of `first`
            assert not R.check_sgd(out, other).ok
        _report(f"{kind}_step", f"graph replay {i} lr={lr:g}", c)


# ------------------------------------------------------------------ fuse_optimizer
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(7, 5)
        self.norm = torch.nn.LayerNorm(5)
        self.b = torch.nn.Linear(5, 3)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_fuse_optimizer_groups_against_the_reference(kind):
    """Two param groups whose boundary lies inside the arena (weights with decay, biases and norm
    parameters without), bf16 shadow, device scalars, grad_scale 0.5: three steps with the learning
    rate changed in between, each checked per group as one reference step from the state before it."""
    from ray_lightning_accelerators_amd.parallel.arena import ParamArena
    from ray_lightning_accelerators_amd.parallel.fused_optim import fuse_optimizer

    torch.manual_seed(3)
    mod = _Tiny().to(DEV)
    decay = [mod.a.weight, mod.b.weight]
    rest = [mod.a.bias, mod.norm.weight, mod.norm.bias, mod.b.bias]
    arena = ParamArena(mod, params=decay + rest)
    arena.enable_bf16_shadow()
    wds = (0.01, 0.0)
    groups = [{"params": decay, "weight_decay": wds[0]}, {"params": rest, "weight_decay": wds[1]}]
    if kind == "sgd":
        opt = torch.optim.SGD(groups, lr=0.05, momentum=0.9)
        cfgs = [R.sgd_cfg("group", momentum=0.9, wd=w, grad_scale=0.5) for w in wds]
    else:
        opt = torch.optim.Adam(groups, lr=3e-3)
        cfgs = [R.adam_cfg("group", wd=w, grad_scale=0.5) for w in wds]
    assert fuse_optimizer(opt, arena, grad_scale_fn=lambda: 0.5) is opt and opt._rla_fused
    opt.enable_device_scalars()
    gss = opt._rla_groups
    assert [(gs.start, gs.end) for gs in gss] == [(0, 52), (52, arena.numel)] and arena.numel == 80
    state_keys = ("m", "v") if kind == "adam" else ("buf",)
    names = {"m": "exp_avg", "v": "exp_avg_sq", "buf": "momentum_buffer"}
    for gs, grp in zip(gss, opt.param_groups):
        for q in grp["params"]:
            o, _ = arena.offsets[arena.index_of(q)]
            assert q.data_ptr() == arena.data.data_ptr() + 4 * o
            for k in state_keys:   # optimizer.state[p] views alias the arena-shaped buffers
                assert opt.state[q][names[k]].data_ptr() == getattr(gs, k).data_ptr() + 4 * (o - gs.start)
    for step, lr in enumerate((0.05, 0.02, 0.1) if kind == "sgd" else (3e-3, 1e-3, 5e-3), 1):
        for grp in opt.param_groups:
            grp["lr"] = lr
        g = 0.3 * torch.randn(arena.numel, generator=torch.Generator().manual_seed(40 + step))
        arena.grad.copy_(g)
        pre_p = arena.data.cpu()
        pre = [{k: getattr(gs, k).cpu() for k in state_keys} for gs in gss]
        opt.step()
        torch.cuda.synchronize()
        for gi, (gs, cfg) in enumerate(zip(gss, cfgs)):
            st = dict(pre[gi], p=pre_p[gs.start:gs.end], g=g[gs.start:gs.end])
            out = {k: getattr(gs, k).cpu() for k in state_keys}
            out["p"] = arena.data[gs.start:gs.end].cpu()
            bf = arena.bf16[gs.start:gs.end].cpu()
            if kind == "adam":
                c = R.check_adam(out, R.ref_adam(st, cfg, t=step, lr=lr), bf)
            else:
                c = R.check_sgd(out, R.ref_sgd(st, cfg, t=step, lr=lr), bf)
            _report(f"{kind}_step", f"fuse_optimizer group {gi} step {step} lr={lr:g}", c)
            assert int(gs.step_t) == step
        assert torch.equal(mod.b.weight.detach().cpu().reshape(-1), arena.data[36:51].cpu())


# ------------------------------------------------------------------ mlp_adam_(update=True)
@pytest.mark.parametrize("L", R.MLP_WIDTHS, ids=lambda L: f"{L[0]}x{L[1]}")
def test_mlp_adam_update(L):
    from ray_lightning_accelerators_amd.ops import fused_mlp

    L1, L2 = L
    cfg = R.MLP_CFG
    lay = fused_mlp.mlp_shadow_layout(L1, L2)
    st = R.make_state(lay["np"], 23 + L1 + L2)
    d = {k: st[k].to(DEV) for k in ("p", "g", "m", "v")}
    shadow = torch.full((lay["total"],), SENTINEL, dtype=torch.bfloat16, device=DEV)
    step_t, lr_t = _device_scalars(cfg.t, cfg.lr)
    fused_mlp.mlp_adam_(d["p"], d["g"], d["m"], d["v"], shadow, L1=L1, L2=L2, lr=123.0, step=step_t, betas=cfg.betas,
                        eps=cfg.eps, weight_decay=cfg.wd, grad_scale=cfg.grad_scale, adamw=cfg.adamw, lr_tensor=lr_t)
    torch.cuda.synchronize()
    sh = shadow.cpu()
    out = {k: d[k].cpu() for k in ("p", "m", "v")}
    out.update(np=sh[:lay["np"]], w2t=sh[lay["w2t"]:lay["w3t"]], w3t=sh[lay["w3t"]:lay["total"]])
    assert torch.equal(d["g"].cpu(), st["g"]) and int(step_t) == cfg.t
    _report("mlp_adam", f"{L1}x{L2} update", R.check_mlp_adam(out, R.ref_mlp_adam(st, cfg, L1, L2), L1, L2))


# ------------------------------------------------------------------ multi_copy
@pytest.mark.parametrize("scale", [0.25, 1.0 / 3.0], ids=["quarter", "third"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["copy", "accumulate"])
@pytest.mark.parametrize("sdt,ddt", R.COPY_DTYPE_PAIRS)
def test_multi_copy(sdt, ddt, accumulate, scale):
    """One table of five pairs (1, 16383, 16384, 16385, 40000 elements) at element offsets 0, 1, 3 of
    their storage; through ``pairs``, then through a prebuilt table used twice."""
    from ray_lightning_accelerators_amd.ops.optim import build_copy_table

    ops = _ops()
    host = R.make_copy_pairs(sdt, ddt, 41)
    srcs = [s.to(DEV)[so:] for s, so, _, _ in host]
    stor = [d.to(DEV) for _, _, d, _ in host]
    dsts = [t[do:] for t, (_, _, _, do) in zip(stor, host)]
    if sdt == "f32" and ddt == "f32":
        al = [(s.data_ptr() | t.data_ptr()) % 16 == 0 for s, t in zip(srcs, dsts)]
        assert any(al) and not all(al)   # the float4 path and the scalar path
    pairs = list(zip(srcs, dsts))

    def check(run, before):
        torch.cuda.synchronize()
        worst = R.Cmp(True, 0.0, "")
        for i, ((s, so, _, do), dst) in enumerate(zip(host, dsts)):
            c = R.check_multi_copy(dst.cpu(), s[so:], before[i], scale, accumulate)
            assert c.ok, f"{run} pair {i} (n={dst.numel()}, offsets {so}/{do}): {c.detail}"
            worst = c if c.ratio >= worst.ratio else worst
            assert torch.equal(stor[i][:do].cpu(), host[i][2][:do])   # in front of the view: untouched
        _report("multi_copy", f"{sdt}->{ddt} accumulate={accumulate} scale={scale:.3g} {run}", worst)

    before = [d[do:].clone() for _, _, d, do in host]
    ops.multi_copy(pairs, scale=scale, accumulate=accumulate)
    check("pairs", before)
    table = build_copy_table(pairs)
    assert table.shape == (sum(-(-n // R.CHUNK) for n in R.COPY_SIZES), 4)
    for run in ("table 1st", "table 2nd"):
        if accumulate:
            before = [d.cpu() for d in dsts]        # accumulates onto what the run before left
        else:
            for d in dsts:
                d.fill_(SENTINEL)
        ops.multi_copy(pairs, scale=scale, accumulate=accumulate, table=table)
        check(run, before)


# ------------------------------------------------------------------ sumsq / scale_
@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_sumsq(n):
    ops = _ops()
    x, y = R.make_vector(n, 31), 3.0 * R.make_vector(n, 32)
    xd, yd = x.to(DEV), y.to(DEV)
    a, b = ops.sumsq(xd), ops.sumsq(yd)          # back to back: each memset precedes its own atomics
    torch.cuda.synchronize()
    for name, v, out in (("x", x, a), ("3y", y, b)):
        ref, bound = R.ref_sumsq(v)
        err = abs(float(out) - ref)
        _report("sumsq", f"n={n} {name} k={R.sumsq_k(n)}",
                R.Cmp(err <= bound, err / bound, f"worst error / bound {err / bound:.3g}"))
    z = torch.zeros(n, device=DEV)
    for pos in R.one_hot_positions(n):
        z[pos] = 1.0
        got = float(ops.sumsq(z))
        z[pos] = 0.0
        assert got == 1.0, f"one-hot at {pos} of {n}: {got}"


@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_scale(n):
    ops = _ops()
    x = R.make_vector(n, 33)
    for s in (0.125, 1.0 / 3.0):
        xd = x.to(DEV)
        ops.scale_(xd, s)
        torch.cuda.synchronize()
        _report("scale_", f"n={n} s={s:.3g}", R.cmp_exact(xd.cpu(), R.ref_scale(x, s)))


# ------------------------------------------------------------------ special values
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_special_values(kind):
    """NaN, +inf, 1e20 (g * g overflows), a subnormal and -0.0 among ordinary gradients: every output
    has the class the reference predicts, the ordinary neighbours stay within their bound."""
    st = R.make_special()
    for cfg in ((R.ADAM_CONFIGS[1],) if kind == "adam" else (R.SGD_CONFIGS[1], R.SGD_CONFIGS[2])):
        if kind == "adam":
            out, bf = _run_adam(st, cfg, True)
            ref = R.ref_adam(st, cfg)
            assert torch.isnan(out["p"][1]) and out["v"][4] == float("inf")
        else:
            out, bf = _run_sgd(st, cfg, True)
            ref = R.ref_sgd(st, cfg)
            assert torch.isnan(out["p"][1]) and out["p"][3] == -float("inf")
        _report(f"{kind}_step", f"special values {cfg.name}", R.check_special(out, ref, kind, bf))


# ------------------------------------------------------------------ alignment contract
def test_misaligned_operands_are_rejected_before_any_launch():
    ops = _ops()
    n = 1024
    cfg_a, cfg_s = R.ADAM_CONFIGS[1], R.SGD_CONFIGS[4]

    def fresh():
        t = {k: torch.full((n + 1,), SENTINEL, device=DEV) for k in ("p", "g", "m", "v", "buf")}
        t["bf"] = torch.full((n + 2,), SENTINEL, dtype=torch.bfloat16, device=DEV)
        return t

    def unchanged(t):
        torch.cuda.synchronize()
        return all(bool((v == SENTINEL).all()) for v in t.values())

    def operands(t, bad):
        o = {k: (v[1:] if k == bad else v[:n]) for k, v in t.items() if k != "bf"}
        o["bf"] = t["bf"][2:] if bad == "bf" else t["bf"][:n]   # 4 bytes off an 8-byte boundary
        return o

    named = {"p": "param", "g": "grad", "m": "exp_avg", "v": "exp_avg_sq", "buf": "momentum_buffer", "bf": "param_bf16"}
    for bad in ("p", "g", "m", "v", "bf"):
        t = fresh()
        o = operands(t, bad)
        with pytest.raises(RuntimeError, match=named[bad] + " must be"):
            ops.fused_adam_(o["p"], o["g"], o["m"], o["v"], step=3, p_bf16=o["bf"], **_adam_kw(cfg_a))
        assert unchanged(t), bad
    for bad in ("p", "g", "buf", "bf"):
        t = fresh()
        o = operands(t, bad)
        with pytest.raises(RuntimeError, match=named[bad] + " must be"):
            ops.fused_sgd_(o["p"], o["g"], o["buf"], step=3, p_bf16=o["bf"], **_sgd_kw(cfg_s))
        assert unchanged(t), bad
    t = fresh()
    with pytest.raises(RuntimeError, match="x must be 16-byte aligned"):
        ops.scale_(t["p"][1:], 0.5)
    with pytest.raises(RuntimeError, match="x must be 16-byte aligned"):
        ops.sumsq(t["p"][1:])
    assert unchanged(t)
    # what the arena hands out passes: a multiple of 4 elements
    ops.scale_(t["p"][4:], 0.5)
    torch.cuda.synchronize()
    assert bool((t["p"][:4] == SENTINEL).all()) and bool((t["p"][4:] == 0.5 * SENTINEL).all())


def test_zz_worst_ratios():
    for kernel in sorted(WORST):
        print(f"[ratio] {kernel} worst over all cases: {WORST[kernel]:.3g}")
