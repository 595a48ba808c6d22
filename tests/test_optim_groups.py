"""sgd_groups_kernel / adam_groups_kernel of csrc/optim_kernels.hip: ONE launch that steps param
groups which interleave in the arena, through a chunk table.  Every segment of a synthetic layout
(lengths 1 .. 40,000 around the chunk size, three groups and one member of no group) against the
float64 single-step references of tests/optim_reference.py, bit for bit against the single-group
kernels, under graph replay with per-group device scalars, and through fuse_optimizer on an arena in
parameters() order.  Bounds and input makers are optim_reference's own."""
import copy

import pytest
import torch

import optim_groups_common as C
import optim_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = {"sgd": ("p", "buf"), "adam": ("p", "m", "v")}
CFGS = {"sgd": C.SGD_GROUPS, "adam": C.ADAM_GROUPS}
SEGMENTS = list(zip(C.OFFSETS, C.SEG_GROUPS))


def _ops():
    from ray_lightning_accelerators_amd import ops

    ops.require()
    return ops


def _table():
    from ray_lightning_accelerators_amd.ops.optim import build_group_table

    return build_group_table(C.OFFSETS, C.SEG_GROUPS, device=DEV)


def _hyper(kind, lr=None):
    hyper = C.sgd_hyper() if kind == "sgd" else C.adam_hyper()
    if lr is not None:
        for h in hyper:
            h["lr"] = lr
    return hyper


def _device_arenas(kind, st):
    d = {k: st[k].to(DEV) for k in KEYS[kind] + ("g",)}
    d["bf"] = torch.full((C.NUMEL,), C.SENTINEL, dtype=torch.bfloat16, device=DEV)
    return d


def _launch(kind, d, table, hyper, steps, lr_tensor=None):
    ops = _ops()
    if kind == "sgd":
        ops.fused_sgd_groups_(d["p"], d["g"], d["buf"], table, hyper, steps=steps, grad_scale=0.5,
                              lr_tensor=lr_tensor, p_bf16=d["bf"])
    else:
        ops.fused_adam_groups_(d["p"], d["g"], d["m"], d["v"], table, hyper, steps=steps, grad_scale=0.5,
                               lr_tensor=lr_tensor, p_bf16=d["bf"])


def _check_segment(kind, out, pre, cfg, t, lr=None, shadow=None):
    if kind == "sgd":
        if cfg.momentum == 0:
            out = {"p": out["p"]}
        return R.check_sgd(out, R.ref_sgd(pre, cfg, t=t, lr=lr), shadow)
    return R.check_adam(out, R.ref_adam(pre, cfg, t=t, lr=lr), shadow)


def _check_arena(kind, got, pre, t, lrs=None, what=""):
    """Every segment of the CPU arenas ``got`` (p, state, bf) as one reference step of its group from
    ``pre``; the ungrouped segment, the velocity under the momentum-0 group and the gradient bitwise
    unchanged; pads zero."""
    keys = KEYS[kind]
    in_segment = torch.zeros(C.NUMEL, dtype=torch.bool)
    for (o, n), grp in SEGMENTS:
        s = slice(o, o + n)
        in_segment[s] = True
        if grp is None:
            for k in keys:
                assert torch.equal(got[k][s], pre[k][s]), f"{what}: ungrouped {k} changed"
            assert bool((got["bf"][s] == C.SENTINEL).all()), f"{what}: ungrouped shadow written"
            continue
        cfg = CFGS[kind][grp]
        if kind == "sgd" and cfg.momentum == 0:
            assert torch.equal(got["buf"][s], pre["buf"][s]), f"{what}: velocity of a momentum-0 group changed"
        c = _check_segment(kind, {k: got[k][s] for k in keys}, {k: pre[k][s] for k in pre}, cfg, t,
                           None if lrs is None else lrs[grp], got["bf"][s])
        print(f"[ratio] {kind}_groups {what} segment at {o} n={n} group {grp}: {c.detail}")
        assert c.ok, f"{what} segment at {o} (n={n}, group {grp}): {c.detail}"
    for k in keys:
        assert bool((got[k][~in_segment] == 0).all()), f"{what}: pad of {k} not zero"
    assert torch.equal(got["g"], pre["g"])


def _cpu(d):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


# ------------------------------------------------------------------ 1. against fp64, 2. same bits
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_every_segment_against_fp64_and_the_single_group_kernels(kind, t):
    ops = _ops()
    pre = C.arena_state(80)
    d = _device_arenas(kind, pre)
    table = _table()
    assert table.is_cuda and table.shape == (12, 3) and torch.equal(table.cpu(), table._rla_host)
    _launch(kind, d, table, _hyper(kind), [t] * 3)
    got = _cpu(d)
    _check_arena(kind, got, pre, t, what=f"t={t}")
    # The same segments through fused_sgd_ / fused_adam_, one slice and one launch each.  The slice is
    # the one the arena hands out, alignment pad included (ParamArena.contiguous_range rounds a range's
    # end up to 4): every element then goes through the single-group kernel's float4 body, as it does
    # in the grouped launch and in a single-group launch over the whole arena -- all bits equal.
    # On the bare slice [o, o + n) sgd_kernel / adam_kernel hand the last n % 4 elements to their
    # scalar tail, which the compiler contracts into other fmas than their own body (sgd: the body
    # rounds buf * momentum and adds it inside the fma of (1 - dampening) * g, the tail the other way
    # round), so there the comparison covers the first n - n % 4 elements and the differing tail
    # elements are counted and printed.
    for padded in (True, False):
        e = _device_arenas(kind, pre)
        for (o, n), grp in SEGMENTS:
            if grp is None:
                continue
            s, cfg = slice(o, o + ((n + 3) // 4 * 4 if padded else n)), CFGS[kind][grp]
            if kind == "sgd":
                ops.fused_sgd_(e["p"][s], e["g"][s], e["buf"][s] if cfg.momentum != 0 else None, step=t,
                               p_bf16=e["bf"][s], lr=cfg.lr, momentum=cfg.momentum, dampening=cfg.dampening,
                               weight_decay=cfg.wd, grad_scale=0.5, nesterov=cfg.nesterov, maximize=cfg.maximize)
            else:
                ops.fused_adam_(e["p"][s], e["g"][s], e["m"][s], e["v"][s], step=t, p_bf16=e["bf"][s], lr=cfg.lr,
                                betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.wd, grad_scale=0.5, adamw=cfg.adamw,
                                maximize=cfg.maximize)
        one = _cpu(e)
        if padded:
            for k in KEYS[kind] + ("bf",):
                assert torch.equal(got[k], one[k]), f"{k} differs from the single-group kernel"
            continue
        tail_diff = 0
        for (o, n), _ in SEGMENTS:
            body, tail = slice(o, o + n - n % 4), slice(o + n - n % 4, o + n)
            for k in KEYS[kind] + ("bf",):
                assert torch.equal(got[k][body], one[k][body]), f"{k} of the segment at {o} differs in the float4 body"
                tail_diff += int((got[k][tail] != one[k][tail]).sum())
        print(f"[bits] {kind}_groups t={t}: {tail_diff} values differ from the single-group kernels' scalar tails "
              f"(of {sum(n % 4 for (_, n), g in SEGMENTS if g is not None)} tail elements)")


# ------------------------------------------------------------------ 3. device scalars under graph replay
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_graph_replay_reads_every_groups_step_and_lr(kind):
    """One captured grouped step (the [G] counter's add_ then the kernel) replayed three times, each
    group's device learning rate changed to a value of its own in between."""
    st0 = C.arena_state(81)
    d = _device_arenas(kind, st0)
    table = _table()
    hyper = _hyper(kind, lr=123.0)            # the host rates must be ignored
    step_all = torch.zeros(3, dtype=torch.int64, device=DEV)
    lr_all = torch.zeros(3, device=DEV)

    def body():
        step_all.add_(1)
        _launch(kind, d, table, hyper, step_all, lr_all)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in KEYS[kind]:                          # the warm-up moved the state: put it back
        d[k].copy_(st0[k])
    d["bf"].fill_(C.SENTINEL)
    step_all.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    torch.cuda.synchronize()
    assert step_all.tolist() == [0, 0, 0] and torch.equal(d["p"].cpu(), st0["p"])   # a capture runs nothing
    scale = 0.1 if kind == "adam" else 1.0
    for i, lrs in enumerate(((0.05, 0.02, 0.3), (0.01, 0.2, 0.004), (0.3, 0.001, 0.07)), 1):
        lrs = [lr * scale for lr in lrs]
        pre = _cpu(d)
        fresh = C.arena_state(81 + i)["g"]
        pre["g"] = torch.where(st0["g"] == 0, st0["g"], fresh)    # pads keep a zero gradient
        for (o, n), grp in SEGMENTS:
            if grp is None:
                pre["g"][o:o + n] = C.SENTINEL
        d["g"].copy_(pre["g"])
        lr_all.copy_(torch.tensor(lrs))
        graph.replay()
        got = _cpu(d)
        assert step_all.tolist() == [i, i, i]
        _check_arena(kind, got, pre, i, lrs, what=f"replay {i}")
        for (o, n), grp in SEGMENTS:              # a neighbouring group's rate is not this group's
            if grp is not None and n >= 128:
                s = slice(o, o + n)
                c = _check_segment(kind, {k: got[k][s] for k in KEYS[kind]}, {k: pre[k][s] for k in pre},
                                   CFGS[kind][grp], i, lrs[(grp + 1) % 3])
                assert not c.ok, f"replay {i}: the segment at {o} also matches group {(grp + 1) % 3}'s rate"


# ------------------------------------------------------------------ 4. fuse_optimizer, natural order
def _fused_tiny(kind):
    from ray_lightning_accelerators_amd.parallel.arena import ParamArena
    from ray_lightning_accelerators_amd.parallel.fused_optim import fuse_optimizer

    torch.manual_seed(3)
    mod = C._Tiny().to(DEV)
    arena = ParamArena(mod)                       # parameters() order: the two groups interleave
    arena.enable_bf16_shadow()
    groups = C.tiny_groups(mod)
    opt = torch.optim.SGD(groups, lr=0.05, momentum=0.9) if kind == "sgd" else torch.optim.Adam(groups, lr=3e-3)
    assert arena.contiguous_range(groups[0]["params"]) is None
    assert fuse_optimizer(opt, arena, grad_scale_fn=lambda: 0.5) is opt and getattr(opt, "_rla_fused", False)
    opt.enable_device_scalars()
    return mod, arena, opt


def _tiny_step(arena, opt, step, lrs):
    for grp, lr in zip(opt.param_groups, lrs):
        grp["lr"] = lr
    g = 0.3 * torch.randn(arena.numel, generator=torch.Generator().manual_seed(40 + step))
    arena.grad.copy_(g)
    opt.step()
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_fuse_optimizer_on_a_natural_order_arena(kind):
    from ray_lightning_accelerators_amd.parallel.fused_optim import _TableGroupState

    mod, arena, opt = _fused_tiny(kind)
    gss = opt._rla_groups
    assert len(gss) == 2 and all(type(gs) is _TableGroupState for gs in gss) and arena.numel == 80
    state_keys = ("m", "v") if kind == "adam" else ("buf",)
    names = {"m": "exp_avg", "v": "exp_avg_sq", "buf": "momentum_buffer"}
    for k in state_keys:                          # one arena-shaped buffer per optimizer, shared by the groups
        assert getattr(gss[0], k) is getattr(gss[1], k) and getattr(gss[0], k).numel() == arena.numel
    assert gss[1].step_t.data_ptr() == gss[0].step_t.data_ptr() + 8 and gss[1].lr_t.data_ptr() == gss[0].lr_t.data_ptr() + 4
    wds = (0.01, 0.0)
    cfgs = [R.sgd_cfg("group", momentum=0.9, wd=w, grad_scale=0.5) if kind == "sgd" else
            R.adam_cfg("group", wd=w, grad_scale=0.5) for w in wds]
    members = []
    for gi, grp in enumerate(opt.param_groups):
        for q in grp["params"]:
            o, n = arena.offsets[arena.index_of(q)]
            members.append((gi, q, o, n))
            assert q.data_ptr() == arena.data.data_ptr() + 4 * o
            for k in state_keys:                  # optimizer.state[p] views alias the shared buffers at the arena offset
                assert opt.state[q][names[k]].data_ptr() == getattr(gss[gi], k).data_ptr() + 4 * o
                assert opt.state[q][names[k]].shape == q.shape
    rates = ((0.05, 0.02), (0.02, 0.1), (0.1, 0.004)) if kind == "sgd" else ((3e-3, 1e-3), (1e-3, 5e-3), (5e-3, 2e-4))
    for step, lrs in enumerate(rates, 1):
        pre = {k: getattr(gss[0], k).cpu() for k in state_keys}
        pre["p"] = arena.data.cpu()
        pre["g"] = _tiny_step(arena, opt, step, lrs).clone()
        post = {k: getattr(gss[0], k).cpu() for k in state_keys}
        post["p"], bf = arena.data.cpu(), arena.bf16.cpu()
        for gi, q, o, n in members:
            s = slice(o, o + n)
            c = _check_segment(kind, {k: post[k][s] for k in state_keys + ("p",)}, {k: pre[k][s] for k in pre},
                               cfgs[gi], step, lrs[gi], bf[s])
            print(f"[ratio] {kind}_groups fuse_optimizer step {step} param at {o} group {gi}: {c.detail}")
            assert c.ok, f"step {step} param at {o} (group {gi}): {c.detail}"
            assert torch.equal(q.detach().cpu().reshape(-1), post["p"][s])
        assert [int(gs.step_t) for gs in gss] == [step, step] and [gs.step for gs in gss] == [step, step]
    # state_dict: torch's keys and shapes
    twin = C._Tiny()
    stock = torch.optim.SGD(C.tiny_groups(twin), lr=0.05, momentum=0.9) if kind == "sgd" else \
        torch.optim.Adam(C.tiny_groups(twin), lr=3e-3)
    for q in twin.parameters():
        q.grad = torch.ones_like(q)
    stock.step()
    sd, ref = opt.state_dict(), stock.state_dict()
    assert sd["state"].keys() == ref["state"].keys()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in ref["param_groups"]]
    for i in ref["state"]:
        assert {k: tuple(v.shape) for k, v in sd["state"][i].items()} == \
            {k: tuple(v.shape) for k, v in ref["state"][i].items()}


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_state_dict_round_trip_changes_no_bit(kind):
    runs = []
    for round_trip in (False, True):
        mod, arena, opt = _fused_tiny(kind)
        for step in (1, 2):
            _tiny_step(arena, opt, step, (0.05, 0.02) if kind == "sgd" else (3e-3, 1e-3))
        if round_trip:
            opt.load_state_dict(copy.deepcopy(opt.state_dict()))
        _tiny_step(arena, opt, 3, (0.02, 0.1) if kind == "sgd" else (1e-3, 5e-3))
        gs = opt._rla_groups[0]
        runs.append([arena.data.cpu(), arena.bf16.cpu()] +
                    [getattr(gs, k).cpu() for k in (("m", "v") if kind == "adam" else ("buf",))])
        assert [int(g.step_t) for g in opt._rla_groups] == [3, 3]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 5. operands refused before any launch
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_bad_operands_are_refused_before_any_launch(kind):
    ops = _ops()
    pre = C.arena_state(82)
    table = _table()
    keys = KEYS[kind] + ("g",)
    base = {k: torch.cat([pre[k], torch.full((4,), C.SENTINEL)]).to(DEV) for k in keys}
    d = {k: base[k][:C.NUMEL] for k in keys}
    d["bf"] = torch.full((C.NUMEL,), C.SENTINEL, dtype=torch.bfloat16, device=DEV)

    def refused(match, table=table, hyper=None, steps=(3, 3, 3), **swap):
        with pytest.raises(RuntimeError, match=match):
            _launch(kind, dict(d, **swap), table, hyper or _hyper(kind), list(steps))
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(base[k][:C.NUMEL].cpu(), pre[k]), f"{match}: {k} changed"
        assert bool((d["bf"] == C.SENTINEL).all())

    refused("table must be a GPU tensor", table=table.cpu())
    refused("table has dtype", table=table.to(torch.int32))
    refused(r"table must be \[nchunks, 3\]", table=torch.cat([table, table], dim=1)[:, :4].contiguous())
    bad = table.clone()
    bad[2, 2] = 3
    refused("group index 3 is not below the group count 3", table=bad)
    bad = table.clone()
    bad[-1, 1] = C.CHUNK + 4
    refused("count", table=bad)
    bad = table.clone()
    bad[-1, 0] = C.NUMEL
    refused("reaches beyond", table=bad)
    bad = table.clone()
    bad[0, 0] = 2
    refused("not a multiple of 4", table=bad)
    refused("param must be 16-byte aligned", p=base["p"][1:1 + C.NUMEL])
    refused("grad must be 16-byte aligned", g=base["g"][1:1 + C.NUMEL])
    refused("param_bf16 must be 8-byte aligned",
            bf=torch.full((C.NUMEL + 2,), C.SENTINEL, dtype=torch.bfloat16, device=DEV)[2:])
    too_many = (_hyper(kind) * 3)[:C.MAX_GROUPS + 1]
    refused("groups", hyper=too_many, steps=[3] * (C.MAX_GROUPS + 1))
    G = C.MAX_GROUPS + 1                          # and the binding itself, past the Python check
    with pytest.raises(RuntimeError, match="the kernel takes 1 to"):
        if kind == "sgd":
            ops.require().sgd_groups_step(d["p"], d["g"], d["buf"], d["bf"], table, table._rla_host, [0.1] * G, [0.9] * G,
                                          [0.0] * G, [0.0] * G, [False] * G, [False] * G, 0.5, None, [3] * G, None)
        else:
            ops.require().adam_groups_step(d["p"], d["g"], d["m"], d["v"], d["bf"], table, table._rla_host, [0.1] * G,
                                           [0.9] * G, [0.999] * G, [1e-8] * G, [0.0] * G, [False] * G, [False] * G, 0.5,
                                           None, [3] * G, None)
    # and what the arena hands out passes
    _launch(kind, d, table, _hyper(kind), [3, 3, 3])
    torch.cuda.synchronize()
    assert not torch.equal(d["p"].cpu(), pre["p"])
