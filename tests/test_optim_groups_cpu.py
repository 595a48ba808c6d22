"""Param groups that interleave in the arena, without a GPU: the chunk table's properties on the
synthetic layout and on ResNet-50's real one, can_fuse's decisions, the CPU reference path of the
table-driven step against an unpatched torch.optim, and the graph-step path of a conv + BatchNorm
module whose two groups alternate (tests/test_optim_groups.py runs the kernels)."""
import copy
import functools
import logging

import pytest
import torch
from torch import nn

import optim_groups_common as C
import optim_reference as R
from ray_lightning_accelerators_amd.ops.optim import GROUP_CHUNK_ELEMS, MAX_OPT_GROUPS, build_group_table
from ray_lightning_accelerators_amd.parallel.arena import ParamArena
from ray_lightning_accelerators_amd.parallel.fused_optim import (_GroupState, _TableGroupState, can_fuse,
                                                                 fuse_optimizer)


def test_constants_match():
    assert (GROUP_CHUNK_ELEMS, MAX_OPT_GROUPS) == (C.CHUNK, C.MAX_GROUPS)


# ------------------------------------------------------------------ 6. table properties
def _check_table(table, offsets, group_of, numel):
    assert table.dtype == torch.int64 and table.dim() == 2 and table.size(1) == 3
    want = torch.full((numel,), -1, dtype=torch.int64)          # group of every element, pads included
    for (o, n), grp in zip(offsets, group_of):
        if grp is not None:
            want[o:o + (n + 3) // 4 * 4] = grp
    got = torch.full((numel,), -1, dtype=torch.int64)
    for off, cnt, grp in table.tolist():
        assert off % 4 == 0 and 0 < cnt <= C.CHUNK and off + cnt <= numel
        assert bool((got[off:off + cnt] == -1).all())            # covered once
        assert bool((want[off:off + cnt] == grp).all())          # inside one group
        got[off:off + cnt] = grp
    assert torch.equal(got, want)                                # every grouped element, no ungrouped one
    assert torch.equal(C.covered(table, numel), (want >= 0).long())


def test_table_of_the_synthetic_layout():
    table = build_group_table(C.OFFSETS, C.SEG_GROUPS)
    _check_table(table, C.OFFSETS, C.SEG_GROUPS, C.NUMEL)
    o = [off for off, _ in C.OFFSETS]
    # one row per short segment (its pad included), CHUNK + 5 in two rows, 40,000 in three; nothing at o[5]
    assert table.tolist() == [
        [o[0], 4, 0], [o[1], 4, 1], [o[2], 4, 0], [o[3], 8, 2], [o[4], 128, 1], [o[6], C.CHUNK, 0],
        [o[7], C.CHUNK, 2], [o[8], C.CHUNK, 1], [o[8] + C.CHUNK, 8, 1],
        [o[9], C.CHUNK, 0], [o[9] + C.CHUNK, C.CHUNK, 0], [o[9] + 2 * C.CHUNK, 40000 - 2 * C.CHUNK, 0]]
    # consecutive members of one group form one run, cut every CHUNK elements from the run's start
    offs, _ = C.layout((5, 7, C.CHUNK, 3))
    assert build_group_table(offs, (1, 1, 1, 0)).tolist() == [[0, C.CHUNK, 1], [C.CHUNK, 16, 1], [C.CHUNK + 16, 4, 0]]
    with pytest.raises(ValueError):
        build_group_table([(0, 4), (2, 4)], (0, 0))


@functools.lru_cache(maxsize=1)
def _resnet50():
    from ray_lightning_accelerators_amd.models.resnet import LightningResNet50

    model = LightningResNet50({"no_decay_norm_bias": True})
    arena = ParamArena(model)
    return model, arena, model.configure_optimizers()


def test_table_of_resnet50s_two_groups():
    model, arena, opt = _resnet50()
    assert len(arena.params) == 161 and arena.numel == 25557032
    decay, rest = (g["params"] for g in opt.param_groups)
    assert (len(decay), sum(p.numel() for p in decay)) == (54, 25502912)
    assert (len(rest), sum(p.numel() for p in rest)) == (107, 54120)
    assert opt.param_groups[0]["weight_decay"] == model.cfg["weight_decay"] and opt.param_groups[1]["weight_decay"] == 0
    group_of = [0 if p.dim() > 1 else 1 for p in arena.params]
    runs = 1 + sum(a != b for a, b in zip(group_of, group_of[1:]))
    assert runs == 108
    table = build_group_table(arena.offsets, group_of)
    _check_table(table, arena.offsets, group_of, arena.numel)
    # a new run starts wherever a row does not continue the row before it within one group
    rows = table.tolist()
    starts = 1 + sum(1 for a, b in zip(rows, rows[1:]) if b[2] != a[2] or b[0] != a[0] + a[1] or a[1] != C.CHUNK)
    assert starts >= 108 and len({(r[0], r[2]) for r in rows}) == len(rows)
    run_lens = []
    for (o, n), grp, prev in zip(arena.offsets, group_of, [None] + group_of[:-1]):
        if grp != prev:
            run_lens.append(0)
        run_lens[-1] += (n + 3) // 4 * 4
    assert len(run_lens) == 108 and min(run_lens) == 128
    assert len(rows) == sum(-(-n // C.CHUNK) for n in run_lens)
    # a single-group ResNet-50 (the default) is one contiguous range: no table
    single = type(model)().configure_optimizers()
    assert len(single.param_groups) == 1


# ------------------------------------------------------------------ 7. can_fuse decisions
def test_can_fuse_accepts_resnet50s_interleaved_groups():
    _, arena, opt = _resnet50()
    assert arena.contiguous_range(opt.param_groups[0]["params"]) is None
    assert can_fuse(opt, arena)


class _Many(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.layers = nn.ModuleList(nn.Linear(3, 2) for _ in range(n))


def test_can_fuse_refusals_and_the_contiguous_path(caplog):
    mod = _Many(C.MAX_GROUPS + 1)
    arena = ParamArena(mod)
    ws, bs = [l.weight for l in mod.layers], [l.bias for l in mod.layers]
    # MAX_GROUPS groups that interleave (weights apart, the biases in one): fused
    at_limit = [{"params": [w]} for w in ws[:C.MAX_GROUPS - 1]] + [{"params": ws[C.MAX_GROUPS - 1:] + bs}]
    assert len(at_limit) == C.MAX_GROUPS and can_fuse(torch.optim.SGD(at_limit, lr=0.1), arena)
    # one more: refused, and the reason logged once
    above = [{"params": [w]} for w in ws[:C.MAX_GROUPS]] + [{"params": ws[C.MAX_GROUPS:] + bs}]
    opt = torch.optim.SGD(above, lr=0.1)
    assert len(above) == C.MAX_GROUPS + 1
    with caplog.at_level(logging.INFO, logger="ray_lightning_accelerators_amd.parallel.fused_optim"):
        assert not can_fuse(opt, arena) and not can_fuse(opt, arena)
    assert sum("param groups interleave" in r.getMessage() for r in caplog.records) == 1
    assert fuse_optimizer(opt, arena) is opt and not getattr(opt, "_rla_fused", False)
    # a member outside the arena
    stray = nn.Parameter(torch.zeros(3))
    assert not can_fuse(torch.optim.SGD([{"params": ws}, {"params": bs + [stray]}], lr=0.1), arena)
    # above the limit but every group a contiguous range: fused as before, one launch per group
    per_layer = [{"params": [l.weight, l.bias]} for l in mod.layers]
    opt = torch.optim.SGD(per_layer, lr=0.1)
    assert can_fuse(opt, arena) and fuse_optimizer(opt, arena)._rla_fused
    assert all(type(gs) is _GroupState for gs in opt._rla_groups)
    assert [(gs.start, gs.end) for gs in opt._rla_groups] == [(12 * i, 12 * i + 12) for i in range(len(per_layer))]


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_contiguous_groups_keep_their_ranges(kind):
    """The layout tests/test_optim_kernels.py fuses (arena reordered by group) and a single group:
    plain _GroupStates with the (start, end) they have always had, buffers of their own."""
    mod = C._Tiny()
    groups = C.tiny_groups(mod)
    arena = ParamArena(mod, params=groups[0]["params"] + groups[1]["params"])
    opt = torch.optim.SGD(groups, lr=0.05, momentum=0.9) if kind == "sgd" else torch.optim.Adam(groups, lr=3e-3)
    assert fuse_optimizer(opt, arena) is opt and opt._rla_fused
    assert all(type(gs) is _GroupState for gs in opt._rla_groups)
    assert [(gs.start, gs.end) for gs in opt._rla_groups] == [(0, 52), (52, arena.numel)] and arena.numel == 80
    buf = "buf" if kind == "sgd" else "m"
    assert [getattr(gs, buf).numel() for gs in opt._rla_groups] == [52, 28]
    mod = C._Tiny()
    arena = ParamArena(mod)
    opt = torch.optim.SGD(mod.parameters(), lr=0.05, momentum=0.9)
    fuse_optimizer(opt, arena)
    assert [(type(gs), gs.start, gs.end) for gs in opt._rla_groups] == [(_GroupState, 0, arena.numel)]


def test_add_param_group_after_fusing_raises():
    mod = C._Tiny()
    arena = ParamArena(mod)
    opt = torch.optim.SGD([{"params": [mod.a.weight, mod.a.bias]}], lr=0.05)
    fuse_optimizer(opt, arena)
    with pytest.raises(RuntimeError, match="add_param_group"):
        opt.add_param_group({"params": [mod.b.weight]})
    assert len(opt.param_groups) == 1


# ------------------------------------------------------------------ 8. CPU reference path against torch
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_cpu_path_against_torch(kind):
    """Three steps of the fused two-group optimizer on _Tiny in parameters() order against a stock
    torch.optim of the same groups on a deep copy, handed the fused optimizer's state before each
    step (through state_dict, torch's own format) and the same gradients: both are fp32 evaluations
    of one reference step, so they differ by at most twice its bound."""
    torch.manual_seed(5)
    mod = C._Tiny()
    twin = copy.deepcopy(mod)
    arena = ParamArena(mod)
    # the reference takes every hyper-parameter at its fp32 value (the kernel's): both optimizers
    # are handed those values, as tests/test_optim_reference.py hands them to torch.optim
    f = R.f32
    wds = (f(0.01), 0.0)
    if kind == "sgd":
        make = lambda m: torch.optim.SGD(C.tiny_groups(m, wds), lr=f(0.05), momentum=f(0.9))   # noqa: E731
        cfgs = [R.sgd_cfg("group", momentum=0.9, wd=w) for w in wds]
    else:
        make = lambda m: torch.optim.Adam(C.tiny_groups(m, wds), lr=f(3e-3), betas=(f(0.9), f(0.999)),  # noqa: E731
                                          eps=f(1e-8))
        cfgs = [R.adam_cfg("group", wd=w) for w in wds]
    opt, ref_opt = make(mod), make(twin)
    assert fuse_optimizer(opt, arena) is opt and opt._rla_fused
    assert all(type(gs) is _TableGroupState for gs in opt._rla_groups)
    names = [n for n, _ in mod.named_parameters()]
    group_of = {"a.weight": 0, "b.weight": 0}
    for step, lr in enumerate((0.05, 0.02, 0.1) if kind == "sgd" else (3e-3, 1e-3, 5e-3), 1):
        for o in (opt, ref_opt):
            for grp in o.param_groups:
                grp["lr"] = f(lr)
        ref_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
        pre = {}
        gen = torch.Generator().manual_seed(60 + step)
        for (n, p), q in zip(mod.named_parameters(), twin.parameters()):
            q.data.copy_(p.data)
            g = 0.3 * torch.randn(p.shape, generator=gen)
            p.grad.copy_(g)
            q.grad = g.clone()
            st = opt.state[p]
            pre[n] = {"p": p.detach().clone().reshape(-1), "g": g.reshape(-1)}
            for k, key in (("m", "exp_avg"), ("v", "exp_avg_sq"), ("buf", "momentum_buffer")):
                if key in st:
                    pre[n][k] = st[key].detach().clone().reshape(-1)
        opt.step()
        ref_opt.step()
        for (n, p), q in zip(mod.named_parameters(), twin.parameters()):
            cfg = cfgs[group_of.get(n, 1)]
            ref = (R.ref_sgd if kind == "sgd" else R.ref_adam)(pre[n], cfg, t=step, lr=lr, exact_scalars=True)
            out = {"p": p.detach().reshape(-1)}
            st = opt.state[p]
            if kind == "sgd":
                out["buf"] = st["momentum_buffer"].reshape(-1)
                c = R.check_sgd(out, ref)
            else:
                out["m"], out["v"] = st["exp_avg"].reshape(-1), st["exp_avg_sq"].reshape(-1)
                c = R.check_adam(out, ref)
                assert float(st["step"]) == step
            assert c.ok, f"{kind} step {step} {n}: {c.detail}"
            diff = (p.detach().double() - q.detach().double()).abs().reshape(-1)
            assert bool((diff <= 2 * ref["bp"]).all()), f"{kind} step {step} {n}: {float((diff / ref['bp']).max())}"
    assert names == [n for n, _ in twin.named_parameters()]
    sd, rsd = opt.state_dict(), ref_opt.state_dict()
    assert sd["param_groups"] == rsd["param_groups"] and sd["state"].keys() == rsd["state"].keys()
    for i in rsd["state"]:
        assert {k: tuple(v.shape) for k, v in sd["state"][i].items()} == \
            {k: tuple(v.shape) for k, v in rsd["state"][i].items()}


def test_cpu_path_leaves_ungrouped_elements_alone():
    """The reference path over the synthetic layout, device-scalar style [G] tensors on the CPU:
    the ungrouped segment and the velocity under the momentum-0 group are bitwise unchanged."""
    from ray_lightning_accelerators_amd.ops.optim import fused_sgd_groups_

    st = {k: v.clone() for k, v in C.arena_state(70).items()}
    table = build_group_table(C.OFFSETS, C.SEG_GROUPS)
    bf = torch.full((C.NUMEL,), C.SENTINEL, dtype=torch.bfloat16)
    fused_sgd_groups_(st["p"], st["g"], st["buf"], table, C.sgd_hyper(), steps=torch.tensor([7, 7, 7]),
                      grad_scale=0.5, lr_tensor=torch.tensor([c.lr for c in C.SGD_GROUPS]), p_bf16=bf)
    pre = C.arena_state(70)
    for (o, n), grp in zip(C.OFFSETS, C.SEG_GROUPS):
        s = slice(o, o + n)
        if grp is None:
            assert all(torch.equal(st[k][s], pre[k][s]) for k in st) and bool((bf[s] == C.SENTINEL).all())
            continue
        cfg = C.SGD_GROUPS[grp]
        out = {"p": st["p"][s]}
        if cfg.momentum != 0:
            out["buf"] = st["buf"][s]
        else:
            assert torch.equal(st["buf"][s], pre["buf"][s])
        seg = {k: pre[k][s] for k in ("p", "g", "buf")}
        c = R.check_sgd(out, R.ref_sgd(seg, cfg, t=7), bf[s])
        assert c.ok, f"segment at {o} (n={n}, group {grp}): {c.detail}"
    with pytest.raises(RuntimeError, match="group index"):
        fused_sgd_groups_(st["p"], st["g"], st["buf"], table, C.sgd_hyper()[:2], steps=[1, 1])
    with pytest.raises(RuntimeError, match="groups"):
        fused_sgd_groups_(st["p"], st["g"], st["buf"], table, C.sgd_hyper() * 3, steps=[1] * 9)


# ------------------------------------------------------------------ 9. graph step
def _interleaved_tiny():
    from test_graph_step import Tiny

    class TwoGroups(Tiny):
        """Tiny (conv + BatchNorm + linear) with weight decay on the dim > 1 parameters only."""

        def configure_optimizers(self):
            params = list(self.parameters())
            groups = [{"params": [p for p in params if p.dim() > 1], "weight_decay": 1e-4},
                      {"params": [p for p in params if p.dim() <= 1], "weight_decay": 0.0}]
            if self.opt_kind == "adam":
                opt = torch.optim.Adam(groups, lr=1e-2)
            else:
                opt = torch.optim.SGD(groups, lr=0.05, momentum=0.9)
            if self.sched:
                return [opt], [{"scheduler": torch.optim.lr_scheduler.StepLR(opt, 2, 0.5), "interval": "step"}]
            return opt

    return TwoGroups


@pytest.mark.parametrize("opt,sched", [("sgd", False), ("adam", False), ("sgd", True)])
def test_graph_step_takes_interleaved_groups(tmpdir, opt, sched):
    from ray_lightning_accelerators_amd.lightning.graph_step import GraphedTrainStep, static_reason
    from test_graph_step import _fit

    TwoGroups = _interleaved_tiny()
    t_g, r_g = _fit(TwoGroups(opt=opt, sched=sched), tmpdir, "g")
    o = t_g.optimizers[0]
    assert len(o.param_groups) == 2 and t_g.accelerator_backend.arena.contiguous_range(o.param_groups[0]["params"]) is None
    assert getattr(o, "_rla_fused", False) and all(type(gs) is _TableGroupState for gs in o._rla_groups)
    assert static_reason(t_g, t_g.model) is None and t_g._graph_step_reason is None
    assert isinstance(t_g._fused, GraphedTrainStep) and not t_g._fused.failed and t_g._fused.steps_done == 24
    # the per-group device scalars are slices of one [G] tensor each
    assert all(gs.step_t.data_ptr() == o._rla_groups[0].step_t.data_ptr() + 8 * i for i, gs in enumerate(o._rla_groups))
    assert [int(gs.step_t) for gs in o._rla_groups] == [24, 24] and [gs.step for gs in o._rla_groups] == [24, 24]
    m_e = TwoGroups(opt=opt, sched=sched)
    m_e.hip_graph_step = False
    t_e, r_e = _fit(m_e, tmpdir, "e")
    assert t_e._fused is None
    assert r_g.losses == r_e.losses and len(r_g.losses) == 24
    for (k, a), b in zip(t_g.model.state_dict().items(), t_e.model.state_dict().values()):
        assert torch.equal(a, b), k
    sd_g, sd_e = o.state_dict(), t_e.optimizers[0].state_dict()
    for i in sd_e["state"]:
        for k, v in sd_e["state"][i].items():
            assert torch.equal(sd_g["state"][i][k], v), (i, k)
