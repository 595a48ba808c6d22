"""Shared by tests/test_optim_groups.py (GPU) and tests/test_optim_groups_cpu.py: the synthetic
arena layout whose param groups interleave, its per-group configurations, and the small modules
the planner tests fuse."""
import functools

import torch

import optim_reference as R

CHUNK = 16384   # ops.optim.GROUP_CHUNK_ELEMS / csrc/kernels.h kOptGroupChunk
MAX_GROUPS = 8  # ops.optim.MAX_OPT_GROUPS / csrc/kernels.h kOptMaxGroups
SEG_LENS = (1, 3, 4, 5, 128, 1023, CHUNK - 1, CHUNK, CHUNK + 5, 40000)
SEG_GROUPS = (0, 1, 0, 2, 1, None, 0, 2, 1, 0)
SENTINEL = 7.0


def layout(lens=SEG_LENS):
    """[(offset, numel)] with every offset rounded up to 4, and the padded total."""
    offs, off = [], 0
    for n in lens:
        offs.append((off, n))
        off += (n + 3) // 4 * 4
    return offs, off


OFFSETS, NUMEL = layout()

# three groups that differ in every per-group hyper-parameter; grad_scale is the launch's
SGD_GROUPS = (
    R.sgd_cfg("g0", lr=0.05, momentum=0.0, wd=0.01, grad_scale=0.5),
    R.sgd_cfg("g1", lr=0.02, momentum=0.9, dampening=0.1, wd=0.0, grad_scale=0.5),
    R.sgd_cfg("g2", lr=0.1, momentum=0.9, nesterov=True, wd=0.003, grad_scale=0.5),
)
ADAM_GROUPS = (
    R.adam_cfg("g0", lr=3e-3, wd=0.01, grad_scale=0.5),
    R.adam_cfg("g1", lr=1e-3, betas=(0.8, 0.95), wd=0.0, grad_scale=0.5),
    R.adam_cfg("g2", lr=5e-3, betas=(0.85, 0.99), wd=0.05, adamw=True, grad_scale=0.5),
)


def sgd_hyper(cfgs=SGD_GROUPS):
    return [dict(lr=c.lr, momentum=c.momentum, dampening=c.dampening, weight_decay=c.wd, nesterov=c.nesterov,
                 maximize=c.maximize) for c in cfgs]


def adam_hyper(cfgs=ADAM_GROUPS):
    return [dict(lr=c.lr, betas=c.betas, eps=c.eps, weight_decay=c.wd, adamw=c.adamw, maximize=c.maximize)
            for c in cfgs]


@functools.lru_cache(maxsize=8)
def arena_state(seed: int):
    """fp32 CPU arenas {p, g, m, v, buf} over the synthetic layout: every grouped segment a
    make_state of its own, pads zero with zero gradient (and zero state), the ungrouped segment
    sentinels in every buffer.  Callers clone what they change."""
    st = {k: torch.zeros(NUMEL) for k in ("p", "g", "m", "v", "buf")}
    for i, ((o, n), grp) in enumerate(zip(OFFSETS, SEG_GROUPS)):
        if grp is None:
            for k in st:
                st[k][o:o + n] = SENTINEL
            continue
        seg = R.make_state(n, seed + i)
        for k in st:
            st[k][o:o + n] = seg[k]
    return st


def covered(table: torch.Tensor, numel: int) -> torch.Tensor:
    """How many rows of a chunk table cover each arena element."""
    cov = torch.zeros(numel, dtype=torch.int64)
    for off, cnt, _ in table.tolist():
        cov[off:off + cnt] += 1
    return cov


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(7, 5)
        self.norm = torch.nn.LayerNorm(5)
        self.b = torch.nn.Linear(5, 3)


def tiny_groups(mod, wds=(0.01, 0.0)):
    """Weights with decay, everything else without: interleaved in parameters() order."""
    decay = [mod.a.weight, mod.b.weight]
    rest = [mod.a.bias, mod.norm.weight, mod.norm.bias, mod.b.bias]
    return [{"params": decay, "weight_decay": wds[0]}, {"params": rest, "weight_decay": wds[1]}]
