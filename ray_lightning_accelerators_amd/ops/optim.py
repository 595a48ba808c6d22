"""Flat-arena optimizer steps and bucket copy kernels (HIP on GPU, torch on CPU).

Replaces the upstream ``torch.optim.Adam``/``SGD`` steps and DDP bucket
flatten/unflatten the reference relies on.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import torch

from . import require, use_native

StepLike = Union[int, torch.Tensor]


def _step_args(step: StepLike) -> Tuple[Optional[torch.Tensor], int]:
    if isinstance(step, torch.Tensor):
        return step, 0
    return None, int(step)


def fused_adam_(
    p: torch.Tensor,
    g: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    *,
    lr: float,
    betas: Tuple[float, float] = (0.9, 0.999),
    eps: float = 1e-8,
    weight_decay: float = 0.0,
    grad_scale: float = 1.0,
    adamw: bool = False,
    maximize: bool = False,
    step: StepLike = 1,
    lr_tensor: Optional[torch.Tensor] = None,
    p_bf16: Optional[torch.Tensor] = None,
) -> None:
    """One Adam/AdamW step over flat fp32 arenas, in place.

    ``step`` is the 1-based step number AFTER this update (torch semantics), a
    Python int or a device int64 tensor (graph-replay friendly).

    Alignment contract (GPU): the kernel reads and writes float4s and stores the
    shadow as packed bf16x4, so ``p``, ``g``, ``m`` and ``v`` must start on a 16-byte
    boundary and ``p_bf16`` on an 8-byte one -- a view into an arena must start at a
    multiple of 4 elements, which ``ParamArena(align=4)`` guarantees.  Anything else
    raises ``RuntimeError`` naming the operand before a launch is issued.  ``n`` itself
    is free: the last ``n % 4`` elements take a scalar tail.
    """
    if use_native(p):
        step_t, host_step = _step_args(step)
        require().adam_step(
            p, g, m, v, p_bf16, float(lr), float(betas[0]), float(betas[1]), float(eps),
            float(weight_decay), float(grad_scale), bool(adamw), bool(maximize), step_t,
            host_step, lr_tensor,
        )
        return
    t = int(step.item()) if isinstance(step, torch.Tensor) else int(step)
    lr_v = float(lr_tensor.item()) if lr_tensor is not None else float(lr)
    b1, b2 = betas
    with torch.no_grad():
        grad = g * grad_scale if grad_scale != 1.0 else g.clone()
        if maximize:
            grad = -grad
        if weight_decay != 0:
            if adamw:
                p.mul_(1 - lr_v * weight_decay)
            else:
                grad = grad.add(p, alpha=weight_decay)
        m.lerp_(grad, 1 - b1)
        v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
        p.addcdiv_(m, denom, value=-(lr_v / bc1))
        if p_bf16 is not None:
            p_bf16.copy_(p)


def fused_sgd_(
    p: torch.Tensor,
    g: torch.Tensor,
    buf: Optional[torch.Tensor],
    *,
    lr: float,
    momentum: float = 0.0,
    dampening: float = 0.0,
    weight_decay: float = 0.0,
    nesterov: bool = False,
    maximize: bool = False,
    grad_scale: float = 1.0,
    step: StepLike = 1,
    lr_tensor: Optional[torch.Tensor] = None,
    p_bf16: Optional[torch.Tensor] = None,
) -> None:
    """One SGD step (torch.optim.SGD semantics) over flat fp32 arenas.

    ``step <= 1`` overwrites the momentum buffer with the gradient, later steps blend
    it.  Alignment contract (GPU) as :func:`fused_adam_`: ``p``, ``g`` and ``buf`` on a
    16-byte boundary, ``p_bf16`` on an 8-byte one, else ``RuntimeError``.
    """
    if use_native(p):
        step_t, host_step = _step_args(step)
        require().sgd_step(
            p, g, buf, p_bf16, float(lr), float(momentum), float(dampening), float(weight_decay),
            float(grad_scale), bool(nesterov), bool(maximize), step_t, host_step, lr_tensor,
        )
        return
    t = int(step.item()) if isinstance(step, torch.Tensor) else int(step)
    lr_v = float(lr_tensor.item()) if lr_tensor is not None else float(lr)
    with torch.no_grad():
        d = g * grad_scale if grad_scale != 1.0 else g.clone()
        if maximize:
            d = -d
        if weight_decay != 0:
            d = d.add(p, alpha=weight_decay)
        if momentum != 0:
            assert buf is not None
            if t <= 1:
                buf.copy_(d)
            else:
                buf.mul_(momentum).add_(d, alpha=1 - dampening)
            d = d.add(buf, alpha=momentum) if nesterov else buf
        p.add_(d, alpha=-lr_v)
        if p_bf16 is not None:
            p_bf16.copy_(p)


MAX_OPT_GROUPS = 8  # csrc/kernels.h kOptMaxGroups
GROUP_CHUNK_ELEMS = 16384  # csrc/kernels.h kOptGroupChunk


def build_group_table(arena_offsets: Sequence[Tuple[int, int]], group_of_param: Sequence[Optional[int]],
                      device=None, chunk: int = GROUP_CHUNK_ELEMS, align: int = 4) -> torch.Tensor:
    """Chunk table of :func:`fused_sgd_groups_` / :func:`fused_adam_groups_`: int64
    ``[rows, 3]``, one row ``(arena element offset, element count, group index)`` per chunk.

    ``arena_offsets`` are the arena's ``(offset, numel)`` per member in arena order
    (``ParamArena.offsets``: every offset a multiple of ``align``), ``group_of_param`` each
    member's group index, or ``None`` for a member of no group.  A chunk is a run of
    consecutive members of one group, the alignment pad after each member included, cut into
    pieces of at most ``chunk`` elements; members of no group are covered by no row.

    Built once per optimizer, never inside a graph capture.  On a GPU the table is copied
    through pinned memory; the host rows stay attached (``table._rla_host``), and the
    bindings check them before every launch."""
    if len(arena_offsets) != len(group_of_param):
        raise ValueError("build_group_table: one group index (or None) per arena member")
    if chunk <= 0 or chunk % align:
        raise ValueError(f"build_group_table: chunk must be a positive multiple of {align}")
    rows: List[List[int]] = []
    run_start = run_end = 0
    run_group: Optional[int] = None

    def flush():
        if run_group is not None:
            for off, cnt in iter_chunks(run_end - run_start, chunk):
                rows.append([run_start + off, cnt, run_group])

    prev_end = 0
    for (off, n), grp in zip(arena_offsets, group_of_param):
        if off % align or off < prev_end:
            raise ValueError("build_group_table: arena offsets must be aligned and ascending")
        end = off + (n + align - 1) // align * align
        prev_end = end
        grp = None if grp is None or grp < 0 else int(grp)
        if grp is not None and grp == run_group and off == run_end:
            run_end = end
            continue
        flush()
        run_start, run_end, run_group = off, end, grp
    flush()
    host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)
    dev = torch.device(device if device is not None else "cpu")
    if dev.type != "cuda":
        return host
    pinned = host.pin_memory()
    table = pinned.to(dev, non_blocking=True)
    table._rla_pinned = pinned
    table._rla_host = host
    return table


def _table_host(table: torch.Tensor) -> torch.Tensor:
    host = getattr(table, "_rla_host", None)
    # a table that build_group_table did not make: one device read (not capturable)
    return host if host is not None else table.detach().cpu()


def _group_steps(steps, ngroups: int) -> Tuple[Optional[torch.Tensor], List[int]]:
    if isinstance(steps, torch.Tensor):
        return steps, [0] * ngroups
    steps = [int(s) for s in steps]
    if len(steps) != ngroups:
        raise ValueError(f"{len(steps)} step counters for {ngroups} param groups")
    return None, steps


def _check_groups(groups: Sequence[dict]) -> int:
    if not 1 <= len(groups) <= MAX_OPT_GROUPS:
        raise RuntimeError(f"param groups: {len(groups)} groups, the kernel takes 1 to {MAX_OPT_GROUPS}")
    return len(groups)


def _reference_rows(table: torch.Tensor, ngroups: int, numel: int) -> List[List[int]]:
    rows = _table_host(table).tolist()
    for i, (off, cnt, grp) in enumerate(rows):
        if not 0 <= grp < ngroups:
            raise RuntimeError(f"table row {i}: group index {grp} is not below the group count {ngroups}")
        if off < 0 or cnt <= 0 or off + cnt > numel:
            raise RuntimeError(f"table row {i}: [{off}, {off + cnt}) reaches beyond the arena's {numel} elements")
    return rows


def fused_adam_groups_(
    p: torch.Tensor,
    g: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    table: torch.Tensor,
    groups: Sequence[dict],
    *,
    steps,
    grad_scale: float = 1.0,
    lr_tensor: Optional[torch.Tensor] = None,
    p_bf16: Optional[torch.Tensor] = None,
) -> None:
    """One Adam/AdamW step of every param group in ONE launch, for groups that interleave
    in the arena.  ``p``, ``g``, ``m``, ``v`` (and ``p_bf16``) are whole arena-shaped
    buffers, ``table`` is :func:`build_group_table`'s, ``groups[i]`` holds group ``i``'s
    ``lr``, ``betas``, ``eps``, ``weight_decay``, ``adamw``, ``maximize``.

    ``steps``: the 1-based step number of each group AFTER this update, a list of ints or
    a device int64 ``[G]`` tensor; ``lr_tensor``: a device fp32 ``[G]`` tensor that
    overrides the groups' ``lr`` (graph replay).  Elements that no table row covers are
    neither read nor written.  Alignment contract as :func:`fused_adam_`.  On the CPU (or
    with ``RLA_DISABLE_NATIVE=1``) :func:`fused_adam_` runs over each row's slice."""
    G = _check_groups(groups)
    step_t, host_steps = _group_steps(steps, G)
    if use_native(p):
        require().adam_groups_step(
            p, g, m, v, p_bf16, table, _table_host(table),
            [float(h["lr"]) for h in groups], [float(h["betas"][0]) for h in groups],
            [float(h["betas"][1]) for h in groups], [float(h["eps"]) for h in groups],
            [float(h["weight_decay"]) for h in groups], [bool(h.get("adamw", False)) for h in groups],
            [bool(h.get("maximize", False)) for h in groups], float(grad_scale), step_t, host_steps, lr_tensor,
        )
        return
    ts = [int(s) for s in step_t.tolist()] if step_t is not None else host_steps
    lrs = [float(x) for x in lr_tensor.tolist()] if lr_tensor is not None else [float(h["lr"]) for h in groups]
    for off, cnt, grp in _reference_rows(table, G, p.numel()):
        h = groups[grp]
        s = slice(off, off + cnt)
        fused_adam_(p[s], g[s], m[s], v[s], lr=lrs[grp], betas=tuple(h["betas"]), eps=h["eps"],
                    weight_decay=h["weight_decay"], grad_scale=grad_scale, adamw=bool(h.get("adamw", False)),
                    maximize=bool(h.get("maximize", False)), step=ts[grp],
                    p_bf16=p_bf16[s] if p_bf16 is not None else None)


def fused_sgd_groups_(
    p: torch.Tensor,
    g: torch.Tensor,
    buf: Optional[torch.Tensor],
    table: torch.Tensor,
    groups: Sequence[dict],
    *,
    steps,
    grad_scale: float = 1.0,
    lr_tensor: Optional[torch.Tensor] = None,
    p_bf16: Optional[torch.Tensor] = None,
) -> None:
    """One SGD step of every param group in ONE launch (see :func:`fused_adam_groups_`).
    ``groups[i]``: ``lr``, ``momentum``, ``dampening``, ``weight_decay``, ``nesterov``,
    ``maximize``.  ``buf`` is one arena-shaped velocity buffer (``None`` when no group has
    momentum); under a group with ``momentum == 0`` it is neither read nor written."""
    G = _check_groups(groups)
    step_t, host_steps = _group_steps(steps, G)
    if use_native(p):
        require().sgd_groups_step(
            p, g, buf, p_bf16, table, _table_host(table),
            [float(h["lr"]) for h in groups], [float(h.get("momentum", 0.0)) for h in groups],
            [float(h.get("dampening", 0.0)) for h in groups], [float(h.get("weight_decay", 0.0)) for h in groups],
            [bool(h.get("nesterov", False)) for h in groups], [bool(h.get("maximize", False)) for h in groups],
            float(grad_scale), step_t, host_steps, lr_tensor,
        )
        return
    ts = [int(s) for s in step_t.tolist()] if step_t is not None else host_steps
    lrs = [float(x) for x in lr_tensor.tolist()] if lr_tensor is not None else [float(h["lr"]) for h in groups]
    for off, cnt, grp in _reference_rows(table, G, p.numel()):
        h = groups[grp]
        s = slice(off, off + cnt)
        mom = float(h.get("momentum", 0.0))
        fused_sgd_(p[s], g[s], buf[s] if mom != 0 else None, lr=lrs[grp], momentum=mom,
                   dampening=float(h.get("dampening", 0.0)), weight_decay=float(h.get("weight_decay", 0.0)),
                   nesterov=bool(h.get("nesterov", False)), maximize=bool(h.get("maximize", False)),
                   grad_scale=grad_scale, step=ts[grp], p_bf16=p_bf16[s] if p_bf16 is not None else None)


_DT = {torch.float32: 0, torch.bfloat16: 1}
CHUNK_ELEMS = 16384


def build_copy_table(pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]], device=None,
                     staging: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Chunk table for :func:`multi_copy`: one row per <=16K-element chunk.

    ``pairs`` are (src, dst) tensors of equal numel (fp32 or bf16, contiguous).
    The table is built once per bucket layout and reused every step.
    """
    rows: List[List[int]] = []
    for src, dst in pairs:
        assert src.numel() == dst.numel(), "copy pair size mismatch"
        assert src.is_contiguous() and dst.is_contiguous()
        sd, dd = _DT[src.dtype], _DT[dst.dtype]
        ss, ds = src.element_size(), dst.element_size()
        n = src.numel()
        for off in range(0, n, CHUNK_ELEMS):
            cnt = min(CHUNK_ELEMS, n - off)
            rows.append([src.data_ptr() + off * ss, dst.data_ptr() + off * ds, cnt, sd | (dd << 8)])
    dev = torch.device(device if device is not None else (pairs[0][0].device if pairs else "cpu"))
    host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    if dev.type != "cuda":
        return host
    if staging is not None:
        # inside a hipGraph capture (no pinned allocation allowed there): a pinned
        # buffer reserved beforehand, which the captured copy node re-reads each replay
        if staging.numel() < host.numel():
            raise RuntimeError("graph staging buffer too small for the copy table")
        st = staging[: host.numel()].view(-1, 4)
        st.copy_(host)
        return st.to(dev, non_blocking=True)
    # pinned staging + async copy: a pageable H2D copy would block the host until
    # the stream drains (one such sync per step cost ResNet-50 ~0.5 ms of GPU idle).
    # The staging buffer lives as long as the table: inside a hipGraph capture the
    # copy becomes a graph node that re-reads it at every replay.
    pinned = host.pin_memory()
    table = pinned.to(dev, non_blocking=True)
    table._rla_pinned = pinned
    return table


def multi_copy(
    pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]],
    scale: float = 1.0,
    accumulate: bool = False,
    table: Optional[torch.Tensor] = None,
) -> None:
    """dst (+)= src * scale for every pair, casting fp32<->bf16, in ONE launch on GPU.

    No alignment requirement: each chunk takes the float4 path only when both of its
    addresses are 16-byte aligned fp32, and an element-wise path otherwise.
    """
    if not pairs:
        return
    if use_native(pairs[0][0]):
        if table is None:
            table = build_copy_table(pairs)
        require().multi_copy(table, float(scale), bool(accumulate))
        return
    with torch.no_grad():
        for src, dst in pairs:
            val = src.float() * scale
            if accumulate:
                val = val + dst.float()
            dst.copy_(val.view_as(dst))


def scale_(x: torch.Tensor, s: float) -> None:
    """x *= s in place.  GPU: ``x`` must start on a 16-byte boundary (float4 accesses; a view
    at a multiple of 4 elements of an arena does), else ``RuntimeError``."""
    if use_native(x):
        require().scale_(x, float(s))
    else:
        x.mul_(s)


def sumsq(x: torch.Tensor) -> torch.Tensor:
    """sum(x^2) as a one-element tensor.  GPU: the same 16-byte contract as :func:`scale_`."""
    if use_native(x):
        return require().sumsq(x)
    return (x.float() * x.float()).sum().reshape(1)


CLIP_THREADS = 256  # csrc/optim_kernels.hip kOptThreads
CLIP_MAX_BLOCKS = 64  # csrc/kernels.h kClipMaxBlocks


def clip_slices(n: int, nblk: int) -> List[Tuple[int, int]]:
    """Element range ``[lo, hi)`` of each of ``clip_partials``' ``nblk`` blocks: the
    ``n // 4`` 16-byte quads in contiguous runs of ``ceil(quads / nblk)``, the ``n % 4``
    scalar tail with the last block; blocks past the data get an empty range."""
    n4 = n // 4
    per = -(-n4 // nblk)
    out = []
    for b in range(nblk):
        q0 = min(b * per, n4)
        q1 = min(q0 + per, n4)
        # the last block's quads always end at n4 (nblk * per >= n4): its range runs on into the tail
        out.append((4 * q0, n if b == nblk - 1 else 4 * q1))
    return out


def clip_partials(x: torch.Tensor, nblk: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-block sums of squares of a flat fp32 arena, ``[nblk]``, in a FIXED order:
    the same input gives the same bits on every call (``sumsq`` adds with float
    atomics).  The fused MNIST step's gradient clipping sums them in index order.

    ``1 <= nblk <= 64``; block ``b`` covers ``clip_slices(n, nblk)[b]``.  GPU: ``x``
    must start on a 16-byte boundary (float4 loads; the ``n % 4`` tail is scalar), else
    ``RuntimeError`` before a launch.  CPU: the kernel's summation order in torch fp32
    -- per thread the quads ``q0 + tid, + 256, ...`` into one accumulator per component,
    the tail element, ``(a0 + a1) + (a2 + a3)``, an xor butterfly over the 64 lanes, the
    four waves in order."""
    nblk = int(nblk)
    if not 1 <= nblk <= CLIP_MAX_BLOCKS:
        raise ValueError(f"clip_partials: nblk must be in [1, {CLIP_MAX_BLOCKS}], got {nblk}")
    if out is not None and (out.numel() != nblk or out.dtype != torch.float32 or out.device != x.device):
        raise ValueError(f"clip_partials: out must be {nblk} fp32 elements on {x.device}")
    if use_native(x):
        return require().clip_partials(x, nblk, out)
    with torch.no_grad():
        flat = x.detach().reshape(-1).float()
        n = flat.numel()
        n4 = n // 4
        per = -(-n4 // nblk)
        iters = -(-per // CLIP_THREADS)
        sq = torch.zeros(nblk, iters * CLIP_THREADS * 4)
        for b in range(nblk):
            q0 = min(b * per, n4)
            q1 = min(q0 + per, n4)
            seg = flat[4 * q0:4 * q1]
            sq[b, : seg.numel()] = seg * seg
        sq = sq.view(nblk, iters, CLIP_THREADS, 4)
        acc = torch.zeros(nblk, CLIP_THREADS, 4)
        for it in range(iters):
            acc += sq[:, it]  # the padding adds +0: exact
        tail = flat[4 * n4:]
        acc[nblk - 1, : tail.numel(), 0] += tail * tail
        a = ((acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])).view(nblk, CLIP_THREADS // 64, 64)
        lanes = torch.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            a = a + a[..., lanes ^ off]
        part = a[:, 0, 0].clone()
        for w in range(1, CLIP_THREADS // 64):
            part += a[:, w, 0]
    if out is not None:
        out.copy_(part)
        return out
    return part.to(x.device)


def iter_chunks(n: int, chunk: int) -> Iterable[Tuple[int, int]]:
    for off in range(0, n, chunk):
        yield off, min(chunk, n - off)
