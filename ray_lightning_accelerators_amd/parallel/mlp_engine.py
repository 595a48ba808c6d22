"""Data-parallel training engine for the MNIST classifier on the fused HIP step.

This is the worker-side hot loop that ``RayAccelerator`` / ``HorovodRayAccelerator``
run for ``MNISTClassifier`` (SURVEY.md §3.5 "one training step"; reference
``ray_lightning/tests/utils.py`` / ``examples/ray_ddp_example.py`` model),
re-designed for MI355X instead of translating PL's DDP loop:

* the dataset is resident in HBM as uint8 (MNIST is uint8; ToTensor's /255 and an
  optional single-channel ``Normalize(mean, std)`` are one FMA in the kernels' u8 -> bf16
  conversion: ``set_data`` / ``attach_dataset(normalize=(mean, std))``), and each rank's
  DistributedSampler shard for the current AND the next epoch is an index list on the
  device, so a step needs NO host->device copy and no host sync at epoch boundaries;
* parameters, gradients and Adam state are flat fp32 arenas; the whole model's
  gradient is ONE allreduce bucket (27,882 floats = 109 KiB at the default
  32/64 config -- far below the ~1 MiB where splitting pays on 7 xGMI links);
* world size 1: ONE launch per step for B <= 32 (csrc/mlp_step3.hip kind Step1:
  every block replays the serial head chain on its own CU, then does its tail
  share), else TWO (head + 49-workgroup tail; Adam fused into both, the next
  step's layer 1 computed by the tail);
  world size > 1: with a ``dp_context`` the same launches, each block exchanging
  its gradient values with the peers over xGMI inside its Adam epilogue (kinds
  Step1DP / StepDP); otherwise head -> tail(grad) -> allreduce(SUM) ->
  tail(adam), the 1/world average folded into ``grad_scale``;
* ``clip_norm`` (global-norm gradient clipping, ``torch.nn.utils.clip_grad_norm_``):
  at every batch and world size head -> tail(grad) -> [allreduce] -> norm partials
  (``ops.optim.clip_partials``, fixed summation order) -> tail(adam), which derives
  the coefficient on the device -- no host sync, bitwise-reproducible, graph-capturable;
* ``accumulate=K`` (gradient accumulation, ``Trainer(accumulate_grad_batches=K)``): a
  window of K micro-batches ends in one optimizer step.  A micro-batch inside its window is
  TWO launches, head -> tail(acc) (gradients added into ``grads``, no Adam, the next
  batch's layer 1 from the unchanged weights); the one that closes it is head ->
  tail(grad, adding) -> [allreduce] -> [norm partials] -> tail(adam, grad_scale 1/(world K)).
  The window position is a function of ``step_in_epoch``, ``n_batches`` and K alone (no
  device read); the epoch's last window may be short and is still weighted 1/K;
* ``optimizer="adamw"`` is Adam's kernels with the decoupled decay on every route;
  ``optimizer="sgd"`` (``momentum`` / ``dampening`` / ``nesterov``, ``torch.optim.SGD``) is
  applied by SGD instances of the tail kernel: head -> tail at world size 1, else (and
  under ``clip_norm`` / ``accumulate``) head -> tail(grad | acc) -> [allreduce] -> [norm
  partials] -> tail(sgd); never one launch, never ``dp_context``;
* ``begin_epoch(..., last_rows=r)``: the epoch's last batch holds ``r <= B`` rows (the short
  last batch of a ``drop_last=False`` loader).  The two-launch kernels and PRIME decide from
  the device cursor which batch that is; every route that is two or more launches just passes
  ``last_rows``.  A one-launch engine runs the two steps that touch the short batch --
  position ``n_batches - 2`` gathers it, ``n_batches - 1`` consumes it -- as head + tail,
  eagerly (its captured graphs hold one-launch steps and stop before them).  With a
  ``dp_context`` the short batch is dropped, with one warning;
* the step's device work can be captured into a hipGraph (``capture``): batch
  cursor, step counter, ring slot and epoch buffer live on the device, so
  replays advance by themselves.

On a CPU device the same engine runs the fp32 PyTorch reference step (the
oracle of the GPU tests) with identical batch order and optimizer semantics.
"""
from __future__ import annotations

import logging
import math
import os
from typing import Callable, Dict, Optional, Sequence

import torch
import torch.distributed as dist

from ..config import get_config
from ..ops import fused_mlp
from ..ops.optim import clip_partials, fused_adam_, fused_sgd_

log = logging.getLogger(__name__)


class FusedStepNumericsError(RuntimeError):
    """The fused MNIST step's layer-1 sum left its 12.20 fixed-point range or met a
    NaN / Inf: the step is no longer the computation that was asked for."""

    def __init__(self, saturated: int, nonfinite: int, last_step: int):
        super().__init__(self.describe(saturated, nonfinite, last_step))
        self.saturated, self.nonfinite, self.last_step = int(saturated), int(nonfinite), int(last_step)

    @staticmethod
    def describe(saturated: int, nonfinite: int, last_step: int) -> str:
        return (f"fused MLP step: {int(saturated)} layer-1 tile partial(s) saturated the 12.20 fixed point "
                f"(|partial| > 32, clamped) and {int(nonfinite)} were NaN / Inf (stored as +-32, so the "
                f"reported loss stays finite); last affected optimizer step {int(last_step)}. "
                "Remedies: Trainer(fused_step=False) (fp32 autograd path), a lower learning rate, or "
                "RLA_MLP_SATURATION=warn to keep training with a warning.")


# blocks of the clipped step's norm launch: 32 x 256 threads cover the default arena's
# 6,970 quads in one pass, and the ADAM tail's scalar lane sums 32 partials
CLIP_NBLK = 32
_CLIP_HEALTH0 = {"clip_norm_last": None, "clip_coef_last": None, "clipped_steps": 0, "nonfinite_norm_steps": 0}


def shard_indices(n: int, world: int, rank: int, epoch: int, seed: int, shuffle: bool,
                  device=None) -> torch.Tensor:
    """torch.utils.data.DistributedSampler's index set for (rank, epoch)."""
    if shuffle:
        g = torch.Generator().manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g)
    else:
        idx = torch.arange(n)
    total = int(math.ceil(n / world)) * world
    if total > n:
        idx = torch.cat([idx, idx[: total - n]])
    out = idx[rank:total:world]
    return out.to(device) if device is not None else out


class FusedMLPEngine:
    def __init__(
        self,
        layer_1: int,
        layer_2: int,
        batch_size: int,
        lr: float = 1e-3,
        betas=(0.9, 0.999),
        eps: float = 1e-8,
        weight_decay: float = 0.0,
        device: Optional[torch.device] = None,
        world_size: int = 1,
        rank: int = 0,
        allreduce: Optional[Callable[[torch.Tensor], None]] = None,
        init_params: Optional[torch.Tensor] = None,
        stats_ring: int = 1024,
        seed: int = 0,
        buffers: Optional[Dict[str, torch.Tensor]] = None,
        dp_context: Optional[Sequence[int]] = None,
        dp_proto: Optional[str] = None,
        dp_rearm: Optional[Callable[[], None]] = None,
        dp_loop: bool = False,
        clip_norm: Optional[float] = None,
        accumulate: int = 1,
        optimizer: str = "adam",
        momentum: float = 0.0,
        dampening: float = 0.0,
        nesterov: bool = False,
        lr_ring: int = 0,
    ):
        """``buffers``: optional external fp32 tensors ``params`` / ``grads`` /
        ``exp_avg`` / ``exp_avg_sq`` (e.g. views of a Trainer's parameter arena,
        so the nn.Module parameters stay the engine's master weights).
        ``dp_context``: ``NativeCommunicator.dp_context(...)`` -- world size > 1
        then runs the fused data-parallel step (the tail kernel exchanges its
        gradient tiles with the peers over xGMI inside the Adam epilogue: two
        launches per step, no separate allreduce).  ``dp_proto``: the one-launch
        step's exchange -- "packed" (one-shot, default), "owner" (reduce-scatter to
        the task's owner, Adam there, all-gather of the weights) or "granule" (round
        2); unset: ``RLA_DP_PROTO``.  ``dp_rearm``: collective reset of the exchange
        region (``NativeCommunicator.dp_rearm``), run before a protocol is first used.
        ``dp_loop``: loopback diagnostic (``dp_context`` of one process whose regions
        all point at its own; see scripts/dp_overhead_probe.py).
        ``clip_norm``: clip the (world-averaged) gradient to this global L2 norm before
        Adam, as ``torch.nn.utils.clip_grad_norm_`` does; None / 0: no clipping.  The step
        then always runs head -> tail(grad) -> [allreduce] -> norm partials -> tail(adam);
        it does not combine with ``dp_context`` (the in-kernel exchange never holds the
        whole averaged gradient before its Adam).
        ``accumulate``: micro-batches per optimizer step (K >= 1; 1: the engine without the
        argument).  Micro-batch i of an epoch closes its window when (i + 1) % K == 0 or it
        is the epoch's last; every micro-batch's gradient weighs 1 / K, clipping applies to
        the averaged sum, the allreduce runs once per window, ``counters[0]`` advances once
        per window while cursor / ring slot / stats rows advance per micro-batch.  Like
        ``clip_norm`` it never runs as one launch and does not combine with ``dp_context``.
        ``optimizer``: "adam" (default), "adamw" (decoupled ``weight_decay``; every route,
        the one-launch step and the in-kernel exchange included) or "sgd" --
        ``torch.optim.SGD`` with ``momentum`` / ``dampening`` / ``nesterov`` applied by the
        tail kernel.  SGD never runs as one launch and does not combine with ``dp_context``:
        world size 1 without clipping or accumulation is head -> tail (two launches), every
        other combination head -> tail(grad | acc) -> [allreduce] -> [norm partials] ->
        tail(sgd).  Its velocity is ``momentum_buffer`` (``buffers["momentum_buffer"]`` when
        external); ``exp_avg`` aliases it and ``exp_avg_sq`` is None.
        ``lr_ring``: 0 (default): the learning rate is one device scalar, rewritten by
        ``set_lr``.  A power of two >= 2 puts the engine in ring mode for its lifetime (graphs
        bake the mask): ``lr_tensor`` holds that many rates and the launch that applies
        optimizer step ``t`` reads entry ``(t - 1) & (lr_ring - 1)``, so ``set_lr_schedule``
        hands a captured graph a different rate at every step without a host write in between.
        A step without a scheduled rate runs at ``lr``, as outside ring mode.  The one-launch
        step runs its schedule instances; the one-launch in-kernel exchange has none, so a
        ``dp_context`` engine then steps as two launches (one warning)."""
        if isinstance(lr_ring, bool) or int(lr_ring) != lr_ring or int(lr_ring) < 0 or int(lr_ring) == 1 \
                or int(lr_ring) & (int(lr_ring) - 1):
            raise ValueError(f"lr_ring must be 0 or a power of two >= 2, got {lr_ring!r}")
        lr_ring = int(lr_ring)
        if optimizer not in ("adam", "adamw", "sgd"):
            raise ValueError(f"optimizer must be 'adam', 'adamw' or 'sgd', got {optimizer!r}")
        momentum, dampening, nesterov = float(momentum), float(dampening), bool(nesterov)
        if optimizer == "sgd":
            if not momentum >= 0.0:
                raise ValueError(f"momentum must be >= 0, got {momentum}")
            if nesterov and (momentum <= 0.0 or dampening != 0.0):
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")
            if dp_context is not None:
                raise ValueError("optimizer='sgd' needs the allreduce route: the in-kernel data-parallel exchange "
                                 "(dp_context) applies Adam -- pass allreduce= and no dp_context")
        elif momentum != 0.0 or dampening != 0.0 or nesterov:
            raise ValueError(f"momentum / dampening / nesterov belong to optimizer='sgd', not {optimizer!r}")
        if isinstance(accumulate, bool) or int(accumulate) != accumulate or int(accumulate) < 1:
            raise ValueError(f"accumulate must be an integer >= 1, got {accumulate!r}")
        accumulate = int(accumulate)
        if accumulate > 1 and dp_context is not None:
            raise ValueError("accumulate > 1 needs the allreduce route: the in-kernel data-parallel exchange "
                             "(dp_context) steps at every batch -- pass allreduce= and no dp_context")
        clip_norm = float(clip_norm) if clip_norm else None
        if clip_norm is not None and not clip_norm > 0.0:
            raise ValueError(f"clip_norm must be positive, got {clip_norm}")
        if clip_norm is not None and dp_context is not None:
            raise ValueError("clip_norm needs the allreduce route: the in-kernel data-parallel exchange "
                             "(dp_context) cannot clip -- pass allreduce= and no dp_context")
        if not fused_mlp.mlp_supported(layer_1, layer_2):
            raise ValueError(f"no fused kernel for layer sizes {layer_1}/{layer_2}")
        if not 1 <= batch_size <= 256:
            raise ValueError("fused MLP engine supports batch sizes 1..256")
        self.L1, self.L2, self.B = int(layer_1), int(layer_2), int(batch_size)
        self.lr, self.betas, self.eps, self.wd = float(lr), tuple(betas), float(eps), float(weight_decay)
        self.optimizer = optimizer
        self.sgd = optimizer == "sgd"
        self.adamw = optimizer == "adamw"
        self.momentum, self.dampening, self.nesterov = momentum, dampening, nesterov
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.native = self.device.type == "cuda"
        self.world_size, self.rank = int(world_size), int(rank)
        self.allreduce = allreduce
        self.dp_ctx = None
        self.dp_loop = bool(dp_loop)
        if dp_context is not None and (self.world_size > 1 or self.dp_loop) and self.device.type == "cuda":
            ctx = [int(v) for v in dp_context]
            if not self.dp_loop and (ctx[0] != self.world_size or ctx[1] != self.rank):
                raise ValueError("dp_context belongs to a different (world, rank)")
            self.dp_ctx = ctx
        self._dp_rearm = dp_rearm
        self._owner_masks = None
        n = fused_mlp.mlp_param_count(self.L1, self.L2)
        if buffers is not None:
            names = ("params", "grads", "momentum_buffer") if self.sgd else ("params", "grads", "exp_avg", "exp_avg_sq")
            for k in names:
                t = buffers[k]
                assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.device == self.device, k
                setattr(self, "exp_avg" if k == "momentum_buffer" else k, t)
            if self.sgd:
                self.exp_avg_sq = None
        else:
            if init_params is None:
                init_params = fused_mlp.init_mlp_params(self.L1, self.L2, torch.Generator().manual_seed(seed))
            self.params = init_params.detach().to(self.device, torch.float32).contiguous().clone()
            # padded to 4 floats: the xGMI one-shot allreduce moves 16-byte vectors
            self._grads_padded = torch.zeros((n + 3) // 4 * 4, device=self.device)
            self.grads = self._grads_padded[:n]
            self.exp_avg = torch.zeros(n, device=self.device)  # SGD: the velocity (momentum_buffer)
            self.exp_avg_sq = None if self.sgd else torch.zeros(n, device=self.device)
        self.lr_ring, self.lr_mask = lr_ring, max(lr_ring - 1, 0)
        self.lr_tensor = torch.full((max(lr_ring, 1),), self.lr, device=self.device)
        # ring mode, host side: what each entry will hold once the stream reaches the next
        # launch; the value every entry holds (None: they differ); the last optimizer step
        # with a scheduled rate; pinned staging buffers with the event of their last copy
        self._ring_host = [self.lr] * lr_ring
        self._ring_uniform: Optional[float] = self.lr
        self._sched_end = 0
        self._lr_stage: list = []
        self.clip_norm = clip_norm
        self.accumulate = accumulate
        # the one-block head's stats row of the current micro-batch (accumulation: the tail
        # moves it to the row counters[MLP3_ROW_WORD] names, one ring row per micro-batch)
        self._head_row = torch.zeros(1, 4, device=self.device)
        self.optimizer_steps = 0  # host count of optimizer steps == counters[0]
        self.clip_part = self.clip_out = None
        if clip_norm is not None:
            self.clip_part = torch.zeros(CLIP_NBLK, device=self.device)
            # [0] norm, [1] coefficient of the last step, [2] steps clipped, [3] steps with a NaN / Inf norm
            self.clip_out = torch.zeros(4, device=self.device)
        self._clip_last = dict(_CLIP_HEALTH0)
        self._clip_since = 0  # global_step when clip_out was last zeroed
        lay = fused_mlp.mlp_shadow_layout(self.L1, self.L2)
        self.shadow = torch.zeros(lay["total"], dtype=torch.bfloat16, device=self.device)
        bufs = fused_mlp.mlp3_buffers(self.L1, self.L2, self.B, self.device)
        # counters: [0] optimizer step, [1] next batch cursor, [2] last consumed cursor,
        # [3] H1pre/X ring slot, [4] epoch buffer of `order` that [1] indexes
        self.counters = bufs["counters"]
        self.dh1t, self.xring, self.h1pre, self.act = bufs["dh1t"], bufs["xring"], bufs["h1pre"], bufs["act"]
        self.yring = bufs["yring"]
        self.head_part = bufs["head_part"]
        self.hand = bufs["hand"]
        # word indices of `hand`; err, sat, nonfinite, last_step are adjacent (one copy reads them)
        self._hl = fused_mlp.mlp3_hand_layout(native=self.native)
        assert [self._hl[k] - self._hl["err"] for k in ("sat", "nonfinite", "last_step")] == [1, 2, 3]
        self.saturation_policy: Optional[str] = None  # None: RLAConfig.mlp_saturation at each check
        self._health_reported = (0, 0)  # counts the warn policy has already logged
        self._health_last = {"saturated": 0, "nonfinite": 0, "last_step": 0, "timed_out": False}
        self._hand_probe = None
        # world size 1, B <= 32: the whole step as ONE launch at every width
        # (RLA_MLP_ONE_LAUNCH=0: head + tail).  Round 5 gated widths > 64 off after
        # intermittent fidelity failures in long GPU sessions; round 6's post-mortem
        # showed the step bitwise equal to the two-launch step from a fresh engine in
        # the failing session (docs/one_launch_investigation.md), so the gate is gone.
        # clipping needs the whole gradient between two launches: never one launch;
        # nor does accumulation (Adam only at a window's close), nor SGD (the one-launch
        # kernel applies Adam)
        self.one_launch = (self.B <= fused_mlp.ONE_LAUNCH_MAX_B and os.environ.get("RLA_MLP_ONE_LAUNCH") != "0"
                           and clip_norm is None and accumulate == 1 and not self.sgd)
        # the dataset's Normalize(mean, std) or None, and the kernels' pixel map derived from it
        self.normalize = None
        self.x_scale, self.x_shift = fused_mlp.input_affine(None)
        # world size > 1 with the xGMI context: the same one launch, each block
        # exchanging its values with the peers (protocol: self.dp_proto)
        self.dp_proto = "packed"
        self.one_launch_dp = False
        # (collective with a rearm callable: every rank builds its engine together)
        self.set_dp_proto(dp_proto or os.environ.get("RLA_DP_PROTO") or "packed", rearm=True)
        if self.lr_mask and self.one_launch and self.dp_ctx is not None and not self.one_launch_dp:
            log.warning("fused MLP step: a learning-rate ring (lr_ring=%d) takes the data-parallel exchange out of "
                        "the one-launch step (its schedule instances exist at world size 1 only): every step runs "
                        "as two launches, head + tail with the in-kernel exchange", self.lr_ring)
        self.stats = torch.zeros(stats_ring, 4, device=self.device)
        self.seed = seed
        self.epoch = 0
        self.step_in_epoch = 0
        self.global_step = 0
        self._graph = None
        self._graph_steps = 0
        self._tail_graphs: Dict[int, "torch.cuda.CUDAGraph"] = {}  # remainder sizes (powers of two)
        self._shadow_stale = False
        self._primed = False
        self._host_epochs = False
        self.x_u8 = self.labels = self.order = None
        self.n_batches = 0
        # valid rows of the epoch's last batch (begin_epoch(last_rows=...)); B: every batch is full
        self.last_rows = self.B
        self.refresh_shadow()

    # ------------------------------------------------- exchange protocol
    def set_dp_proto(self, name: str, rearm: bool = True) -> None:
        """Select the one-launch step's exchange protocol ("packed" / "owner" /
        "granule"; "wave" / "all" are two-launch flag protocols).  Collective when
        ``rearm`` (every rank switches together): the region is reset first, because
        a granule left by another protocol could carry a current-looking tag."""
        if name not in fused_mlp.DP_PROTOS and name not in ("wave", "all"):
            raise ValueError(f"unknown data-parallel exchange protocol {name!r}")
        if self.dp_proto == "owner" and name != "owner" and getattr(self, "_stepped_owner", False):
            # leaving owner: non-owners' Adam state is stale -- consolidate first
            self.sync_optimizer_state()
        self._stepped_owner = False
        self.dp_proto = name
        self.one_launch_dp = self._one_launch_dp_ok()
        if rearm and self.dp_ctx is not None and self._dp_rearm is not None:
            self._dp_rearm()
        self._drop_graphs()

    def dp_owner_mask(self, rank: Optional[int] = None) -> torch.Tensor:
        """Bool mask over the parameter arena: the elements whose Adam state this rank
        keeps under the "owner" protocol (mirror of the kernel's dp_task_owner: W1
        tile kt -> task kt; dW2 tile (ct, nt) -> 49 + ct * (L2/16) + nt; dW3 tile nt ->
        49 + (L1/16)(L2/16) + nt; bias chunk of 64 -> after those; owner = task % N)."""
        rank = self.rank if rank is None else int(rank)
        world = self.dp_ctx[0] if self.dp_ctx is not None else self.world_size
        L1, L2 = self.L1, self.L2
        tn1, tn2 = L1 // 16, L2 // 16
        tiles = 784 // 16
        w1 = (torch.arange(784) // 16).repeat(L1)  # [L1 rows][784 pixels], row-major
        nb = L1 + L2 + 10
        w2 = tiles + (torch.arange(L1) // 16).repeat(L2) * tn2 + (torch.arange(L2) // 16).repeat_interleave(L1)
        w3 = tiles + tn1 * tn2 + (torch.arange(L2) // 16).repeat(10)
        bias = tiles + tn1 * tn2 + tn2 + torch.arange(nb) // 64
        b1, b2, b3 = bias[:L1], bias[L1:L1 + L2], bias[L1 + L2:]
        task = torch.cat([w1, b1, w2, b2, w3, b3])  # arena order: W1 B1 W2 B2 W3 B3
        assert task.numel() == fused_mlp.mlp_param_count(L1, L2)
        return (task % world) == rank

    @property
    def momentum_buffer(self) -> Optional[torch.Tensor]:
        """SGD's velocity (torch's ``momentum_buffer``, the arena behind ``exp_avg``); None
        for the Adam engines."""
        return self.exp_avg if self.sgd else None

    def sync_optimizer_state(self) -> None:
        """Owner protocol: every rank's Adam state becomes the owners' (each element's
        current m / v live only on its task's owner) -- a masked SUM allreduce, exact
        (one nonzero term).  Collective; run before anything reads exp_avg /
        exp_avg_sq (checkpoints, optimizer_state_dict, a protocol switch)."""
        if not (self.native and self.one_launch_dp and self.dp_proto == "owner" and self.world_size > 1):
            return
        if self.dp_loop:
            return  # loopback: one process holds every "rank's" state
        if self.allreduce is None:
            raise RuntimeError("owner protocol: sync_optimizer_state needs the engine's allreduce")
        if self._owner_masks is None:
            self._owner_masks = self.dp_owner_mask().to(self.device, torch.float32)
        for t in (self.exp_avg, self.exp_avg_sq):
            t.mul_(self._owner_masks)
            self.allreduce(t)

    def _publish_counters(self) -> None:
        """Host edits of the device state go to both copies (current / advanced)."""
        self.counters[5:10].copy_(self.counters[0:5])

    def check(self, blocking: bool = True) -> None:
        """Raise if a one-launch step's in-launch hand-off ever timed out (a block
        polled past its bound: the step it belongs to is not trustworthy), then report
        the kernels' saturation / non-finite counts as ``RLAConfig.mlp_saturation``
        says (``warn`` / ``raise`` / ``ignore``; ``health`` has the counts).
        ``blocking=False`` (the Trainer's epoch ends): the words are copied to pinned
        host memory asynchronously and the copy made at the PREVIOUS call is the one
        checked -- no device sync at an epoch boundary, detection one epoch late; a
        blocking call at the end of the fit reads the current values."""
        if not self.native:
            return
        lo, hi = self._hl["err"], self._hl["last_step"] + 1
        prev = getattr(self, "_hand_probe", None)
        if prev is not None:
            buf, ev = prev
            ev.synchronize()  # enqueued one epoch ago: long complete
            self._hand_probe = None
            self._apply_health(buf.tolist())
        if blocking:
            self._apply_health(self.hand[lo:hi].tolist())
            return
        buf = getattr(self, "_hand_pin", None)
        if buf is None:
            buf = self._hand_pin = torch.zeros(hi - lo, dtype=self.hand.dtype, pin_memory=True)
        buf.copy_(self.hand[lo:hi], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hand_probe = (buf, ev)

    def _health_dict(self, words) -> Dict[str, object]:
        """``hand[err : last_step + 1]`` as the dict ``health`` returns."""
        o = self._hl["err"]
        return {"saturated": int(words[self._hl["sat"] - o]), "nonfinite": int(words[self._hl["nonfinite"] - o]),
                "last_step": int(words[self._hl["last_step"] - o]), "timed_out": int(words[0]) != 0}

    def _apply_health(self, words) -> None:
        """One reading of the error / health words: the time-out always raises, the
        counts go through the saturation policy."""
        h = self._health_last = self._health_dict(words)
        if h["timed_out"]:
            raise RuntimeError("fused MLP one-launch step: an in-launch hand-off timed out")
        sat, bad = h["saturated"], h["nonfinite"]
        policy = self.saturation_policy or get_config().mlp_saturation
        if policy == "ignore" or (sat == 0 and bad == 0):
            return
        if policy == "raise":
            raise FusedStepNumericsError(sat, bad, h["last_step"])
        seen = self._health_reported
        if sat > seen[0] or bad > seen[1]:  # one warning per check that sees a count grow
            self._health_reported = (sat, bad)
            log.warning(FusedStepNumericsError.describe(sat, bad, h["last_step"]))

    def health(self, blocking: bool = True) -> Dict[str, object]:
        """What the step kernels counted since the engine was built (or ``reset_health``):
        ``saturated`` -- layer-1 tile partials beyond +-32 that the 12.20 fixed point
        replaced by the clamp; ``nonfinite`` -- NaN / Inf partials (which the conversion
        turns into a finite +-32, so the loss stays finite); ``last_step`` -- the latest
        optimizer step whose launch counted one (0: none, or the priming before step 1);
        ``timed_out`` -- the hand-off error word.  Exact device-side counts: they include
        graph replays.  ``blocking=False``: the last reading a ``check`` made, no sync.
        The CPU reference engine sums in fp32: all zeros."""
        if not self.native:
            return {"saturated": 0, "nonfinite": 0, "last_step": 0, "timed_out": False, **self._clip_health(True)}
        if not blocking:
            return {**self._health_last, **self._clip_health(False)}
        self._health_last = self._health_dict(self.hand[self._hl["err"]:self._hl["last_step"] + 1].tolist())
        return {**self._health_last, **self._clip_health(True)}

    def _clip_health(self, blocking: bool) -> Dict[str, object]:
        """The clipped step's report (``clip_out``): ``clip_norm_last`` / ``clip_coef_last``
        -- the last step's gradient norm and coefficient (None before the first step or
        without ``clip_norm``), ``clipped_steps`` -- steps whose coefficient was below 1,
        ``nonfinite_norm_steps`` -- steps whose norm was NaN / Inf (passed through, as
        torch does).  Device-side counts: graph replays included.  ``blocking=False``:
        the last blocking reading.  An engine without ``clip_norm`` reports none of them."""
        if self.clip_out is None:
            return {}
        if blocking:
            norm, coef, clipped, bad = self.clip_out.tolist()
            seen = self.global_step > self._clip_since  # a step ran since the engine was built / reset
            self._clip_last = {"clip_norm_last": norm if seen else None, "clip_coef_last": coef if seen else None,
                               "clipped_steps": int(clipped), "nonfinite_norm_steps": int(bad)}
        return dict(self._clip_last)

    def reset_health(self) -> None:
        """Zero the saturation / non-finite counts and the last affected step
        (stream-ordered; the time-out word stays).  A reading still in flight from
        ``check(blocking=False)`` is dropped: it predates the reset."""
        if self.native:
            self.hand[self._hl["sat"]:self._hl["last_step"] + 1].zero_()
        if self.clip_out is not None:
            self.clip_out.zero_()
        self._clip_last = dict(_CLIP_HEALTH0)
        self._clip_since = self.global_step
        self._hand_probe = None
        self._health_reported = (0, 0)
        self._health_last = {"saturated": 0, "nonfinite": 0, "last_step": 0,
                             "timed_out": bool(self._health_last["timed_out"])}

    def set_step(self, step: int) -> None:
        self.counters[0] = int(step)
        self.optimizer_steps = int(step)
        self._sched_end = 0  # a schedule belongs to the count it was given under
        self._publish_counters()

    @property
    def comm_buffer(self) -> torch.Tensor:
        """The gradient bucket handed to the allreduce (16-byte padded when owned)."""
        return getattr(self, "_grads_padded", self.grads)

    # ------------------------------------------------- host-driven epochs
    def _one_launch_dp_ok(self) -> bool:
        """Whether the in-kernel exchange runs inside the one-launch step.  (A normalised
        dataset: the one-launch kernel has its Normalize instances at world size 1 only, so
        the exchange then runs in the two-launch step's tail.)"""
        ctx, name = self.dp_ctx, self.dp_proto
        need = 2 * fused_mlp.mlp_param_count(self.L1, self.L2) if name == "granule" else fused_mlp.DP_AREA_FLOATS
        return (self.one_launch and ctx is not None and name in fused_mlp.DP_PROTOS and ctx[2] >= need
                and (self.x_scale, self.x_shift) == fused_mlp.input_affine(None)
                and not self.lr_mask)  # nor a schedule instance: a rate ring runs in the two-launch tail

    def _set_normalize(self, normalize) -> None:
        """The dataset's single-channel ``Normalize(mean, std)`` (None: ToTensor alone).  A
        changed pixel map invalidates what was gathered and captured under the old one: the
        graphs (they bake the two scalars) and the primed batch."""
        scale, shift = fused_mlp.input_affine(normalize)
        if (scale, shift) != (self.x_scale, self.x_shift):
            self._drop_graphs()
            self._primed = False
        self.normalize = fused_mlp.normalize_pair(normalize)
        self.x_scale, self.x_shift = scale, shift
        if self.one_launch_dp and self.dp_proto == "owner" and getattr(self, "_stepped_owner", False):
            self.sync_optimizer_state()  # leaving the owner protocol: consolidate the Adam state first
            self._stepped_owner = False
        was = self.one_launch_dp
        self.one_launch_dp = self._one_launch_dp_ok()
        if was and not self.one_launch_dp:
            log.warning("fused MLP step: the dataset's Normalize%s takes the data-parallel exchange out of the "
                        "one-launch step (its Normalize instances exist at world size 1 only): every step now runs "
                        "as two launches, head + tail with the in-kernel exchange", self.normalize)

    def attach_dataset(self, images_u8: torch.Tensor, labels: torch.Tensor, normalize=None) -> None:
        """Trainer mode: the dataset is resident, the host supplies each epoch's order.
        ``normalize``: ``(mean, std)`` of a single-channel ``Normalize`` after ToTensor, folded
        into the kernels' u8 -> bf16 conversion (``ops.fused_mlp.input_affine``)."""
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 2 and images_u8.size(1) == 784
        self._set_normalize(normalize)
        self.x_u8 = images_u8.to(self.device).contiguous()
        self.labels = labels.to(self.device, torch.int64).contiguous()
        self.n_data = self.x_u8.size(0)
        self._host_epochs = True

    def begin_epoch(self, order: torch.Tensor, n_batches: int, checked: bool = False,
                    last_rows: Optional[int] = None) -> None:
        """Load one epoch's sample order and re-prime: ``n_batches * B`` indices, or with
        ``last_rows`` (the short last batch of a ``drop_last=False`` loader, 1 <= last_rows <= B)
        ``(n_batches - 1) * B + last_rows``.  The short batch is one optimizer step (one
        micro-batch under ``accumulate``) whose loss and gradient are the mean over its rows
        and whose stats row counts them.  With the in-kernel exchange (``dp_context``) it is
        dropped, with one warning: that route has no short batch.

        Both order buffers get the same list, so the last step's look-ahead
        gather wraps into valid indices; the next ``begin_epoch`` re-primes."""
        n_batches = int(n_batches)
        last_rows = fused_mlp.check_last_rows(last_rows, self.B, "begin_epoch")
        if last_rows != self.B and self.dp_ctx is not None:
            if not getattr(self, "_short_drop_warned", False):
                self._short_drop_warned = True
                log.warning("fused MLP step: the in-kernel data-parallel exchange (dp_context) has no short batch "
                            "-- its owner protocol shards the Adam state over every step -- so the last batch of "
                            "%d rows (batch size %d) is dropped each epoch; the allreduce route trains on it",
                            last_rows, self.B)
            n_batches, last_rows = n_batches - 1, self.B
        n_real = (n_batches - 1) * self.B + last_rows
        order = order.reshape(-1)[:n_real]
        assert n_batches >= 1 and order.numel() == n_real
        # the kernels trust indices (a host order is checked without a device sync;
        # ``checked``: the caller already did)
        if not checked or order.device.type != "cpu":
            assert int(order.max()) < self.n_data and int(order.min()) >= 0
        if last_rows != self.B:
            # padded to the stride n_batches * B with a valid index (the kernels never read it)
            order = torch.cat([order, order[:1].expand(self.B - last_rows)])
        if (self.order is None or self.order.size(1) != order.numel() or self.n_batches != n_batches
                or self.last_rows != last_rows):
            # the captured graph bakes the order pointer, n_batches and last_rows: only a new
            # shape forces a re-capture, a new epoch of the same shape reuses it
            if self.order is None or self.order.size(1) != order.numel():
                self.order = torch.empty(2, order.numel(), dtype=torch.int64, device=self.device)
            self._drop_graphs()
        self.last_rows = last_rows
        if order.device.type == "cpu" and self.native:
            # staged through a pinned buffer: an async H2D copy instead of a blocking
            # pageable one; the previous epoch's copy must be done before reuse
            if getattr(self, "_order_ev", None) is not None:
                self._order_ev.synchronize()
            pin = getattr(self, "_order_pin", None)
            if pin is None or pin.numel() != order.numel():
                pin = self._order_pin = torch.empty(order.numel(), dtype=torch.int64, pin_memory=True)
            pin.copy_(order)
            self.order[0].copy_(pin, non_blocking=True)
            self._order_ev = torch.cuda.Event()
            self._order_ev.record()
        else:
            self.order[0].copy_(order.to(self.device))
        self.order[1].copy_(self.order[0])
        self.n_batches = int(n_batches)
        self.counters[1:5].zero_()
        self._publish_counters()
        self.step_in_epoch = 0
        self._primed = False

    # ------------------------------------------------------------------ data
    def set_data(self, images_u8: torch.Tensor, labels: torch.Tensor, shuffle: bool = True, normalize=None) -> None:
        """Make the (full) dataset resident on the device; shards are per-rank index lists.
        ``normalize``: as ``attach_dataset``."""
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 2 and images_u8.size(1) == 784
        self._set_normalize(normalize)
        self.x_u8 = images_u8.to(self.device).contiguous()
        self.labels = labels.to(self.device, torch.int64).contiguous()
        self.shuffle = shuffle
        self.n_data = self.x_u8.size(0)
        per_rank = int(math.ceil(self.n_data / self.world_size))
        self.n_batches = per_rank // self.B
        self.last_rows = self.B  # this mode drops the remainder
        if self.n_batches < 1:
            raise ValueError("dataset shard smaller than one batch")
        self.order = torch.empty(2, self.n_batches * self.B, dtype=torch.int64, device=self.device)
        self._fill_order(0)
        self._fill_order(1)
        self.counters[1:5].zero_()
        self._publish_counters()
        self.epoch = 0
        self.step_in_epoch = 0
        self._drop_graphs()
        self._primed = False

    def _fill_order(self, epoch: int) -> None:
        """Write ``epoch``'s shard order into buffer ``epoch % 2`` (stream-ordered)."""
        idx = shard_indices(self.n_data, self.world_size, self.rank, epoch, self.seed, self.shuffle)
        idx = idx[: self.n_batches * self.B]
        assert int(idx.max()) < self.n_data and int(idx.min()) >= 0  # the kernels trust indices
        self.order[epoch % 2].copy_(idx.to(self.device), non_blocking=True)

    # ------------------------------------------------------------ broadcast
    def broadcast_from(self, src: int = 0) -> None:
        if self.world_size > 1 and dist.is_initialized():
            if self.params.is_cuda and dist.get_backend() == "gloo":  # CPU bootstrap group
                tmp = self.params.cpu()
                dist.broadcast(tmp, src)
                self.params.copy_(tmp)
            else:
                dist.broadcast(self.params, src)
        self.refresh_shadow()

    def refresh_shadow(self) -> None:
        """Rebuild the bf16 weight shadows after the fp32 params changed outside a step."""
        fused_mlp.mlp_refresh_shadow(self.params, self.shadow, self.L1, self.L2)
        self._shadow_stale = False
        self._primed = False

    def load_params(self, flat: torch.Tensor) -> None:
        with torch.no_grad():
            self.params.copy_(flat.reshape(-1).to(self.params))
        self.refresh_shadow()

    def set_lr(self, lr: float) -> None:
        """The rate of every step from now on (ring mode: the whole ring, and any schedule is
        forgotten)."""
        self.lr = float(lr)
        self.lr_tensor.fill_(self.lr)
        if self.lr_mask:
            self._ring_host = [self.lr] * self.lr_ring
            self._ring_uniform = self.lr
            self._sched_end = 0

    # ------------------------------------------------------------- LR ring
    def set_lr_schedule(self, rates: Sequence[float]) -> None:
        """Ring mode: ``rates[i]`` is the learning rate of optimizer step
        ``optimizer_steps + 1 + i`` (at most ``lr_ring`` of them; an earlier schedule is
        replaced).  The values travel in stream order with the launches -- steps already
        dispatched keep their rates, no host sync -- and are rounded to fp32 as
        ``set_lr`` rounds, so a scheduled run equals a ``set_lr``-per-step run bit for bit.
        Steps past the schedule run at ``lr``."""
        if not self.lr_mask:
            raise RuntimeError("set_lr_schedule needs ring mode: build the engine with lr_ring=<power of two>")
        rates = [float(r) for r in rates]
        if len(rates) > self.lr_ring:
            raise ValueError(f"set_lr_schedule: {len(rates)} rates do not fit a ring of {self.lr_ring}")
        self._sched_end = 0
        if rates:
            self._ring_write(self.optimizer_steps + 1, rates)
            self._sched_end = self.optimizer_steps + len(rates)

    def _ring_write(self, first_step: int, rates: Sequence[float]) -> None:
        """Entries of optimizer steps ``first_step ..`` := ``rates`` (<= lr_ring values), on
        the current stream; two copies where the range wraps."""
        n, R = len(rates), self.lr_ring
        i0 = (first_step - 1) & self.lr_mask
        for j, r in enumerate(rates):
            self._ring_host[(i0 + j) & self.lr_mask] = r
        if self._ring_uniform is None or any(r != self._ring_uniform for r in rates):
            self._ring_uniform = None
        src = torch.tensor(rates, dtype=torch.float64).to(torch.float32)  # fill_'s rounding
        buf = None
        if self.native:
            buf = self._stage_buffer()
            buf[:n].copy_(src)
            src = buf
        n1 = min(n, R - i0)
        self.lr_tensor[i0:i0 + n1].copy_(src[:n1], non_blocking=True)
        if n1 < n:
            self.lr_tensor[:n - n1].copy_(src[n1:n], non_blocking=True)
        if buf is not None:
            ev = torch.cuda.Event()
            ev.record()
            self._lr_stage.append((buf, ev))

    def _stage_buffer(self) -> torch.Tensor:
        """A pinned ``[lr_ring]`` buffer no copy still reads: chunks are dispatched back to
        back without a sync, so a buffer is taken again only once the event behind its last
        copy has completed (else a new one joins the pool)."""
        for k, (b, ev) in enumerate(self._lr_stage):
            if ev.query():
                del self._lr_stage[k]
                return b
        return torch.empty(self.lr_ring, dtype=torch.float32, pin_memory=True)

    def _opt_steps_in(self, n: int) -> int:
        """Optimizer steps among the next ``n`` batches (accumulation: the windows that close)."""
        if self.accumulate == 1:
            return n
        return sum(self._window(self.step_in_epoch + i)[1] for i in range(n))

    def _ring_prepare(self, n: int) -> None:
        """Ring mode, before ``n`` batches are dispatched: the optimizer steps among them that
        have no scheduled rate get ``lr`` written into their entries (stream-ordered)."""
        if not self.lr_mask or self._ring_uniform == self.lr:
            return
        t0 = self.optimizer_steps + 1
        lo, hi = max(t0, self._sched_end + 1), t0 + self._opt_steps_in(n)
        if hi - lo > self.lr_ring:
            raise RuntimeError(f"ring mode: one dispatch of {hi - lo} optimizer steps exceeds lr_ring={self.lr_ring}")
        if lo < hi and any(self._ring_host[(t - 1) & self.lr_mask] != self.lr for t in range(lo, hi)):
            i0, m = (lo - 1) & self.lr_mask, hi - lo
            n1 = min(m, self.lr_ring - i0)
            self.lr_tensor[i0:i0 + n1].fill_(self.lr)
            if n1 < m:
                self.lr_tensor[:m - n1].fill_(self.lr)
            for t in range(lo, hi):
                self._ring_host[(t - 1) & self.lr_mask] = self.lr

    # ----------------------------------------------------------------- step
    def _kw3(self) -> dict:
        return dict(x_u8=self.x_u8, labels=self.labels, order=self.order, counters=self.counters,
                    n_batches=self.n_batches, B=self.B, L1=self.L1, L2=self.L2, params=self.params,
                    grads=self.grads, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, shadow=self.shadow,
                    dh1t=self.dh1t, xring=self.xring, h1pre=self.h1pre, act=self.act, yring=self.yring,
                    head_part=self.head_part, hand=self.hand, lr=self.lr, betas=self.betas,
                    eps=self.eps, weight_decay=self.wd, lr_tensor=self.lr_tensor, adamw=self.adamw,
                    x_scale=self.x_scale, x_shift=self.x_shift, last_rows=self.last_rows, lr_mask=self.lr_mask)

    def _short_pos(self, pos: int) -> bool:
        """Whether the step at epoch position ``pos`` touches the epoch's short last batch:
        position ``n_batches - 2`` gathers it, ``n_batches - 1`` consumes it (with one or two
        batches per epoch, every step does).  The one-launch kernel has no short batch, so an
        engine that runs one launch per step runs these two as head + tail."""
        return self.last_rows != self.B and pos >= self.n_batches - 2

    def _sgd_kw(self) -> dict:
        """The SGD arguments of the launch that applies the optimizer (MLP3_STEP /
        MLP3_TAIL_ADAM); empty for the Adam engines."""
        if not self.sgd:
            return {}
        return dict(sgd_momentum=self.momentum, sgd_dampening=self.dampening, sgd_nesterov=self.nesterov)

    def prime(self) -> None:
        """Layer-1 pre-activations of the pending batch from the current weights."""
        if self._shadow_stale:
            self._shadow_stale = False
            fused_mlp.mlp_refresh_shadow(self.params, self.shadow, self.L1, self.L2)
        if self.native:
            self.h1pre.zero_()
            fused_mlp.mlp3_launch(fused_mlp.MLP3_PRIME, **self._kw3())
        self._primed = True

    def _window(self, pos: int, in_graph: bool = False):
        """(index inside its accumulation window, whether it closes the window) of the
        micro-batch at epoch position ``pos``.  ``in_graph``: ``pos`` counts from a
        window-aligned start before the epoch's short last window (what a graph holds)."""
        k = self.accumulate
        closing = (pos + 1) % k == 0 or (not in_graph and pos + 1 >= self.n_batches)
        return pos % k, closing

    @property
    def _grad_scale(self) -> float:
        return 1.0 / (self.world_size * self.accumulate)

    def _device_step(self, graph_pos: Optional[int] = None) -> None:
        """One batch on the device (or the fp32 reference step on the CPU): an optimizer
        step, or with ``accumulate`` > 1 one micro-batch (``graph_pos``: its position in
        the graph being captured, else ``step_in_epoch`` places it)."""
        if self.x_u8 is None:
            raise RuntimeError("set_data() first")
        if not self._primed:
            self.prime()
        if self.accumulate > 1:
            micro, closing = (self._window(self.step_in_epoch) if graph_pos is None
                              else self._window(graph_pos, in_graph=True))
            if not self.native:
                self._reference_step(micro, closing)
                return
            kw = self._kw3()
            acc = dict(acc_add=micro > 0, acc_rows=True, acc_head_row=self._head_row)
            # a one-block head writes its row to _head_row (a one-row ring); the tail files it
            fused_mlp.mlp3_launch(fused_mlp.MLP3_HEAD, stats=self._head_row, advance_step=closing, **kw)
            if not closing:
                fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_ACC, stats=self.stats, **acc, **kw)
                return
            fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_GRAD, stats=self.stats, **acc, **kw)
            if self.allreduce is not None:
                self.allreduce(self.comm_buffer)
            clip = {}
            if self.clip_norm is not None:
                clip_partials(self.grads, CLIP_NBLK, out=self.clip_part)
                clip = dict(clip_part=self.clip_part, clip_max_norm=self.clip_norm, clip_out=self.clip_out)
            fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_ADAM, grad_scale=self._grad_scale, **clip, **self._sgd_kw(),
                                  **kw)
            return
        if not self.native:
            self._reference_step()
        else:
            kw = self._kw3()
            if self.clip_norm is not None:
                fused_mlp.mlp3_launch(fused_mlp.MLP3_HEAD, stats=self.stats, **kw)
                fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_GRAD, stats=self.stats, **kw)
                if self.allreduce is not None:
                    self.allreduce(self.comm_buffer)
                clip_partials(self.grads, CLIP_NBLK, out=self.clip_part)
                fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_ADAM, grad_scale=1.0 / self.world_size,
                                      clip_part=self.clip_part, clip_max_norm=self.clip_norm,
                                      clip_out=self.clip_out, **self._sgd_kw(), **kw)
            elif self.world_size == 1 and not self.dp_loop:
                # a captured graph of one-launch steps is replayed before the short batch only
                # (_graph_ok); an eager step is placed by step_in_epoch
                one = self.one_launch and (graph_pos is not None or not self._short_pos(self.step_in_epoch))
                if one:  # never meets the short batch: every batch it gathers or consumes is full
                    fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1, stats=self.stats, **{**kw, "last_rows": self.B})
                else:
                    fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP, stats=self.stats, **self._sgd_kw(), **kw)
            elif self.dp_ctx is not None:
                kind = fused_mlp.MLP3_STEP1_DP if self.one_launch_dp else fused_mlp.MLP3_STEP_DP
                fused_mlp.mlp3_launch(kind, stats=self.stats, grad_scale=1.0 / self.dp_ctx[0],
                                      dp_ctx=self.dp_ctx, dp_proto=fused_mlp.DP_PROTOS.get(self.dp_proto, -1),
                                      dp_loop=self.dp_loop, **kw)
                self._stepped_owner = self._stepped_owner or (self.one_launch_dp and self.dp_proto == "owner")
            else:
                fused_mlp.mlp3_launch(fused_mlp.MLP3_HEAD, stats=self.stats, **kw)
                fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_GRAD, stats=self.stats, **kw)  # multi-block head stats
                if self.allreduce is not None:
                    self.allreduce(self.comm_buffer)
                fused_mlp.mlp3_launch(fused_mlp.MLP3_TAIL_ADAM, grad_scale=1.0 / self.world_size,
                                      **self._sgd_kw(), **kw)

    def _reference_step(self, micro: int = 0, closing: bool = True) -> None:
        """fp32 PyTorch step with the device kernels' batch / counter semantics
        (``accumulate`` > 1: micro-batch ``micro`` of its window, Adam when ``closing``)."""
        c = self.counters
        cursor, ob = int(c[1]), int(c[4])
        acc = self.accumulate > 1
        # the reference kernels keep their one-scalar contract: the ring entry of the optimizer
        # step this window applies (counters[0] + 1), as a one-element view
        i_lr = int(c[0]) & self.lr_mask
        lr_now = self.lr_tensor[i_lr:i_lr + 1]
        # SGD: mlp_train_step leaves the gradient, fused_sgd_ follows below
        fused = self.world_size == 1 and self.clip_norm is None and not acc and not self.sgd
        fused_mlp.mlp_train_step(
            self.params, self.grads, L1=self.L1, L2=self.L2, B=self.B, labels=self.labels, x_u8=self.x_u8,
            order=self.order[ob], counters=c[:2], n_batches=self.n_batches, exp_avg=self.exp_avg,
            exp_avg_sq=self.exp_avg_sq, stats=self._head_row if acc else self.stats, accumulate_grad=micro > 0,
            apply_adam=fused, advance_step=closing, lr=self.lr,
            betas=self.betas, eps=self.eps, weight_decay=self.wd, lr_tensor=lr_now, adamw=self.adamw,
            x_scale=self.x_scale, x_shift=self.x_shift, last_rows=self.last_rows,
        )
        c[2] = cursor
        c[3] = int(c[3]) ^ 1
        if cursor + 1 >= self.n_batches:
            c[4] = ob ^ 1
        if acc:  # one stats row per micro-batch, as the accumulating tails file it
            w = fused_mlp.MLP3_ROW_WORD
            self.stats[int(c[w]) % self.stats.size(0)] = self._head_row[0]
            c[w] += 1
        self._publish_counters()
        if not closing:
            return
        if not fused:
            if self.allreduce is not None:
                self.allreduce(self.comm_buffer)
            if self.clip_norm is not None:
                self._reference_clip()
            if self.sgd:  # first = counters[0] <= 1, the kernels' rule
                fused_sgd_(self.params, self.grads, self.exp_avg if self.momentum != 0.0 else None, lr=self.lr,
                           momentum=self.momentum, dampening=self.dampening, weight_decay=self.wd,
                           nesterov=self.nesterov, grad_scale=self._grad_scale, step=self.counters[0:1],
                           lr_tensor=lr_now)
                return
            fused_adam_(self.params, self.grads, self.exp_avg, self.exp_avg_sq, lr=self.lr, betas=self.betas,
                        eps=self.eps, weight_decay=self.wd, grad_scale=self._grad_scale, adamw=self.adamw,
                        step=self.counters[0:1], lr_tensor=lr_now)

    def _reference_clip(self) -> None:
        """The ADAM tail's clipping in torch fp32: scales ``grads`` in place by the
        coefficient (the 1 / world average stays in ``grad_scale``) and keeps ``clip_out``."""
        part = clip_partials(self.grads, CLIP_NBLK, out=self.clip_part)
        ss = torch.zeros((), dtype=torch.float32)
        for i in range(CLIP_NBLK):  # index order, as the kernel's scalar lane
            ss = ss + part[i]
        norm = ss.sqrt() * torch.tensor(self._grad_scale, dtype=torch.float32)
        coef = torch.clamp(torch.tensor(self.clip_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)
        if bool(torch.isnan(coef)):
            coef = torch.ones(())  # fminf(1, NaN) = 1: the kernel passes a NaN norm through
        if float(coef) < 1.0:
            self.grads.mul_(coef)
            self.clip_out[2] += 1
        if not bool(torch.isfinite(norm)):
            self.clip_out[3] += 1
        self.clip_out[0], self.clip_out[1] = norm, coef

    def _advance_host(self, n: int) -> None:
        self.optimizer_steps += self._opt_steps_in(n)  # accumulation: the windows that close
        self.global_step += n
        self.step_in_epoch += n
        if self.step_in_epoch >= self.n_batches:
            # the device switched to the other order buffer in the same step
            self.epoch += 1
            self.step_in_epoch = 0
            if self._host_epochs:
                return  # the host calls begin_epoch()
            # buffer (epoch + 1) % 2 was last read by the step just enqueued
            self._fill_order(self.epoch + 1)

    def steps_to_epoch_end(self) -> int:
        return self.n_batches - self.step_in_epoch

    def _drop_graphs(self) -> None:
        self._graph = None
        self._tail_graphs = {}

    def capture(self, steps_per_graph: int = 1, remainders: bool = True) -> bool:
        """Capture ``steps_per_graph`` consecutive steps into one hipGraph.

        ``remainders``: also capture 1, 2, 4, ... step graphs below it, so a
        dispatch that is not a multiple of ``steps_per_graph`` (the Trainer's
        chunks end at log / validation / epoch boundaries) runs as a few replays
        instead of eager launches (~40 us of host work per eager step against
        ~9 us of GPU time, so eager remainders starved the GPU)."""
        K = self.accumulate
        if K > 1 and (steps_per_graph < K or steps_per_graph % K != 0):
            # a graph holds whole windows: each captured launch has its place in the window baked in
            raise ValueError(f"capture({steps_per_graph}): with accumulate={K} a graph must hold whole windows "
                             f"(a multiple of {K} batches)")
        if self.lr_mask and steps_per_graph // K > self.lr_ring:
            raise ValueError(f"capture({steps_per_graph}): a graph of {steps_per_graph // K} optimizer steps does "
                             f"not fit the learning-rate ring (lr_ring={self.lr_ring})")
        if not self.native:
            return False
        self._ring_prepare(K)  # the warm-up batches' rates, ahead of the side stream's wait
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        # warm the allocator / RCCL outside capture (a real step; keeps counters consistent);
        # accumulation: K real batches, so both kinds of micro-batch have run
        for _ in range(K):
            with torch.cuda.stream(s):
                self._device_step()
            torch.cuda.current_stream().wait_stream(s)
            self._advance_host(1)
            if K > 1:  # the next warm-up batch follows what _advance_host enqueued
                s.wait_stream(torch.cuda.current_stream())

        def record(n: int):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for i in range(n):
                    self._device_step(i)  # K == 1: only marks the step as captured
            return g

        try:
            g = record(steps_per_graph)
        except Exception:
            self._drop_graphs()
            return False
        self._graph = g
        self._graph_steps = steps_per_graph
        self._tail_graphs = {}
        if remainders:
            k = K  # 1 without accumulation; else whole windows only
            while k < steps_per_graph:
                try:
                    self._tail_graphs[k] = record(k)  # capture only: the device state does not move
                except Exception:
                    break
                k *= 2
        return True

    def _graph_ok(self, remaining: int, k: Optional[int] = None) -> bool:
        k = self._graph_steps if k is None else k
        if self.accumulate > 1:
            # only from a window-aligned position, and only before the epoch's short last window
            full = self.n_batches // self.accumulate * self.accumulate
            if self.step_in_epoch % self.accumulate != 0 or self.step_in_epoch + k > full:
                return False
        if (self.last_rows != self.B and self.one_launch and self.world_size == 1 and not self.dp_loop
                and self._short_pos(self.step_in_epoch + k - 1)):
            # the graph holds one-launch steps: the two steps that gather and consume the
            # epoch's short last batch run eagerly, as head + tail
            return False
        return (self._graph is not None and self._primed and remaining >= k
                and self.step_in_epoch + k <= self.n_batches)

    def _pick_graph(self, remaining: int):
        """The largest captured graph that fits the remaining steps (and the epoch)."""
        if self._graph_ok(remaining):
            return self._graph, self._graph_steps
        for k in sorted(self._tail_graphs, reverse=True):
            if self._graph_ok(remaining, k):
                return self._tail_graphs[k], k
        return None, 1

    def step(self) -> None:
        """Run one (or ``steps_per_graph`` when captured) batch(es): optimizer steps, or
        micro-batches with ``accumulate`` > 1."""
        if self._graph_ok(self._graph_steps):
            self._ring_prepare(self._graph_steps)
            self._graph.replay()
            self._advance_host(self._graph_steps)
            return
        self._ring_prepare(1)
        self._device_step()
        self._advance_host(1)

    def run(self, n_steps: int) -> None:
        done = 0
        while done < n_steps:
            g, k = self._pick_graph(n_steps - done)
            self._ring_prepare(k)
            if g is not None:
                g.replay()
            else:
                self._device_step()
            self._advance_host(k)
            done += k

    # --------------------------------------------------------------- export
    def recent_stats(self, n: int = 1) -> torch.Tensor:
        """Last n (loss, correct, count, step) rows, oldest first (host copy).  With
        ``accumulate`` > 1: the last n micro-batch rows (column 3: the optimizer step each
        contributes to)."""
        t = self.global_step
        ring = self.stats.size(0)
        rows = [(t - 1 - i) % ring for i in range(min(n, t, ring))][::-1]
        return self.stats[rows].cpu() if rows else torch.zeros(0, 4)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: v.detach().cpu().clone() for k, v in fused_mlp.mlp_unpack(self.params, self.L1, self.L2).items()}

    def optimizer_state_dict(self) -> Dict:
        """torch.optim.Adam / AdamW / SGD .state_dict() layout (Lightning checkpoint
        `optimizer_states`).  Collective under the owner protocol (state consolidation)."""
        if self.sgd:
            # torch's SGD state: a momentum_buffer per parameter once a step has run (none
            # without momentum), and no step count
            names = list(fused_mlp.mlp_unpack(self.params, self.L1, self.L2))
            state = {}
            if self.momentum != 0.0 and self.optimizer_steps > 0:
                buf = fused_mlp.mlp_unpack(self.exp_avg, self.L1, self.L2)
                state = {i: {"momentum_buffer": buf[k].detach().cpu().clone()} for i, k in enumerate(names)}
            group = {"lr": self.lr, "momentum": self.momentum, "dampening": self.dampening,
                     "weight_decay": self.wd, "nesterov": self.nesterov, "maximize": False, "foreach": None,
                     "differentiable": False, "fused": None, "params": list(range(len(names)))}
            return {"state": state, "param_groups": [group]}
        self.sync_optimizer_state()
        step = float(self.counters[0].item())
        m = fused_mlp.mlp_unpack(self.exp_avg, self.L1, self.L2)
        v = fused_mlp.mlp_unpack(self.exp_avg_sq, self.L1, self.L2)
        state = {}
        for i, k in enumerate(m):
            state[i] = {"step": torch.tensor(step), "exp_avg": m[k].detach().cpu().clone(),
                        "exp_avg_sq": v[k].detach().cpu().clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.wd,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                 "differentiable": False, "fused": None, "params": list(range(len(m)))}
        return {"state": state, "param_groups": [group]}
