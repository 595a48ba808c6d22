"""Fused MNIST-classifier MLP step (784 -> L1 -> L2 -> 10).

GPU: one HIP launch per training step (``csrc/mlp_kernels.hip``): forward,
log_softmax + NLL + accuracy, backward and -- at world size 1 -- the Adam
update fused into the weight-gradient epilogues.  CPU: an fp32 PyTorch
reference with identical semantics (also the oracle for the GPU tests).

Parameter arena layout (== ``nn.Linear`` state_dict order of
``layer_1``/``layer_2``/``layer_3``):  W1[L1,784] b1[L1] W2[L2,L1] b2[L2] W3[10,L2] b3[10].
"""
from __future__ import annotations

import math
import struct
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import require, use_native

IN_FEATURES = 784
NUM_CLASSES = 10
SUPPORTED = {(32, 32), (32, 64), (32, 128), (32, 256), (64, 64), (64, 128), (64, 256),
             (128, 64), (128, 128), (128, 256)}


def mlp_param_count(L1: int, L2: int) -> int:
    return L1 * IN_FEATURES + L1 + L2 * L1 + L2 + NUM_CLASSES * L2 + NUM_CLASSES


def mlp_supported(L1: int, L2: int) -> bool:
    return (int(L1), int(L2)) in SUPPORTED


def mlp_unpack(flat: torch.Tensor, L1: int, L2: int) -> Dict[str, torch.Tensor]:
    """Views of the arena as nn.Linear tensors (state_dict key order)."""
    shapes = [
        ("layer_1.weight", (L1, IN_FEATURES)), ("layer_1.bias", (L1,)),
        ("layer_2.weight", (L2, L1)), ("layer_2.bias", (L2,)),
        ("layer_3.weight", (NUM_CLASSES, L2)), ("layer_3.bias", (NUM_CLASSES,)),
    ]
    out, off = {}, 0
    for name, shp in shapes:
        n = math.prod(shp)
        out[name] = flat[off:off + n].view(shp)
        off += n
    assert off == flat.numel(), "arena size mismatch"
    return out


def _f32(v: float) -> float:
    """``v`` rounded once to fp32 (returned as a Python float).  No tensor is built: the
    launch wrappers call this per launch."""
    v = float(v)
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:  # finite, beyond fp32: what the C cast gives
        return math.copysign(math.inf, v)


# the kernels' default u8 -> bf16 map (csrc/kernels.h kMLPXScale): ToTensor alone
X_SCALE_DEFAULT = _f32(1.0 / 255.0)


def normalize_pair(normalize) -> Optional[Tuple[float, float]]:
    """``(mean, std)`` of a single-channel ``Normalize`` as two floats (each given as a scalar,
    a one-element sequence or tensor); None stays None.  More than one channel, ``std <= 0``
    or a non-finite value raises."""
    if normalize is None:
        return None

    def scalar(v, name):
        if isinstance(v, torch.Tensor):
            v = v.reshape(-1).tolist()
        if isinstance(v, (list, tuple)):
            if len(v) != 1:
                raise ValueError(f"{name} must be one value (single-channel Normalize), got {v!r}")
            v = v[0]
        return float(v)

    mean, std = normalize
    mean, std = scalar(mean, "mean"), scalar(std, "std")
    if not (math.isfinite(std) and std > 0.0):
        raise ValueError(f"Normalize: std must be finite and > 0, got {std}")
    if not math.isfinite(mean):
        raise ValueError(f"Normalize: mean must be finite, got {mean}")
    return mean, std


def input_affine(normalize=None) -> Tuple[float, float]:
    """``(x_scale, x_shift)`` of the kernels' u8 -> bf16 conversion
    ``bf16(fmaf(u8, x_scale, x_shift))`` -- the one place that derives them.  ``None``:
    ToTensor alone, ``(float32(1/255), 0.0)``, bitwise the kernels' former ``u8 * (1/255)``.
    ``(mean, std)`` (``normalize_pair``): ``float32(1 / (255 std))``, ``float32(-mean / std)``,
    each computed in float64 and rounded once."""
    pair = normalize_pair(normalize)
    if pair is None:
        return X_SCALE_DEFAULT, 0.0
    mean, std = pair
    scale, shift = _f32(1.0 / (255.0 * std)), _f32(-mean / std) + 0.0  # (+ 0.0: mean 0 gives +0, not -0)
    if not (math.isfinite(scale) and scale > 0.0 and math.isfinite(shift)):
        raise ValueError(f"Normalize({mean}, {std}) leaves the fp32 range (scale {scale}, shift {shift})")
    return scale, shift


def check_input_affine(x_scale: float, x_shift: float) -> Tuple[float, float]:
    """What every launch accepts (the kernels' own rule, csrc/kernels.h): a finite positive
    fp32 scale and a finite fp32 shift."""
    sc, sh = _f32(x_scale), _f32(x_shift)
    if not (math.isfinite(sc) and sc > 0.0 and math.isfinite(sh)):
        raise ValueError(f"x_scale must be finite and > 0 and x_shift finite, got {x_scale}, {x_shift}")
    return sc, sh


def u8_to_input(x_u8: torch.Tensor, x_scale: float = X_SCALE_DEFAULT, x_shift: float = 0.0) -> torch.Tensor:
    """The kernels' pixel map in fp32 FMA semantics: ``float32(u8 * x_scale + x_shift)``, the
    product and sum exact in float64 (8 + 24 significant bits) and rounded once.  The
    kernels round this value to bf16."""
    return (x_u8.double() * float(x_scale) + float(x_shift)).float()


def check_last_rows(last_rows, B: int, what: str) -> int:
    """Valid rows of an epoch's last batch: None means a full one, else an integer in [1, B]
    (the kernels' rule, csrc/kernels.h: launch_mlp3 answers -15 for anything else)."""
    if last_rows is None:
        return int(B)
    if isinstance(last_rows, bool) or int(last_rows) != last_rows or not 1 <= int(last_rows) <= int(B):
        raise ValueError(f"{what}: last_rows must be an integer in [1, B = {int(B)}], got {last_rows!r} "
                         "(nothing was launched)")
    return int(last_rows)


def _gather_batch(x_u8, x_f32, labels, order, cursor, B, index=None, x_scale=X_SCALE_DEFAULT, x_shift=0.0):
    if x_u8 is not None:
        if index is None:
            index = order[cursor * B:(cursor + 1) * B]
        rows = x_u8.index_select(0, index)
        if x_scale == X_SCALE_DEFAULT and x_shift == 0.0:
            x = rows.float() / 255.0  # ToTensor alone: the reference as it always was (equal after bf16 rounding)
        else:
            # a Normalize: the FMA, rounded to bf16 as the kernels store it (xring / LDS)
            x = u8_to_input(rows, x_scale, x_shift).to(torch.bfloat16).float()
        y = labels.index_select(0, index)
    else:
        x = x_f32.reshape(B, IN_FEATURES).float()
        y = labels
    return x, y


def _reference_forward(p: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    h1 = F.relu(F.linear(x, p["layer_1.weight"], p["layer_1.bias"]))
    h2 = F.relu(F.linear(h1, p["layer_2.weight"], p["layer_2.bias"]))
    return F.linear(h2, p["layer_3.weight"], p["layer_3.bias"])


def mlp_train_step(
    params: torch.Tensor,
    grads: torch.Tensor,
    *,
    L1: int,
    L2: int,
    B: int,
    labels: torch.Tensor,
    x_u8: Optional[torch.Tensor] = None,
    x_f32: Optional[torch.Tensor] = None,
    order: Optional[torch.Tensor] = None,
    counters: Optional[torch.Tensor] = None,
    n_batches: int = 0,
    exp_avg: Optional[torch.Tensor] = None,
    exp_avg_sq: Optional[torch.Tensor] = None,
    stats: Optional[torch.Tensor] = None,
    accumulate_grad: bool = False,
    apply_adam: bool = False,
    advance_step: bool = True,
    lr: float = 1e-3,
    betas: Tuple[float, float] = (0.9, 0.999),
    eps: float = 1e-8,
    weight_decay: float = 0.0,
    lr_tensor: Optional[torch.Tensor] = None,
    adamw: bool = False,
    stamps: Optional[torch.Tensor] = None,
    x_scale: float = X_SCALE_DEFAULT,
    x_shift: float = 0.0,
    last_rows: Optional[int] = None,
) -> None:
    """One training micro-step of the MNIST MLP over a flat parameter arena.

    u8 mode (``x_u8`` = GPU-resident uint8 dataset [N, 784]): the batch is
    ``order[cursor*B:(cursor+1)*B]`` with ``cursor = counters[1]``, which the
    step advances (mod ``n_batches``) -- so a captured hipGraph replays
    successive batches.  ``counters[0]`` is the optimizer step t.  A pixel enters the
    network as ``fmaf(u8, x_scale, x_shift)`` (``input_affine``); ``x_f32`` mode ignores both.
    ``last_rows`` (u8 mode, the fp32 reference only): the batch at cursor ``n_batches - 1``
    holds that many rows, ``order[cursor*B : cursor*B + last_rows]``; loss and gradient are
    their mean and the stats row counts them (None or ``B``: every batch is full).
    """
    if x_u8 is not None:
        x_scale, x_shift = check_input_affine(x_scale, x_shift)
    last_rows = check_last_rows(last_rows, B, "mlp_train_step")
    if last_rows != int(B) and (x_u8 is None or use_native(params)):
        raise ValueError("mlp_train_step: a short last batch (last_rows < B) exists in the u8-mode fp32 reference "
                         "and in the mlp3 kernels (mlp3_launch) only")
    if use_native(params):
        require().mlp_train_step(
            x_u8, x_f32, labels, order, counters, int(n_batches), int(B), int(L1), int(L2),
            params, grads, exp_avg, exp_avg_sq, stats, bool(accumulate_grad), bool(apply_adam),
            bool(advance_step), float(lr), float(betas[0]), float(betas[1]), float(eps),
            float(weight_decay), lr_tensor, bool(adamw), stamps, float(x_scale), float(x_shift),
        )
        return
    # ---- fp32 reference ----
    cursor = int(counters[1].item()) if (counters is not None and x_u8 is not None) else 0
    rows = last_rows if (x_u8 is not None and cursor == int(n_batches) - 1) else int(B)
    index = order[cursor * B:cursor * B + rows] if rows != int(B) else None
    x, y = _gather_batch(x_u8, x_f32, labels, order, cursor, B, index=index, x_scale=x_scale, x_shift=x_shift)
    with torch.enable_grad():
        leaf = params.detach().clone().requires_grad_(True)
        p = mlp_unpack(leaf, L1, L2)
        logits = _reference_forward(p, x)
        logp = F.log_softmax(logits, dim=1)
        loss = F.nll_loss(logp, y)
        (g,) = torch.autograd.grad(loss, [leaf])
    with torch.no_grad():
        if accumulate_grad:
            g = g + grads
        t = (int(counters[0].item()) if counters is not None else 0) + 1
        if apply_adam:
            from .optim import fused_adam_

            gbuf = g.clone()
            fused_adam_(params, gbuf, exp_avg, exp_avg_sq, lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay, adamw=adamw, step=t, lr_tensor=lr_tensor)
        else:
            grads.copy_(g)
        if counters is not None:
            if advance_step:
                counters[0] = t
            if x_u8 is not None:
                counters[1] = (cursor + 1) % n_batches if n_batches > 0 else cursor + 1
        if stats is not None:
            ring = stats.numel() // 4
            slot = (t - 1) % max(ring, 1)
            correct = (logp.argmax(dim=1) == y).sum().float()
            stats.view(-1, 4)[slot] = torch.stack(
                [loss.detach(), correct, torch.tensor(float(rows)), torch.tensor(float(t))])


def mlp_shadow_layout(L1: int, L2: int) -> Dict[str, int]:
    """bf16 shadow layout: row-major copy [0, np), W2^T at w2t, W3^T (classes padded to 16) at w3t."""
    np_ = mlp_param_count(L1, L2)
    w2t = (np_ + 7) // 8 * 8
    w3t = w2t + L1 * L2
    return {"np": np_, "w2t": w2t, "w3t": w3t, "total": w3t + 16 * L2}


def mlp_refresh_shadow(params: torch.Tensor, shadow: torch.Tensor, L1: int, L2: int) -> None:
    """Recompute every bf16 shadow from the fp32 master weights."""
    if use_native(params):
        require().mlp_adam(params, params, params, params, shadow, int(L1), int(L2), 0.0, 0.9, 0.999, 1e-8, 0.0,
                           1.0, False, False, None, None)
        return
    lay = mlp_shadow_layout(L1, L2)
    v = mlp_unpack(params, L1, L2)
    with torch.no_grad():
        shadow[: lay["np"]].copy_(params)
        shadow[lay["w2t"]: lay["w3t"]].copy_(v["layer_2.weight"].t().reshape(-1))
        w3t = torch.zeros(L2, 16, dtype=params.dtype, device=params.device)
        w3t[:, :NUM_CLASSES] = v["layer_3.weight"].t()
        shadow[lay["w3t"]: lay["total"]].copy_(w3t.reshape(-1))


MLP3_STEP, MLP3_HEAD, MLP3_TAIL_GRAD, MLP3_TAIL_ADAM, MLP3_PRIME, MLP3_STEP_DP, MLP3_STEP1, MLP3_STEP1_DP = range(8)
# the tail of a micro-batch that does not close its gradient-accumulation window
MLP3_TAIL_ACC = 8
# counters word that counts the stats rows written under ``acc_rows`` (kernels.h kMLP3RowWord)
MLP3_ROW_WORD = 11
ONE_LAUNCH_MAX_B = 32  # MLP3_STEP1 / MLP3_STEP1_DP: one head workgroup
# exchange protocols of MLP3_STEP1_DP (csrc/mlp_step3.hip, "Wave-positioned exchange protocols")
DP_GRANULE, DP_PACKED, DP_OWNER = 0, 1, 2
DP_PROTOS = {"granule": DP_GRANULE, "packed": DP_PACKED, "owner": DP_OWNER}
# floats per (slot, rank) receive area of the packed / owner protocols (comm/xgmi.h kDpUnitAreaFloats)
DP_AREA_FLOATS = 327680


def mlp3_dp_capacity(L1: int, L2: int) -> int:
    """Receive-area capacity (floats) for NativeCommunicator.dp_context that every
    one-launch protocol fits: 2 floats per parameter (granule) or the wave-positioned
    areas (packed / owner)."""
    return max(2 * mlp_param_count(L1, L2), DP_AREA_FLOATS)


def mlp3_hand_words(L1: int, L2: int) -> int:
    """int64 words of the one-launch step's acknowledgement / error buffer (csrc/mlp_step3.hip)."""
    return 32


# word indices of ``hand`` as csrc/mlp_step3.hip defines them (``_C.mlp3_hand_layout()``;
# this copy serves the CPU engine and is checked against the extension when it loads)
HAND_LAYOUT = {"ack": 0, "err": 16, "sat": 17, "nonfinite": 18, "last_step": 19, "words": 32}
_hand_layout: Optional[Dict[str, int]] = None


def mlp3_hand_layout(native: bool = True) -> Dict[str, int]:
    """Where the kernels keep what in ``hand``: ``ack`` / ``err`` (the one-launch
    hand-off), ``sat`` / ``nonfinite`` / ``last_step`` (health of the layer-1 partial
    sums).  ``native``: read it from the extension (an engine on the GPU does)."""
    global _hand_layout
    if not native:
        return dict(HAND_LAYOUT)
    if _hand_layout is None:
        lay = {k: int(v) for k, v in require().mlp3_hand_layout().items()}
        if lay != HAND_LAYOUT:
            raise RuntimeError(f"hand layout of the extension {lay} differs from ops.fused_mlp.HAND_LAYOUT")
        _hand_layout = lay
    return dict(_hand_layout)


# further words of ``hand``: the one-launch step's cache of Adam's bias corrections for
# the NEXT step (csrc/mlp_step3.hip, ``_C.mlp3_adam_cache_layout()``).  ``step`` and
# ``betas`` (bits(beta1) | bits(beta2) << 32) are the key; ``bc1`` holds 1 - beta1^step and
# ``bc2_sqrt`` sqrt(1 - beta2^step), both as f64 bits.  A launch whose step or betas
# differ from the key ignores the entry and computes the values itself.
ADAM_CACHE_LAYOUT = {"step": 20, "betas": 21, "bc1": 22, "bc2_sqrt": 23}


def mlp3_adam_cache_layout(native: bool = True) -> Dict[str, int]:
    """Word indices of the bias-correction cache in ``hand`` (kept apart from
    ``mlp3_hand_layout``, which describes the hand-off and health words)."""
    if native:
        lay = {k: int(v) for k, v in require().mlp3_adam_cache_layout().items()}
        if lay != ADAM_CACHE_LAYOUT:
            raise RuntimeError(f"Adam cache layout of the extension {lay} differs from ops.fused_mlp.ADAM_CACHE_LAYOUT")
    return dict(ADAM_CACHE_LAYOUT)


W1_TILES = IN_FEATURES // 16
H1_SAT = 32.0  # |tile partial| beyond this is clamped by the 12.20 conversion


def mlp3_h1_health(x_rows: torch.Tensor, w1_bf16: torch.Tensor) -> Tuple[int, int]:
    """(saturated, nonfinite) over the 49 x B x L1 layer-1 tile partials of one batch,
    as the kernels classify them (csrc/mlp_step3.hip ``h1_check``): fp32 partial
    sums over 16 pixels of bf16 operands; non-finite = NaN or Inf, saturated =
    finite and beyond +-32 (what the fixed-point conversion clamps).  Pure torch, on
    the CPU: the oracle of the health counters.  ``x_rows``: [B, 784] pixels as they
    enter layer 1 -- in [0, 1], or normalised (``u8_to_input``) -- real batch rows only,
    ``w1_bf16``: [L1, 784]."""
    xt = x_rows.detach().cpu().to(torch.bfloat16).double().view(x_rows.size(0), W1_TILES, 16)
    wt = w1_bf16.detach().cpu().to(torch.bfloat16).double().view(w1_bf16.size(0), W1_TILES, 16)
    part = torch.einsum("bti,mti->tbm", xt, wt).float()  # fp32 MFMA partials
    mag = part.abs()
    bad = ~(mag <= torch.finfo(torch.float32).max)
    sat = (mag > H1_SAT) & ~bad
    return int(sat.sum()), int(bad.sum())


def mlp3_h1_copies(L1: int) -> int:
    """H1pre copies per ring slot (csrc/mlp_step3.hip ``H1Copies``): the 49 W1 tiles'
    layer-1 partials are atomically added into ``copies`` separate buffers (tile kt
    into copy kt % copies), which the head sums as it loads them."""
    return 2 if int(L1) <= 64 else 1


def mlp3_buffers(L1: int, L2: int, B: int, device) -> Dict[str, torch.Tensor]:
    """Device scratch of the v3 pipelined step (see csrc/mlp_step3.hip)."""
    bp = (B + 31) // 32 * 32
    return {
        "dh1t": torch.zeros(L1 * bp, dtype=torch.bfloat16, device=device),
        "xring": torch.zeros(2 * W1_TILES * bp * 16, dtype=torch.bfloat16, device=device),
        # 12.20 fixed point (int32): integer atomics make the 49-way split-K sum
        # order-independent; [slot][copy][Bp * L1] (see mlp3_h1_copies)
        "h1pre": torch.zeros(2 * mlp3_h1_copies(L1) * bp * L1, dtype=torch.int32, device=device),
        "act": torch.zeros((L1 + 2 * L2 + 16) * bp, dtype=torch.bfloat16, device=device),
        "yring": torch.full((2 * bp,), -1, dtype=torch.int32, device=device),
        # [0, 5) current state, [5, 10) the head's advanced copy (published by the tail),
        # [10] the one-launch step's launch sequence number (its hand-off tag),
        # [11] stats rows written by accumulating tails (one per micro-batch)
        "counters": torch.zeros(16, dtype=torch.int64, device=device),
        # one-launch step: [0] per-block state acknowledgements (monotonic), [16] wait-timeout flag;
        # every step kind: [17] saturated / [18] non-finite layer-1 partials, [19] last such step
        "hand": torch.zeros(mlp3_hand_words(L1, L2), dtype=torch.int64, device=device),
        # per-head-workgroup (sum NLL, #correct, #rows, -) when the batch spans several
        "head_part": torch.zeros(bp // 32 * 4, device=device),
    }


def mlp3_launch(
    kind: int,
    *,
    x_u8: torch.Tensor,
    labels: torch.Tensor,
    order: torch.Tensor,
    counters: torch.Tensor,
    n_batches: int,
    B: int,
    L1: int,
    L2: int,
    params: torch.Tensor,
    grads: torch.Tensor,
    exp_avg: Optional[torch.Tensor],
    exp_avg_sq: Optional[torch.Tensor],
    shadow: torch.Tensor,
    dh1t: torch.Tensor,
    xring: torch.Tensor,
    h1pre: torch.Tensor,
    act: torch.Tensor,
    yring: torch.Tensor,
    stats: Optional[torch.Tensor] = None,
    advance_step: bool = True,
    lr: float = 1e-3,
    betas: Tuple[float, float] = (0.9, 0.999),
    eps: float = 1e-8,
    weight_decay: float = 0.0,
    grad_scale: float = 1.0,
    lr_tensor: Optional[torch.Tensor] = None,
    adamw: bool = False,
    stamps: Optional[torch.Tensor] = None,
    dp_ctx: Optional[Sequence[int]] = None,
    head_part: Optional[torch.Tensor] = None,
    hand: Optional[torch.Tensor] = None,
    dp_proto: int = -1,
    dp_loop: bool = False,
    repeat: int = 1,
    clip_part: Optional[torch.Tensor] = None,
    clip_max_norm: float = 0.0,
    clip_out: Optional[torch.Tensor] = None,
    clip_nblk: Optional[int] = None,
    acc_add: bool = False,
    acc_rows: bool = False,
    acc_head_row: Optional[torch.Tensor] = None,
    sgd_momentum: Optional[float] = None,
    sgd_dampening: float = 0.0,
    sgd_nesterov: bool = False,
    x_scale: float = X_SCALE_DEFAULT,
    x_shift: float = 0.0,
    last_rows: Optional[int] = None,
    lr_mask: int = 0,
) -> None:
    """One v3 launch (GPU only; ``repeat``: that many identical launches back to back
    from one C++ loop -- every step's state lives on the device).  ``kind``: MLP3_STEP (head + fused tail, world size 1),
    MLP3_HEAD / MLP3_TAIL_GRAD (gradients, before the allreduce), MLP3_TAIL_ADAM
    (Adam with ``grad_scale`` + next-step layer-1 partial, after it), MLP3_PRIME
    (layer-1 pre-activations of the pending batch from the current weights; the
    caller zeroes ``h1pre`` first), MLP3_STEP_DP (head + tail whose Adam epilogue
    sums the gradient tiles of all ranks over xGMI itself; ``dp_ctx`` is
    ``NativeCommunicator.dp_context``), MLP3_STEP1 (the whole step in ONE launch,
    world size 1, B <= 32: every block replays the head's serial chain on its own
    CU and then does its tail share; ``hand`` holds the blocks' acknowledgements), MLP3_STEP1_DP
    (MLP3_STEP1 for world size > 1: each block allreduces its gradient values over xGMI as
    tagged granules between its gradient and its Adam; ``dp_ctx`` as for MLP3_STEP_DP,
    receive area >= 2 floats per parameter for ``dp_proto`` 0).  ``dp_proto``: the
    one-launch exchange -- DP_GRANULE (0, round 2), DP_PACKED (1, one-shot, two values
    per granule), DP_OWNER (2, reduce-scatter / owner Adam / all-gather); -1 reads
    ``RLA_DP_PROTO``.  ``dp_loop``: loopback diagnostic (one process plays every rank of
    ``dp_ctx`` through its own region).  ``order`` is [2, n_batches * B]:
    the current and the next epoch's sample order (counters[4] selects).

    Gradient clipping (MLP3_TAIL_ADAM only; any other kind raises before a launch):
    ``clip_part`` = ``ops.optim.clip_partials(grads, nblk)``, ``clip_max_norm`` > 0.  The
    tail sums the partials in index order, ``norm = sqrt(sum) * grad_scale``, ``coef =
    min(1, clip_max_norm / (norm + 1e-6))`` (``torch.nn.utils.clip_grad_norm_``), and its
    Adam reads ``grads * grad_scale * coef``.  ``clip_nblk``: partials to read (default:
    all of ``clip_part``).  ``clip_out`` (optional, 4 fp32): [0] norm, [1] coef,
    [2] += 1 when coef < 1, [3] += 1 when the norm is NaN / Inf.

    Gradient accumulation (MLP3_TAIL_GRAD / MLP3_TAIL_ACC only; any other kind raises
    before a launch): MLP3_TAIL_ACC is the tail of a micro-batch that does not close its
    window -- gradients, no Adam, the next batch's layer-1 partial from the unchanged
    weights; it takes no clip arguments.  ``acc_add``: ``grads`` += this micro-batch's
    gradient (one fp32 add per element) instead of the overwrite.  ``acc_rows``: the tail
    writes the micro-batch's stats row at ``counters[MLP3_ROW_WORD] % ring`` and advances
    that word; ``acc_head_row`` ([4] fp32, B <= 32) is where the head launch, given it as
    a one-row ``stats``, left the row.

    SGD (MLP3_STEP / MLP3_TAIL_ADAM only; any other kind raises before a launch):
    ``sgd_momentum`` given (0.0 for plain SGD; None: Adam) makes the tail apply
    ``torch.optim.SGD`` with ``lr`` / ``weight_decay`` / ``grad_scale`` (and the clip
    coefficient) as given, ``sgd_dampening`` and ``sgd_nesterov``.  ``exp_avg`` is then the
    velocity (torch's ``momentum_buffer``, 16-byte aligned; may be None when the momentum is 0,
    and is never touched then) and ``exp_avg_sq`` is unused (None).  The first optimizer step
    (``counters[0] <= 1`` after the head's advance) sets the velocity to the gradient.

    ``x_scale`` / ``x_shift`` (``input_affine``): every gather of a batch (head, PRIME, the
    tails' and the one-launch step's look-ahead) stores ``bf16(fmaf(u8, x_scale, x_shift))``;
    padded rows stay zero.  Non-finite values or a scale <= 0 raise before any launch.
    MLP3_STEP1 runs its Normalize instance for any other map than the default; MLP3_STEP1_DP
    has none (MLP3_STEP_DP serves a normalised dataset) and raises.

    ``last_rows`` (None: ``B``): valid rows of the batch at epoch cursor ``n_batches - 1`` -- the
    short last batch of a ``drop_last=False`` loader; every other cursor holds ``B`` rows.  The
    kernels decide from the device cursor: whoever gathers that batch (the head launch's gather
    blocks, PRIME) reads ``order[cursor*B : cursor*B + last_rows]`` only and stages zero pixels
    and label -1 beyond; whoever consumes it (head, tails) scales loss and gradient by
    ``1 / last_rows`` and files the stats row ``(mean NLL, #correct, last_rows, step)``.
    ``order`` keeps the stride ``n_batches * B``; its padding slots are never read.  Outside
    ``[1, B]``, or below ``B`` on MLP3_STEP1 / MLP3_STEP1_DP / MLP3_STEP_DP (which have no short
    batch): ValueError before any launch (launch_mlp3's code -15).

    ``lr_mask`` (0: ``lr_tensor`` is the one scalar): ``lr_tensor`` is a ring of ``lr_mask + 1``
    rates, a power of two, and a launch that applies the optimizer for optimizer step ``t``
    (1-based: Adam's bias-correction count, the counter behind SGD's first-step rule) reads
    ``lr_tensor[(t - 1) & lr_mask]``.  Nothing on the device writes the ring, so a captured
    graph follows a schedule the host keeps ahead of it.  MLP3_STEP1 runs its schedule
    instances; MLP3_STEP1_DP has none (MLP3_STEP_DP serves a ring): ValueError before any
    launch (code -16).  Kinds that apply no optimizer ignore it."""
    lr_mask = int(lr_mask)
    if lr_mask < 0 or lr_mask & (lr_mask + 1):
        raise ValueError(f"mlp3_launch: lr_mask must be 2^k - 1, got {lr_mask}")
    if lr_mask and (lr_tensor is None or lr_tensor.numel() < lr_mask + 1):
        raise ValueError(f"mlp3_launch: lr_mask = {lr_mask} needs lr_tensor of {lr_mask + 1} rates")
    x_scale, x_shift = check_input_affine(x_scale, x_shift)
    last_rows = check_last_rows(last_rows, B, "mlp3_launch")
    if last_rows != int(B) and kind in (MLP3_STEP1, MLP3_STEP1_DP, MLP3_STEP_DP):
        raise ValueError(f"mlp3_launch: last_rows = {last_rows} < B = {int(B)} on kind {kind}: the one-launch step "
                         "and the in-kernel exchange have no short batch (nothing was launched)")
    if kind == MLP3_STEP1_DP and (x_scale, x_shift) != (X_SCALE_DEFAULT, 0.0):
        raise ValueError("mlp3_launch: MLP3_STEP1_DP has no Normalize instance -- use MLP3_STEP_DP")
    if sgd_momentum is not None:
        if kind not in (MLP3_STEP, MLP3_TAIL_ADAM):
            raise ValueError(f"mlp3_launch: SGD arguments belong to MLP3_STEP / MLP3_TAIL_ADAM, not kind {kind}")
        if not float(sgd_momentum) >= 0.0:
            raise ValueError(f"mlp3_launch: sgd_momentum must be >= 0, got {sgd_momentum}")
        if float(sgd_momentum) != 0.0 and exp_avg is None:
            raise ValueError("mlp3_launch: SGD with momentum needs the velocity tensor (exp_avg)")
        if sgd_nesterov and (float(sgd_momentum) <= 0.0 or float(sgd_dampening) != 0.0):
            raise ValueError("mlp3_launch: Nesterov momentum requires a momentum and zero dampening")
    elif sgd_dampening or sgd_nesterov:
        raise ValueError("mlp3_launch: sgd_dampening / sgd_nesterov need sgd_momentum")
    if acc_add or acc_rows or acc_head_row is not None:
        if kind not in (MLP3_TAIL_GRAD, MLP3_TAIL_ACC):
            raise ValueError(f"mlp3_launch: accumulation arguments belong to MLP3_TAIL_GRAD / MLP3_TAIL_ACC, "
                             f"not kind {kind}")
        if acc_rows and (stats is None or (int(B) <= ONE_LAUNCH_MAX_B and acc_head_row is None)):
            raise ValueError(f"mlp3_launch: acc_rows needs stats (and acc_head_row for B <= 32), kind {kind}")
    if kind == MLP3_TAIL_ACC and (clip_part is not None or clip_out is not None or clip_max_norm
                                  or clip_nblk is not None):
        raise ValueError(f"mlp3_launch: MLP3_TAIL_ACC (kind {kind}) takes no clip arguments: its window is open")
    if clip_part is not None or clip_out is not None or clip_max_norm or clip_nblk is not None:
        if kind != MLP3_TAIL_ADAM:
            raise ValueError(f"mlp3_launch: clip arguments belong to MLP3_TAIL_ADAM, not kind {kind}")
        if clip_part is None or not clip_max_norm > 0.0:
            raise ValueError("mlp3_launch: clipping needs clip_part and clip_max_norm > 0")
    require().mlp3(
        int(kind), x_u8, labels, order, counters, int(n_batches), int(B), int(L1), int(L2), params, grads, exp_avg,
        exp_avg_sq, shadow, dh1t, xring, h1pre, act, yring, stats, bool(advance_step), float(lr), float(betas[0]),
        float(betas[1]), float(eps), float(weight_decay), float(grad_scale), lr_tensor, bool(adamw), stamps,
        [int(v) for v in (dp_ctx or ())], head_part, hand, int(dp_proto), bool(dp_loop), int(repeat),
        clip_part, float(clip_max_norm), clip_out, -1 if clip_nblk is None else int(clip_nblk),
        bool(acc_add), bool(acc_rows), acc_head_row,
        None if sgd_momentum is None else float(sgd_momentum), float(sgd_dampening), bool(sgd_nesterov),
        float(x_scale), float(x_shift), int(last_rows), lr_mask,
    )


def mlp_adam_(params, grads, exp_avg, exp_avg_sq, shadow, *, L1: int, L2: int, lr: float, step: torch.Tensor,
              betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, grad_scale: float = 1.0,
              adamw: bool = False, lr_tensor: Optional[torch.Tensor] = None) -> None:
    """Adam over the MLP arena (world size > 1, after the allreduce) + shadow refresh."""
    if use_native(params):
        require().mlp_adam(params, grads, exp_avg, exp_avg_sq, shadow, int(L1), int(L2), float(lr), float(betas[0]),
                           float(betas[1]), float(eps), float(weight_decay), float(grad_scale), bool(adamw), True,
                           step, lr_tensor)
        return
    from .optim import fused_adam_

    fused_adam_(params, grads, exp_avg, exp_avg_sq, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                grad_scale=grad_scale, adamw=adamw, step=step, lr_tensor=lr_tensor)
    mlp_refresh_shadow(params, shadow, L1, L2)


def mlp_eval(
    params: torch.Tensor,
    *,
    L1: int,
    L2: int,
    B: int,
    labels: torch.Tensor,
    out: torch.Tensor,
    x_u8: Optional[torch.Tensor] = None,
    x_f32: Optional[torch.Tensor] = None,
    index: Optional[torch.Tensor] = None,
    logits: Optional[torch.Tensor] = None,
    x_scale: float = X_SCALE_DEFAULT,
    x_shift: float = 0.0,
) -> None:
    """Forward only.  ``out`` [2]: out[0] += sum NLL, out[1] += #correct.  ``out``
    [ceil(B/32), 2]: per-32-row-chunk (sum NLL, #correct), overwritten -- the GPU
    kernel then runs one workgroup per chunk and the caller's ``out.sum(0)`` is
    deterministic.  Optional log-probs into ``logits``.  u8 mode reads a pixel as
    ``fmaf(u8, x_scale, x_shift)`` (``input_affine``)."""
    if x_u8 is not None:
        x_scale, x_shift = check_input_affine(x_scale, x_shift)
    if use_native(params):
        require().mlp_eval(x_u8, x_f32, labels, index, int(B), int(L1), int(L2), params, logits, out,
                           float(x_scale), float(x_shift))
        return
    x, y = _gather_batch(x_u8, x_f32, labels, None, 0, B, index=index, x_scale=x_scale, x_shift=x_shift)
    with torch.no_grad():
        logp = F.log_softmax(_reference_forward(mlp_unpack(params, L1, L2), x), dim=1)
        nll = F.nll_loss(logp, y, reduction="none")
        hit = (logp.argmax(dim=1) == y).float()
        if out.dim() == 2:
            pad = out.size(0) * 32 - B
            out[:, 0] = F.pad(nll, (0, pad)).view(-1, 32).sum(1)
            out[:, 1] = F.pad(hit, (0, pad)).view(-1, 32).sum(1)
        else:
            out[0] += nll.sum()
            out[1] += hit.sum()
        if logits is not None:
            logits.view(B, NUM_CLASSES).copy_(logp)


def init_mlp_params(L1: int, L2: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """nn.Linear default init (kaiming_uniform(a=sqrt(5)) == U(+-1/sqrt(fan_in))) into a flat arena."""
    flat = torch.empty(mlp_param_count(L1, L2), dtype=torch.float32)
    views = mlp_unpack(flat, L1, L2)
    fans = {"layer_1": IN_FEATURES, "layer_2": L1, "layer_3": L2}
    for name, t in views.items():
        bound = 1.0 / math.sqrt(fans[name.split(".")[0]])
        t.uniform_(-bound, bound, generator=generator)
    return flat
