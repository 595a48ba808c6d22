"""Convolutions on NHWC bf16 activations, the backend chosen per operation and shape.

Every ResNet-50 convolution goes through this file: the stride-1 1x1 layers
(``Conv1x1NHWC`` / ``_Conv1x1Fn``), the KxK and strided layers (``conv_nhwc`` /
``_ConvNHWCFn``) and the 7x7 stem (``stem_conv`` / ``_StemFn``), each forward, input
gradient (dgrad) and weight gradient (wgrad; fp32, the master weight's gradient).
The backends are the in-tree MFMA kernels (``*_hip``), a hipBLASLt GEMM and MIOpen.

A 1x1 convolution over a channels_last tensor IS a GEMM on the [N*H*W, C] view:

  forward  y[M, Cout]  = x[M, Cin]  . W^T
  dgrad    dx[M, Cin]  = dy[M, Cout] . W
  wgrad    dW[Cout, Cin] = dy^T . x

MIOpen runs these as convolutions; for ResNet-50's shapes it is the faster choice
for some (e.g. the wgrad of the large 56x56 layers) and far slower for others: its
wgrad costs ~80 us whatever the size (zero-fill + split-K atomics + a bf16->fp32
cast, profiles/r3_rn50/kernel_stats_rn50_steady.csv) and its forward of the
14x14 / 7x7 layers runs 2-5x a hipBLASLt GEMM (profiles/r3_rn50/conv1x1_probe_perop.log).
So every (operation, shape) picks its backend once, timed on the device at first
use (like cudnn.benchmark): each operation builds ONE table ``{name: callable}``,
``_pick`` names the winner and that table's callable runs.  ``RLA_CONV1X1`` and
``RLA_CONV_WGRAD`` pin a backend by its name in the table (``miopen|gemm|hip|...``),
``RLA_CONV3X3S2_DGRAD`` that of the stride-2 3x3 input gradient (``_pick_dgrad_s2``).

Around the convolutions themselves:

* ``GradFork``: two convolutions reading one tensor sum their input gradients in place;
* ``BNStats``: a forward whose kernel has the BatchNorm statistics of its output in
  the epilogue hands them to that BatchNorm, which then skips its own pass;
* deferred BatchNorm (ops/bn.py DeferredApply, ``pre``): the input is a BatchNorm +
  ReLU's *input* and the forward and weight-gradient kernels apply the map to
  their operands, so the activation is never written.

``Conv1x1NHWC`` is a drop-in ``nn.Conv2d(cin, cout, 1, bias=False)`` (same
parameter and state-dict key); anything outside the fast path (CPU, fp32, NCHW,
odd alignment) runs the stock convolution.
"""
from __future__ import annotations

import functools
import os
from typing import Callable, Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

# keyed by (op, M, Cin, Cout) for the 1x1 layers, (op, M, Cin, Cout, KH, KW, stride, pad) for KxK
_choice: Dict[Tuple, str] = {}
_timings: Dict[Tuple, Dict[str, float]] = {}
stats = {"fast": 0, "fallback": 0, "bn_dgrad_fused": 0, "bn_dgrad_fused_3x3": 0, "stem": 0, "pre_applied": 0}


def _mode() -> str:
    return os.environ.get("RLA_CONV1X1", "auto")


def _wmode() -> str:
    """``RLA_CONV_WGRAD``: backend of the weight gradients (auto: timed per shape)."""
    return os.environ.get("RLA_CONV_WGRAD", "auto")


_REPS = 3
_DETERMINISTIC_ORDER = ("hip", "hip_gen", "gemm", "miopen")


def _time(fn, reps: int = _REPS) -> float:
    """Device time of ``reps`` calls.  The device is held by a spin kernel while the
    host enqueues them, so the calls run back to back: a backend's host-side cost
    (MIOpen's is tens of us per call) is hidden, as it is inside a GPU-bound step --
    timing an idle device would charge it to the kernels."""
    fn()  # warm: library kernel load / solver search
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(2_000_000)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def _pick(op: str, key: Tuple[int, ...], cands) -> str:
    mode = _mode()
    if op.startswith("wgrad"):
        # RLA_CONV_WGRAD picks the weight-gradient backend; RLA_CONV1X1=miopen|gemm
        # still pins the 1x1 layers' wgrad when it is left on auto
        mode = _wmode() if _wmode() != "auto" or op != "wgrad" else mode
    if mode in cands:
        return mode
    if torch.are_deterministic_algorithms_enabled():
        # Trainer(deterministic=True): no timing (two runs could pick different
        # kernels that round differently), and never MIOpen's split-K-atomic wgrad:
        # the MFMA kernel (fixed-order split reduction), else the GEMM
        for name in _DETERMINISTIC_ORDER:
            if name in cands:
                return name
    return _timed_pick((op,) + key, cands)


def _timed_pick(k: Tuple, cands) -> str:
    """The cached pick of ``k`` = (op, *key), timing ``cands`` on the device at first use."""
    c = _choice.get(k)
    if c is None and torch.cuda.is_current_stream_capturing():
        return "miopen"  # no timing inside a graph capture (it synchronises)
    if c is None:
        # two rounds, each candidate's best: one noisy window (MIOpen's first calls
        # of a shape vary by 2x on a fresh box) must not decide the backend
        t = {name: _time(fn, _REPS) for name, fn in cands.items()}
        for name, fn in cands.items():
            t[name] = min(t[name], _time(fn, _REPS))
        c = min(t, key=t.get)
        _choice[k] = c
        _timings[k] = {name: round(v * 1e3 / _REPS, 1) for name, v in t.items()}  # device us per call
    return c


def choices() -> Dict[str, Dict[str, float]]:
    """The autotuned backends so far: ``"op M Cin Cout" -> {backend: us, ..., "pick": name}``."""
    return {" ".join(map(str, k)): dict(_timings.get(k, {}), pick=c) for k, c in _choice.items()}


def _run(op: str, key: Tuple[int, ...], cands: Dict[str, Callable]):
    """The result of ``op``'s picked backend: the callable that ``_pick`` timed, run once more."""
    return cands[_pick(op, key, cands)]()


def _run_stats(op: str, key: Tuple[int, ...], cands: Dict[str, Callable], fused: str, bn_stats: "BNStats"):
    """``_run`` for a forward whose output a training BatchNorm reads: ``cands[fused]``
    returns (y, part) from a statistics epilogue and hands ``part`` to that BatchNorm;
    the others return y alone and BatchNorm then runs its own partial pass, so they
    are timed with that pass (and run without it)."""
    timed = {name: fn if name == fused else (lambda fn=fn: _bn_partial(fn())) for name, fn in cands.items()}
    name = _pick(op, key, timed)
    if name != fused:
        return cands[name]()
    y, bn_stats.part = cands[name]()
    return y


# the library calls, one spelling each (stride / padding as pairs; dilation 1, groups 1, no bias)

def _miopen_fwd(x: torch.Tensor, w4: torch.Tensor, stride=(1, 1), padding=(0, 0)) -> torch.Tensor:
    return torch.ops.aten.convolution(x, w4, None, list(stride), list(padding), [1, 1], False, [0, 0], 1)


def _miopen_bwd(dy: torch.Tensor, x: torch.Tensor, w4: torch.Tensor, stride, padding, need_dx: bool, need_dw: bool):
    """(dx, dw) of one MIOpen call, None where not asked for; dw in fp32 (MIOpen's is bf16)."""
    dx, dw = torch.ops.aten.convolution_backward(dy, x, w4, None, list(stride), list(padding), [1, 1], False, [0, 0],
                                                 1, [need_dx, need_dw, False])[:2]
    return dx, (dw.float() if need_dw else None)


def _gemm_fwd(x2: torch.Tensor, wb: torch.Tensor) -> torch.Tensor:
    return torch.mm(x2, wb.t())


def _gemm_dgrad(dy2: torch.Tensor, wb: torch.Tensor) -> torch.Tensor:
    return torch.mm(dy2, wb)


def _gemm_wgrad(dy2: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    return torch.ops.aten.mm.dtype(dy2.t(), x2, torch.float32)  # fp32 straight from the GEMM: no cast kernel


def wgrad_ok(cin: int, cout: int) -> bool:
    """Shapes the MFMA weight-gradient kernel covers (csrc/conv_wgrad.hip)."""
    return cin % 64 == 0 and cout % 64 == 0 and os.environ.get("RLA_CONV_WGRAD", "auto") != "off"


def wgrad_hip(dy: torch.Tensor, x: torch.Tensor, kernel_size, stride, padding, splits: int = 0,
              algo: int = 0, pre_ss: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient of an NHWC bf16 convolution on the MFMA kernel: ``dy`` [N, Cout,
    OH, OW] and ``x`` [N, Cin, H, W], both channels_last bf16; returns the fp32
    gradient [Cout, Cin, KH, KW] with channels_last strides (the kernel writes the
    [Cout, KH, KW, Cin] memory order directly).  ``algo`` 0: the 3x3 / stride-1 /
    pad-1 halo kernel where it applies, else the generic one; 1: always generic.
    ``pre_ss`` (either kernel, any geometry): ``x`` is a deferred BatchNorm + ReLU's input
    and the kernel stages relu(x * scale + shift) inside the image, zero in the padding
    (ops/bn.py DeferredApply)."""
    from . import require

    n, cin, h, w = x.shape
    cout, oh, ow = dy.size(1), dy.size(2), dy.size(3)
    kh, kw = kernel_size
    out = require().conv_wgrad(dy.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1), n, h, w, cin, oh, ow, cout, kh, kw,
                               stride[0], stride[1], padding[0], padding[1], splits, algo, pre_ss)
    return out.permute(0, 3, 1, 2)


def conv3x3_ok(x: torch.Tensor, wb: torch.Tensor, stride, padding) -> bool:
    """3x3 / stride 1 / pad 1 layers the MFMA convolution kernel covers (csrc/conv3x3.hip)."""
    if tuple(wb.shape[2:]) != (3, 3) or tuple(stride) != (1, 1) or tuple(padding) != (1, 1):
        return False
    if os.environ.get("RLA_CONV3X3", "auto") == "off":
        return False
    n, cin, h, w = x.shape
    cout = wb.size(0)
    return (cin % 64 == 0 and cout % 64 == 0 and wb.is_contiguous(memory_format=torch.channels_last)
            and _conv3x3_shape_ok(n, h, w, cin, cout))


@functools.lru_cache(maxsize=256)
def _bn_bwd_shape_ok(m: int, k: int, n: int) -> bool:
    from . import require

    return bool(require().conv1x1_bn_bwd_ok(m, k, n))


def _conv3x3_shape_ok(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    # not cached here, see _conv3x3s2_shape_ok
    from . import require

    return bool(require().conv3x3_supported(n, h, w, cin, cout))


def conv3x3_hip(x: torch.Tensor, wb: torch.Tensor) -> torch.Tensor:
    """``conv2d(x, wb, stride=1, padding=1)`` on the MFMA kernel: ``x`` [N, Cin, H, W]
    channels_last bf16, ``wb`` [Cout, Cin, 3, 3] channels_last bf16 (its memory IS the
    kernel's [Cout][3][3][Cin]); returns [N, Cout, H, W] channels_last."""
    from . import require

    n, cin, h, w = x.shape
    cout = wb.size(0)
    y = require().conv3x3(x.permute(0, 2, 3, 1), wb.permute(0, 2, 3, 1), n, h, w, cin, cout)
    return y.permute(0, 3, 1, 2)


def conv3x3_stats_hip(x: torch.Tensor, wb: torch.Tensor, pre=None):
    """:func:`conv3x3_hip` plus the per-channel partial sums of its bf16 output from the
    epilogue (csrc/conv3x3.hip ST): returns (y channels_last, part [rows, 2, Cout]).
    ``pre`` (ops/bn.py DeferredApply): ``x`` is that BatchNorm's input and the kernel
    convolves relu(x * scale + shift), with zero padding (csrc/conv3x3.hip PRE)."""
    from . import require

    n, cin, h, w = x.shape
    cout = wb.size(0)
    pre_args = () if pre is None else (pre.st, pre.take_nbt())
    y, part = require().conv3x3_stats(x.permute(0, 2, 3, 1), wb.permute(0, 2, 3, 1), n, h, w, cin, cout, *pre_args)
    return y.permute(0, 3, 1, 2), part


class _TimingPre:
    """A DeferredApply stand-in for timing candidates: same statistics, no
    num_batches_tracked increment."""

    __slots__ = ("st",)

    def __init__(self, pre):
        self.st = pre.st

    def take_nbt(self):
        return None


def _applied(x: torch.Tensor, pre) -> torch.Tensor:
    """relu(x * scale + shift) by the apply kernel (a timing candidate: no autograd)."""
    from . import require

    y = torch.empty_like(x, memory_format=torch.channels_last)
    require().bn_apply(x.permute(0, 2, 3, 1), pre.st[2], pre.st[3], None, True, y.permute(0, 2, 3, 1))
    return y


def conv3x3_stats_enabled() -> bool:
    """``RLA_CONV3X3_STATS=off`` keeps the 3x3 forward's BatchNorm statistics in BN's own pass."""
    return os.environ.get("RLA_CONV3X3_STATS", "auto") != "off"


def conv3x3_dgrad_hip(dy: torch.Tensor, wb: torch.Tensor) -> torch.Tensor:
    """Input gradient of a 3x3 / stride 1 / pad 1 convolution = the same convolution
    of ``dy`` with the weight flipped in both taps and transposed in channels; the
    kernel reads the forward weight that way itself (no re-layout kernel)."""
    from . import require

    n, cout, h, w = dy.shape
    cin = wb.size(1)
    dx = require().conv3x3(dy.permute(0, 2, 3, 1), wb.permute(0, 2, 3, 1), n, h, w, cout, cin, True)
    return dx.permute(0, 3, 1, 2)


def conv3x3_dgrad_bn_hip(dy: torch.Tensor, wb: torch.Tensor, xb: torch.Tensor, ss: torch.Tensor):
    """:func:`conv3x3_dgrad_hip` with the PRECEDING BatchNorm + ReLU's backward in the
    epilogue (csrc/conv3x3.hip BWD): ``xb`` [N, Cin, H, W] channels_last bf16 is that
    BatchNorm's input and ``ss`` its [4, Cin] forward statistics.  Returns (d channels_last,
    part [rows, 2, Cin]): d = dx where xb * scale + shift > 0, else 0 -- bitwise what the
    BatchNorm's own recomputed-mask passes see -- and the fixed-order partial sums of d and
    d * xb that ``bn_bwd_finalize`` reads."""
    from . import require

    n, cout, h, w = dy.shape
    cin = wb.size(1)
    d, part = require().conv3x3_dgrad_bn(dy.permute(0, 2, 3, 1), wb.permute(0, 2, 3, 1), n, h, w, cout, cin,
                                         xb.permute(0, 2, 3, 1), ss)
    return d.permute(0, 3, 1, 2), part


def fuse_bn_dgrad_3x3_mode() -> str:
    """``RLA_FUSE_BN_DGRAD_3X3``: a 3x3 / stride-1 conv marked ``fuse_bn_dgrad`` (ResNet's
    bottleneck conv2, the only reader of bn1's output) computes that BatchNorm's backward
    mask and partial sums in its input-gradient epilogue.  ``0``: never; ``1``: wherever
    the kernel covers the shape; ``auto`` (default): per shape, whichever of the fused
    kernel and the plain input gradient + BatchNorm's own partial pass is faster
    (``dgrad_kxk_bn`` in :func:`choices`)."""
    m = os.environ.get("RLA_FUSE_BN_DGRAD_3X3", "auto")
    return m if m in ("0", "1") else "auto"


def _dgrad_bn_shape_ok(n: int, h: int, w: int, cr: int, co: int) -> bool:
    # not cached here, see _conv3x3s2_shape_ok
    from . import require

    return bool(require().conv3x3_dgrad_bn_ok(n, h, w, cr, co))


def _fold_3x3_ok(fold, x: torch.Tensor, wb: torch.Tensor) -> bool:
    """The producer BatchNorm left its input and statistics (ops/bn.py _FoldSlot.xin / st)
    and the fused input-gradient kernel covers the layer."""
    xin, st = getattr(fold, "xin", None), getattr(fold, "st", None)
    if xin is None or st is None or fuse_bn_dgrad_3x3_mode() == "0":
        return False
    n, cin, h, w = x.shape
    return (xin.shape == x.shape and xin.dtype == torch.bfloat16 and xin.is_cuda
            and xin.is_contiguous(memory_format=torch.channels_last) and xin.data_ptr() % 16 == 0
            and st.dtype == torch.float32 and tuple(st.shape) == (4, cin) and st.is_contiguous()
            and _dgrad_bn_shape_ok(n, h, w, wb.size(0), cin))


def _pick_dgrad_bn(key: Tuple[int, ...], dy: torch.Tensor, wb: torch.Tensor, fold) -> str:
    """``fused`` or ``split`` for a 3x3 input gradient whose input is a fold-carrying
    BatchNorm + ReLU output (both fixed-order, so deterministic mode takes ``fused``
    untimed; a graph capture with no cached pick takes ``split``)."""
    mode = fuse_bn_dgrad_3x3_mode()
    if mode == "1" or torch.are_deterministic_algorithms_enabled():
        return "fused"
    from . import require

    xin, st = fold.xin, fold.st

    def split():
        da = conv3x3_dgrad_hip(dy, wb)
        return da, require().bn_partial(xin.permute(0, 2, 3, 1), None, da.permute(0, 2, 3, 1), xin.size(1), 1, True,
                                        None, None, st, None)

    cands = {"fused": lambda: conv3x3_dgrad_bn_hip(dy, wb, xin, st), "split": split}
    be = _pick("dgrad_kxk_bn", key, cands)
    return be if be in cands else "split"  # _pick's capture answer names no candidate here


def conv3x3s2_ok(x: torch.Tensor, wb: torch.Tensor, stride, padding) -> bool:
    """3x3 / stride 2 / pad 1 forwards the MFMA kernel covers (csrc/conv3x3s2.hip): bf16
    channels_last operands on the GPU, Cin % 16 == 0, Cout % 64 == 0 and a tile halo that
    fits its LDS image.  ``RLA_CONV3X3=off`` turns this kernel off too."""
    if tuple(wb.shape[2:]) != (3, 3) or tuple(stride) != (2, 2) or tuple(padding) != (1, 1):
        return False
    if not x.is_cuda or os.environ.get("RLA_CONV3X3", "auto") == "off":
        return False
    n, cin, h, w = x.shape
    cout = wb.size(0)
    return (cin % 16 == 0 and cout % 64 == 0 and x.dtype == torch.bfloat16 and wb.dtype == torch.bfloat16
            and x.is_contiguous(memory_format=torch.channels_last)
            and wb.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0 and wb.data_ptr() % 16 == 0
            and _conv3x3s2_shape_ok(n, h, w, cin, cout))


def _conv3x3s2_shape_ok(n: int, h: int, w: int, cin: int, cout: int) -> bool:
    # The three 3x3 predicates (this one, _conv3x3_shape_ok, _dgrad_bn_shape_ok) are not
    # cached here: the answer follows the work split, hence the planning CU count
    # (set_plan_cus) and RLA_CONV3X3_TM, and must be the one the launch will give.  The
    # binding builds the launch's own geometry and keeps every partition walk it has made.
    from . import require

    return bool(require().conv3x3s2_supported(n, h, w, cin, cout))


def conv3x3s2_hip(x: torch.Tensor, wb: torch.Tensor) -> torch.Tensor:
    """``conv2d(x, wb, stride=2, padding=1)`` on the MFMA kernel: ``x`` [N, Cin, H, W]
    channels_last bf16, ``wb`` [Cout, Cin, 3, 3] channels_last bf16; returns
    [N, Cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1] channels_last."""
    from . import require

    n, cin, h, w = x.shape
    cout = wb.size(0)
    y = require().conv3x3s2(x.permute(0, 2, 3, 1), wb.permute(0, 2, 3, 1), n, h, w, cin, cout)
    return y.permute(0, 3, 1, 2)


def conv3x3s2_stats_hip(x: torch.Tensor, wb: torch.Tensor):
    """:func:`conv3x3s2_hip` plus the per-channel partial sums of its bf16 output from the
    epilogue (csrc/conv3x3s2.hip ST): returns (y channels_last, part [rows, 2, Cout])."""
    from . import require

    n, cin, h, w = x.shape
    cout = wb.size(0)
    y, part = require().conv3x3s2_stats(x.permute(0, 2, 3, 1), wb.permute(0, 2, 3, 1), n, h, w, cin, cout)
    return y.permute(0, 3, 1, 2), part


def conv3x3s2_dgrad_ok(dy: torch.Tensor, wb: torch.Tensor, h: int, w: int) -> bool:
    """Input gradients of a 3x3 / stride 2 / pad 1 layer with an [h, w] input the MFMA kernel
    covers (csrc/conv3x3s2_dgrad.hip): ``dy`` [N, Cout, OH, OW] and the forward weight ``wb``
    [Cout, Cin, 3, 3], both bf16 channels_last on the GPU and 16-byte aligned, Cout % 16 == 0,
    Cin % 64 == 0 and a tile halo that fits its LDS image.  ``RLA_CONV3X3=off`` turns this
    kernel off too."""
    if dy.dim() != 4 or wb.dim() != 4 or tuple(wb.shape[2:]) != (3, 3):
        return False
    if not dy.is_cuda or not wb.is_cuda or os.environ.get("RLA_CONV3X3", "auto") == "off":
        return False
    n, cout, oh, ow = dy.shape
    cin = wb.size(1)
    return (wb.size(0) == cout and (oh, ow) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
            and cout % 16 == 0 and cin % 64 == 0 and dy.dtype == torch.bfloat16 and wb.dtype == torch.bfloat16
            and dy.is_contiguous(memory_format=torch.channels_last)
            and wb.is_contiguous(memory_format=torch.channels_last)
            and dy.data_ptr() % 16 == 0 and wb.data_ptr() % 16 == 0
            and _conv3x3s2_dgrad_shape_ok(n, h, w, cout, cin))


def _conv3x3s2_dgrad_shape_ok(n: int, h: int, w: int, cr: int, co: int) -> bool:
    # not cached here, see _conv3x3s2_shape_ok
    from . import require

    return bool(require().conv3x3s2_dgrad_supported(n, h, w, cr, co))


def conv3x3s2_dgrad_hip(dy: torch.Tensor, wb: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """Input gradient of ``conv2d(x, wb, stride=2, padding=1)`` for an [h, w] input on the MFMA
    kernel: ``dy`` [N, Cout, OH, OW] channels_last bf16, ``wb`` the forward weight [Cout, Cin,
    3, 3] channels_last bf16, read as it lies in memory; returns [N, Cin, h, w] channels_last,
    every element written once (fixed order: bitwise reproducible)."""
    from . import require

    n, cout = dy.size(0), dy.size(1)
    cin = wb.size(1)
    dx = require().conv3x3s2_dgrad(dy.permute(0, 2, 3, 1), wb.permute(0, 2, 3, 1), n, h, w, cout, cin)
    return dx.permute(0, 3, 1, 2)


def _s2_dgrad_mode() -> str:
    """``RLA_CONV3X3S2_DGRAD=auto|hip|miopen``: backend of the stride-2 3x3 input gradient
    (auto: timed per shape; deterministic mode: the in-tree kernel)."""
    m = os.environ.get("RLA_CONV3X3S2_DGRAD", "auto")
    return m if m in ("hip", "miopen") else "auto"


def _pick_dgrad_s2(key: Tuple[int, ...], cands) -> str:
    """``hip`` or ``miopen`` for a 3x3 / stride-2 input gradient (``dgrad_s2`` in
    :func:`choices`).  The in-tree kernel runs in a fixed order, so deterministic mode takes
    it untimed; a graph capture with no cached pick takes ``miopen``."""
    mode = _s2_dgrad_mode()
    if mode in cands:
        return mode
    if torch.are_deterministic_algorithms_enabled():
        return "hip"
    return _timed_pick(("dgrad_s2",) + key, cands)


def _nhwc2d(t: torch.Tensor) -> torch.Tensor:
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c)


def _from2d(t2: torch.Tensor, n: int, h: int, w: int) -> torch.Tensor:
    return t2.view(n, h, w, t2.size(1)).permute(0, 3, 1, 2)


class GradFork:
    """Two convolutions reading the SAME input (a bottleneck's conv1 and its
    downsample conv): their input gradients meet in ONE tensor instead of two
    tensors and an autograd add kernel (``CUDAFunctor_add<bf16>``,
    ~200 us per ResNet-50 step).  Whichever backward runs first parks its full dgrad
    here and returns None for the input; the second accumulates its contribution
    INTO that tensor -- a GEMM with beta = 1 (stride 1), or a GEMM on the
    subsampled rows plus an add into every s-th pixel only (stride s > 1) -- and
    returns the sum.  Order-independent; autograd sees None + sum.  Only when BOTH
    consumers took a fast path (each registers in its forward): with one consumer on a
    stock fallback, the fast one returns its own gradient and autograd adds as usual."""

    __slots__ = ("dx", "users")

    def __init__(self):
        self.dx: Optional[torch.Tensor] = None
        self.users = 0


def _fork_dx(fork: Optional[GradFork], full, accumulate) -> Optional[torch.Tensor]:
    """``full()``: this op's dgrad as a new tensor; ``accumulate(d)``: add it into ``d``."""
    if fork is None or fork.users < 2:
        return full()
    if fork.dx is None:
        fork.dx = full()
        return None
    d, fork.dx = fork.dx, None
    if accumulate is None:
        d.add_(full())  # no fused form for this op: a plain add (still one tensor less)
    else:
        accumulate(d)
    return d


def _acc_dgrad(d: torch.Tensor, dy2: torch.Tensor, wb: torch.Tensor) -> None:
    """d += dy . W for a stride-1 1x1 conv: in the GEMM (beta = 1) on d's NHWC view."""
    if d.permute(0, 2, 3, 1).is_contiguous():
        _nhwc2d(d).addmm_(dy2, wb)
    else:
        d.add_(_from2d(_gemm_dgrad(dy2, wb), d.size(0), d.size(2), d.size(3)))


class BNStats:
    """Hand-off of a convolution's epilogue BatchNorm statistics to the BatchNorm that
    consumes its output: the conv fills ``part`` ([rows, 2, C] fp32 partial sums of
    its bf16 output, ``bn_finalize``'s layout) when its backend computed them, and
    ``BatchNormAct2d`` then skips its own partial pass over the output."""

    __slots__ = ("part",)

    def __init__(self):
        self.part: Optional[torch.Tensor] = None


def conv1x1_stats_ok(m: int, cin: int, cout: int) -> bool:
    """Shapes of the 1x1 MFMA forward with BatchNorm statistics (csrc/conv1x1.hip)."""
    return os.environ.get("RLA_CONV1X1_STATS", "auto") != "off" and _conv1x1_stats_shape_ok(m, cin, cout)


@functools.lru_cache(maxsize=256)
def _conv1x1_stats_shape_ok(m: int, k: int, n: int) -> bool:
    from . import require

    return bool(require().conv1x1_stats_ok(m, k, n))


def conv1x1_stats_hip(x: torch.Tensor, wb: torch.Tensor, pre=None):
    """``conv2d(x, wb)`` for a 1x1 / stride-1 layer on the MFMA kernel, plus the
    per-channel partial sums of its bf16 output: ``x`` [N, Cin, H, W] channels_last
    bf16, ``wb`` [Cout, Cin] bf16.  Returns (y channels_last, part [rows, 2, Cout]).
    ``pre`` (ops/bn.py DeferredApply): ``x`` is that BatchNorm's input and the kernel
    convolves relu(x * scale + shift) instead."""
    from . import require

    n, _, h, w = x.shape
    pre_args = () if pre is None else (pre.st, pre.take_nbt())
    y2, part = require().conv1x1_stats(_nhwc2d(x), wb, *pre_args)
    return _from2d(y2, n, h, w), part


def conv1x1_pre_ok(m: int, cin: int, cout: int) -> bool:
    """Where a 1x1 conv applies a deferred BatchNorm + ReLU in its own kernels (forward
    and weight gradient): K <= 128, the shapes whose forward runs on the in-tree kernel
    anyway (profiles/r5_pair/rn50_graph.log ``fwd_st``; at K >= 256 the library GEMM +
    the apply pass is faster)."""
    return cin <= 128 and conv1x1_stats_ok(m, cin, cout) and wgrad_ok(cin, cout)


def fuse_bn_dgrad_enabled() -> bool:
    """A 1x1 conv marked ``fuse_bn_dgrad`` (ResNet's identity-block conv1, whose input
    y is a residual BatchNorm+ReLU's output with no other autograd consumer: the
    identity shortcut's gradient is folded) computes that BatchNorm's backward partial
    in its input-gradient kernel (csrc/conv1x1.hip BWD): d = (dx + dy2) * (y > 0) is
    written once and the plain input gradient is never materialised.
    ``RLA_FUSE_BN_DGRAD=0`` turns it off (same-box A/B: +0.5 %, profiles/r4_c1)."""
    return os.environ.get("RLA_FUSE_BN_DGRAD", "1") == "1"


def _bn_partial(y: torch.Tensor) -> torch.Tensor:
    from . import require

    return require().bn_partial(y.permute(0, 2, 3, 1), None, None, y.size(1), 0, False, None)


class _Conv1x1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, shadow=None, fork=None, bn_stats=None, fuse_bn=False, pre=None):
        n, cin, h, w = x.shape
        cout = weight.size(0)
        # the arena's bf16 shadow (ops/shadow.py) when there is one: no cast kernel
        wb = (shadow if shadow is not None else weight.detach().to(torch.bfloat16)).reshape(cout, cin)
        x2 = _nhwc2d(x)
        key = (x2.size(0), cin, cout)
        w4 = wb.view(cout, cin, 1, 1)
        ctx.pre_st = pre.st if pre is not None else None
        cands = {
            "gemm": lambda: _from2d(_gemm_fwd(x2, wb), n, h, w),
            "miopen": lambda: _miopen_fwd(x, w4),
        }
        if pre is not None:
            # x is a deferred BatchNorm + ReLU's input (ops/bn.py DeferredApply): the
            # kernels apply its map to their operands; the caller checked conv1x1_pre_ok
            # (and passes no fork and no fuse_bn)
            y, part = conv1x1_stats_hip(x, wb, pre)
            if bn_stats is not None:
                bn_stats.part = part
        elif bn_stats is not None and conv1x1_stats_ok(x2.size(0), cin, cout):
            # the next BatchNorm's statistics: in this GEMM's epilogue, or the library
            # forward + BN's own partial pass -- whichever is faster for the shape
            y = _run_stats("fwd_st", key, {"hip": lambda: conv1x1_stats_hip(x, wb), **cands}, "hip", bn_stats)
        else:
            y = _run("fwd", key, cands)
        ctx.save_for_backward(x, wb)
        ctx.key = key
        ctx.fork = fork
        if fork is not None:
            fork.users += 1
        # x is a residual BatchNorm+ReLU's output (its fold slot carries that layer's
        # input): the input gradient may absorb the BatchNorm's backward partial
        fold = getattr(x, "_rla_fold", None)
        ctx.fold = fold if (fuse_bn and fork is None and fold is not None and getattr(fold, "x3", None) is not None
                            and fuse_bn_dgrad_enabled()
                            and _bn_bwd_shape_ok(x2.size(0), cout, cin)) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        n, cin, h, w = x.shape
        cout = wb.size(0)
        dy = dy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy2, x2 = _nhwc2d(dy), _nhwc2d(x)
        w4 = wb.view(cout, cin, 1, 1)
        geo = ((1, 1), (0, 0))  # stride, padding
        st = ctx.pre_st  # x is a deferred BatchNorm + ReLU's input: no fork, no fold
        dgrad = {
            "gemm": lambda: _from2d(_gemm_dgrad(dy2, wb), n, h, w),
            "miopen": lambda: _miopen_bwd(dy, x, w4, *geo, True, False)[0],
        }
        wgrad = {
            "gemm": lambda: _gemm_wgrad(dy2, x2).view(cout, cin, 1, 1),
            "miopen": lambda: _miopen_bwd(dy, x, w4, *geo, False, True)[1],
        }
        if wgrad_ok(cin, cout) or st is not None:
            wgrad["hip"] = lambda: wgrad_hip(dy, x, (1, 1), *geo, pre_ss=st)
        dx = dw = None
        be_d = be_w = None
        fork = ctx.fork if ctx.needs_input_grad[0] else None
        fold = ctx.fold
        if fold is not None and fold.dres is not None and ctx.needs_input_grad[0]:
            # d = (dy . W + dres_next) * (x > 0) and its BatchNorm partial sums in one
            # kernel; the producer BatchNorm's backward takes d as its dy
            from . import require
            from .bn import fold_stats

            d2, part = require().conv1x1_bn_bwd(dy2, wb.t().contiguous(), _nhwc2d(fold.dres), x2,
                                                _nhwc2d(fold.x3))
            fold.dres, fold.bwd_part = None, part
            fold_stats["folded"] += 1
            stats["bn_dgrad_fused"] += 1
            dx = _from2d(d2, n, h, w)
            fold.bwd_d = dx  # bn backward checks it receives exactly this tensor
        elif fork is not None and fork.users >= 2 and fork.dx is not None:
            # second of a forked pair: dx += dy . W in the GEMM itself (beta = 1)
            dx = _fork_dx(fork, None, lambda d: _acc_dgrad(d, dy2, wb))
        elif ctx.needs_input_grad[0]:
            be_d = _pick("dgrad", ctx.key, dgrad)
        if ctx.needs_input_grad[1]:
            # deferred-BatchNorm input: the input gradient (w.r.t. the activation) does not
            # read x; the weight gradient stages relu(x * scale + shift), on the MFMA kernel only
            be_w = "hip" if st is not None else _pick("wgrad", ctx.key, wgrad)
        if be_d == "miopen" and be_w == "miopen" and fork is None:
            # both from MIOpen: one call (its host cost is tens of us per call)
            dx, dw = _miopen_bwd(dy, x, w4, *geo, True, True)
        else:
            if be_d is not None:
                dx = _fork_dx(fork, dgrad[be_d], None)
            if be_w is not None:
                dw = wgrad[be_w]()
        return dx, dw, None, None, None, None, None


def fast_ok(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 and x.numel() > 0
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0
            and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and x.size(1) % 8 == 0 and conv.out_channels % 8 == 0)


class Conv1x1NHWC(nn.Conv2d):
    """``nn.Conv2d(cin, cout, 1, bias=False)`` with per-operation MIOpen / GEMM backends."""

    _rla_reads_bf16_shadow = True

    def __init__(self, in_channels: int, out_channels: int, device=None, dtype=None):
        super().__init__(in_channels, out_channels, 1, 1, 0, bias=False, device=device, dtype=dtype)
        # set by a model whose structure makes this layer its input's only autograd
        # consumer (see fuse_bn_dgrad_enabled)
        self.fuse_bn_dgrad = False

    def forward(self, x: torch.Tensor, fork: Optional[GradFork] = None,
                bn_stats: Optional[BNStats] = None) -> torch.Tensor:
        """``bn_stats``: the BatchNorm reading this output is training on batch
        statistics -- let this layer compute them where that is faster (BNStats)."""
        pre = getattr(x, "_rla_pre", None)
        if pre is not None:
            # a deferred BatchNorm + ReLU output (ops/bn.py DeferredApply): applied in this
            # conv's kernels where the shape allows, else materialised here
            from .bn import materialize

            if (fork is None and fast_ok(x, self) and _mode() != "off" and not pre.used
                    and conv1x1_pre_ok(x.size(0) * x.size(2) * x.size(3), x.size(1), self.out_channels)):
                pre.used = True
                stats["fast"] += 1
                stats["pre_applied"] += 1
                from .shadow import bf16_weight

                return _Conv1x1Fn.apply(x, self.weight, bf16_weight(self.weight), None, bn_stats, False, pre)
            x = materialize(x)
        if torch.is_autocast_enabled("cuda") and x.is_cuda and x.dtype == torch.float32:
            x = x.to(torch.bfloat16)
        if fast_ok(x, self) and _mode() != "off":
            stats["fast"] += 1
            from .shadow import bf16_weight

            return _Conv1x1Fn.apply(x, self.weight, bf16_weight(self.weight), fork, bn_stats, self.fuse_bn_dgrad)
        stats["fallback"] += 1
        return F.conv2d(x, self.weight)


class _ConvNHWCFn(torch.autograd.Function):
    """KxK (or strided) bf16 NHWC convolution: MIOpen or, for 3x3 / stride 1 / pad 1, the
    MFMA kernels for the forward and dgrad, for 3x3 / stride 2 / pad 1 the MFMA forward
    and the MFMA quad-tiled dgrad (``conv3x3s2_dgrad_hip``; ``dgrad_s2``, picked by
    ``_pick_dgrad_s2``: the in-tree kernel untimed in deterministic mode); the weight
    gradient from MIOpen or the MFMA kernel (``wgrad_hip``); each picked per shape on device
    time.  The weight gradient reaches the fp32 master weight in fp32."""

    @staticmethod
    def forward(ctx, x, weight, wb, stride, padding, fork=None, bn_stats=None, pre=None, fold=None):
        ctx.pre_st = pre.st if pre is not None else None
        ctx.c3 = pre is not None or conv3x3_ok(x, wb, stride, padding)
        ctx.s2 = False  # the stride-2 forward predicate held (gates the in-tree input gradient)
        # fold: the _FoldSlot of the BatchNorm + ReLU (no residual) whose output x is -- or,
        # with pre, stands for -- and which no one else reads: the input gradient may
        # absorb that BatchNorm's backward mask and partial sums (conv3x3_dgrad_bn_hip)
        ctx.fold = fold if (ctx.c3 and fork is None and fold is not None and _fold_3x3_ok(fold, x, wb)) else None
        cands = {"miopen": lambda: _miopen_fwd(x, wb, stride, padding)}
        if pre is not None:
            # x is a deferred BatchNorm + ReLU's input (ops/bn.py DeferredApply): the
            # forward stages the activation itself (conv_nhwc chose this path: 3x3 /
            # stride 1 / pad 1, no fork)
            y, bn_stats.part = conv3x3_stats_hip(x, wb, pre)
        elif not ctx.c3 and conv3x3s2_ok(x, wb, stride, padding):
            # 3x3 / stride 2 / pad 1 (ResNet's downsample conv2): the stride-2 MFMA forward
            # against the library; backward adds the in-tree input gradient to the strided
            # layer's candidates
            ctx.s2 = True
            key = (x.size(0) * x.size(2) * x.size(3), x.size(1), wb.size(0), 3, 3, 2, 1)
            if (bn_stats is not None and conv3x3_stats_enabled()
                    and not torch.are_deterministic_algorithms_enabled()):
                cands["hip_st"] = lambda: conv3x3s2_stats_hip(x, wb)
                y = _run_stats("fwd_kxk_st", key, cands, "hip_st", bn_stats)
            else:
                # deterministic mode too: _pick's fixed order lands on "hip" (bitwise
                # reproducible) and the BatchNorm makes its own pass
                cands["hip"] = lambda: conv3x3s2_hip(x, wb)
                y = _run("fwd_kxk", key, cands)
        elif not ctx.c3:
            y = cands["miopen"]()  # the only backend of any other strided or non-3x3 forward
        else:
            key = (x.size(0) * x.size(2) * x.size(3), x.size(1), wb.size(0), 3, 3, 1, 1)
            if bn_stats is not None and conv3x3_stats_enabled():
                # the next BatchNorm's statistics: in this kernel's epilogue, or the
                # library forward + BN's own partial pass -- whichever is faster
                cands["hip_st"] = lambda: conv3x3_stats_hip(x, wb)
                y = _run_stats("fwd_kxk_st", key, cands, "hip_st", bn_stats)
            else:
                cands["hip"] = lambda: conv3x3_hip(x, wb)
                y = _run("fwd_kxk", key, cands)
        ctx.save_for_backward(x, wb)
        ctx.geo = (tuple(stride), tuple(padding))
        ctx.fork = fork
        if fork is not None:
            fork.users += 1
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        stride, padding = ctx.geo
        dy = dy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        cout, cin, kh, kw = wb.shape
        st = ctx.pre_st  # x is a deferred BatchNorm + ReLU's input (3x3 / stride 1 / pad 1, no fork)
        dgrad = {"miopen": lambda: _miopen_bwd(dy, x, wb, stride, padding, True, False)[0]}
        if ctx.c3:
            dgrad["hip"] = lambda: conv3x3_dgrad_hip(dy, wb)
        # deferred-BatchNorm input: the weight gradient stages relu(x * scale + shift) (halo
        # or generic MFMA kernel, csrc/conv_wgrad.hip PRE), which MIOpen cannot; the input
        # gradient does not read x
        wgrad = {"miopen": lambda: _miopen_bwd(dy, x, wb, stride, padding, False, True)[1]} if st is None else {}
        wgrad["hip"] = lambda: wgrad_hip(dy, x, (kh, kw), stride, padding, pre_ss=st)
        if (kh, kw, stride, padding) == (3, 3, (1, 1), (1, 1)):
            # "hip" is the halo kernel here; the generic tap-GEMM kernel competes too
            wgrad["hip_gen"] = lambda: wgrad_hip(dy, x, (kh, kw), stride, padding, algo=1, pre_ss=st)
        dx = dw = None
        fork = ctx.fork if ctx.needs_input_grad[0] else None
        if fork is not None and fork.users >= 2 and fork.dx is not None and (kh, kw) == (1, 1) \
                and padding == (0, 0):
            # second of a forked pair, strided 1x1: GEMM over the output pixels, added
            # into every stride-th input pixel of the parked dgrad (1/s^2 of it)
            n_, _, oh_, ow_ = dy.shape
            g2 = _gemm_dgrad(_nhwc2d(dy), wb.reshape(cout, cin))

            def acc(d):
                # (measured and reverted, round 5: the same sum as ONE strided batched
                # GEMM with beta = 1 into every stride-th pixel -- hipBLASLt ran it as
                # MT256x16x64 at ~205 us a call vs ~21 us for this GEMM + strided add)
                s_ = stride[0]
                if (s_ == stride[1] and d.dtype == torch.bfloat16 and g2.dtype == torch.bfloat16
                        and d.is_contiguous(memory_format=torch.channels_last) and g2.is_contiguous()
                        and d.size(1) % 8 == 0 and (d.size(2) - 1) // s_ + 1 == oh_
                        and (d.size(3) - 1) // s_ + 1 == ow_):
                    # 16-byte vectors over the NHWC rows, same fp32 add + one rounding
                    # as ATen's add_ (which took its non-vectorised strided path)
                    from . import require

                    require().strided_add_(d, g2, s_)
                    return
                view = d[:, :, ::stride[0], ::stride[1]]
                view.add_(_from2d(g2, n_, oh_, ow_))

            dx = _fork_dx(fork, None, acc)
            fork = None  # the input gradient is settled
        need_dx = bool(ctx.needs_input_grad[0]) and dx is None
        be_d = be_w = None
        fold = ctx.fold
        if (need_dx and fold is not None and ctx.fork is None and fold.xin is not None and not fold.claimed
                and _pick_dgrad_bn((x.size(0) * x.size(2) * x.size(3), cin, cout, 3, 3, 1, 1), dy, wb, fold)
                == "fused"):
            # d = dgrad masked by the producer BatchNorm's recomputed ReLU mask, and that
            # BatchNorm's backward partial sums, in one kernel; its backward takes d as its dy
            dx, part = conv3x3_dgrad_bn_hip(dy, wb, fold.xin, fold.st)
            fold.bwd_part, fold.bwd_d = part, dx  # bn backward checks it receives exactly this tensor
            stats["bn_dgrad_fused_3x3"] += 1
            need_dx = False
        if ctx.needs_input_grad[1]:
            key = (x.size(0) * dy.size(2) * dy.size(3), cin, cout, kh, kw, stride[0], padding[0])
            be_w = _pick("wgrad_kxk" if st is None else "wgrad_kxk_pre", key, wgrad)
        if need_dx and ctx.c3:
            key = (x.size(0) * x.size(2) * x.size(3), cin, cout, 3, 3, 1, 1)
            be_d = _pick("dgrad_kxk", key, dgrad)
        elif need_dx and ctx.s2 and conv3x3s2_dgrad_ok(dy, wb, x.size(2), x.size(3)):
            # 3x3 / stride 2 / pad 1 whose forward predicate held: the quad-tiled MFMA kernel
            # against the library (in deterministic mode the kernel, untimed)
            dgrad["hip"] = lambda: conv3x3s2_dgrad_hip(dy, wb, x.size(2), x.size(3))
            be_d = _pick_dgrad_s2((x.size(0) * x.size(2) * x.size(3), cin, cout, 3, 3, 2, 1), dgrad)
        elif need_dx:  # MIOpen is the only backend of any other strided or non-3x3 input gradient
            be_d = "miopen"
        if be_d == "miopen" and be_w == "miopen":
            # MIOpen for both gradients: one call, as F.conv2d's autograd makes it
            dxm, dw = _miopen_bwd(dy, x, wb, stride, padding, True, True)
            dx = _fork_dx(fork, lambda: dxm, None)
        else:
            if be_d is not None:
                dx = _fork_dx(fork, dgrad[be_d], None)
            if be_w is not None:
                dw = wgrad[be_w]()
        return dx, dw, None, None, None, None, None, None, None


@functools.lru_cache(maxsize=64)
def _stem_shape_ok(n: int, h: int, w: int) -> bool:
    from . import require

    return bool(require().stem_supported(n, h, w))


def stem_fast_ok(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    """The ResNet stem (7x7 / stride 2 / pad 3, 3 -> 64, no bias) on an NHWC bf16 input
    the MFMA stem kernel covers (csrc/stem.hip); ``RLA_STEM=off`` keeps MIOpen."""
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 and x.size(1) == 3
            and conv.in_channels == 3 and conv.out_channels == 64 and conv.kernel_size == (7, 7)
            and conv.stride == (2, 2) and conv.padding == (3, 3) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.padding_mode == "zeros"
            and os.environ.get("RLA_STEM", "auto") != "off" and _stem_shape_ok(x.size(0), x.size(2), x.size(3)))


def stem_hip(x: torch.Tensor, wb: torch.Tensor, stats: bool = False):
    """``conv2d(x, wb, stride=2, padding=3)`` for the stem on the MFMA kernel: ``x`` [N, 3,
    H, W] bf16 (any layout; made NHWC-contiguous), ``wb`` [64, 3, 7, 7] bf16 channels_last.
    Returns y [N, 64, OH, OW] channels_last, or (y, part [rows, 2, 64]) with ``stats``."""
    from . import require

    xn = x.permute(0, 2, 3, 1).contiguous()
    out = require().stem_fwd(xn, wb.permute(0, 2, 3, 1).contiguous(), stats)
    y = out[0].permute(0, 3, 1, 2)
    return (y, out[1]) if stats else y


def stem_wgrad_hip(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Weight gradient of the stem on the MFMA kernel (csrc/stem.hip): fp32 [64, 3, 7, 7]
    with channels_last strides (the master weight's layout)."""
    from . import require

    dw = require().stem_wgrad(x.permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous())
    return dw.permute(0, 3, 1, 2)


class _StemFn(torch.autograd.Function):
    """Stem forward (with the next BatchNorm's statistics when asked) and weight gradient
    on the MFMA kernels; the input gradient, if one is wanted, from MIOpen."""

    @staticmethod
    def forward(ctx, x, weight, wb, bn_stats=None):
        if bn_stats is not None:
            y, bn_stats.part = stem_hip(x, wb, stats=True)
        else:
            y = stem_hip(x, wb)
        ctx.save_for_backward(x, wb)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _miopen_bwd(dy, x, wb, (2, 2), (3, 3), True, False)[0]
        if ctx.needs_input_grad[1]:
            dw = stem_wgrad_hip(x, dy)
        return dx, dw, None, None


def stem_conv(x: torch.Tensor, conv: nn.Conv2d, wb: torch.Tensor, bn_stats: Optional[BNStats] = None) -> torch.Tensor:
    """``conv(x)`` for the ResNet stem (:func:`stem_fast_ok`) with the bf16 shadow ``wb``."""
    stats["stem"] += 1
    return _StemFn.apply(x, conv.weight, wb, bn_stats)


def kxk_fast_ok(x: torch.Tensor, conv: nn.Conv2d) -> bool:
    return (x.is_cuda and x.dim() == 4 and x.dtype == torch.bfloat16 and x.numel() > 0
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.padding_mode == "zeros" and isinstance(conv.padding, tuple)
            and wgrad_ok(conv.in_channels, conv.out_channels))


def conv_nhwc(x: torch.Tensor, conv: nn.Conv2d, wb: torch.Tensor, fork: Optional[GradFork] = None,
              bn_stats: Optional[BNStats] = None) -> torch.Tensor:
    """``conv(x)`` with the bf16 weight ``wb`` (the arena shadow), the weight gradient
    going to ``conv.weight`` in fp32 (``fork``: see :class:`GradFork`; ``bn_stats``:
    see :class:`BNStats`, filled only by the 3x3 MFMA forwards, stride 1 or 2)."""
    # before materialize(x), whose result no longer carries the tag
    fold = getattr(x, "_rla_fold", None) if getattr(conv, "fuse_bn_dgrad", False) else None
    pre = getattr(x, "_rla_pre", None)
    if pre is not None:
        # a deferred BatchNorm + ReLU output (ops/bn.py DeferredApply): the 3x3 statistics
        # forward stages the activation itself where that is faster than the apply pass +
        # the regular kernel (timed per shape; the PRE kernel is the run-time-shape
        # instance), else the activation is materialised here
        from .bn import materialize

        if (fork is None and bn_stats is not None and not pre.used and conv3x3_stats_enabled()
                and x.size(1) <= 512 and conv3x3_ok(x, wb, conv.stride, conv.padding)):
            key = (x.size(0) * x.size(2) * x.size(3), x.size(1), wb.size(0), 3, 3, 1, 1)
            tp = _TimingPre(pre)
            be = os.environ.get("RLA_CONV3X3_PRE", "auto")  # pre | apply | auto (timed)
            if be not in ("pre", "apply"):
                be = _pick("fwd_kxk_pre", key, {
                    "pre": lambda: conv3x3_stats_hip(x, wb, tp),
                    "apply": lambda: conv3x3_stats_hip(_applied(x, tp), wb),
                })
            if be == "pre":
                pre.used = True
                stats["fast"] += 1
                stats["pre_applied"] += 1
                return _ConvNHWCFn.apply(x, conv.weight, wb, conv.stride, conv.padding, None, bn_stats, pre, fold)
        x = materialize(x)
    stats["fast"] += 1
    return _ConvNHWCFn.apply(x, conv.weight, wb, conv.stride, conv.padding, fork, bn_stats, None, fold)
