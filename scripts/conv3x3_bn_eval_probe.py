"""The four stride-1 3x3 conv + eval-mode BatchNorm shapes of ResNet-50 and its stem at batch 128
(bf16, NHWC, ``no_grad``, bf16 autocast) on the two arms of the eval dispatch: ``fused``
(csrc/conv3x3.hip ACT: BatchNorm and ReLU in the convolution's rounding loop; the stem kernel
with bn1 + ReLU folded into the max pool) and ``split`` (the modules' own forwards: the library
convolution, the coefficient ops, ``bn_apply``, and for the stem the pool behind them).  The
arms are timed the way the dispatch times them (``_time``: device events behind a spin kernel),
interleaved over ROUNDS rounds; one JSON line per (shape, arm) with the best and the median
round, then the dispatch's own picks (``choices()``)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_lightning_accelerators_amd import ops  # noqa: E402
from ray_lightning_accelerators_amd.ops import conv as C  # noqa: E402
from ray_lightning_accelerators_amd.ops.bn import BatchNormAct2d  # noqa: E402
from ray_lightning_accelerators_amd.ops.pool import MaxPool2dNHWC  # noqa: E402
from ray_lightning_accelerators_amd.ops.shadow import ConvBF16  # noqa: E402

B = int(os.environ.get("BATCH", "128"))
SHAPES = [(56, 64), (28, 128), (14, 256), (7, 512)]  # (H = W, Cin = Cout): bottleneck conv2 -> bn2 relu
REPS, ROUNDS = 20, 7


def _bn(dev, c):
    bn = BatchNormAct2d(c).to(dev).eval()
    bn.running_mean.normal_(0, 0.5)
    bn.running_var.uniform_(0.25, 4.0)
    return bn


def _race(tag, arms, **extra):
    """Both arms over ROUNDS interleaved rounds -> JSON lines; the relative difference of their outputs."""
    ref = arms["split"]().float()
    err = float((arms["fused"]().float() - ref).norm() / ref.norm())
    t = {name: [] for name in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            t[name].append(C._time(fn, REPS) * 1e3 / REPS)
    best = min(t, key=lambda k: statistics.median(t[k]))
    for name, v in t.items():
        print(json.dumps(dict(tag, batch=B, arm=name, us_best=round(min(v), 1),
                              us_median=round(statistics.median(v), 1), won=name == best,
                              rel_diff_vs_split=round(err, 6), **extra)), flush=True)


def probe(dev):
    m_ = ops.require()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for hw, c in SHAPES:
            x = torch.randn(B, c, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            conv = ConvBF16(c, c, 3, 1, 1, bias=False).to(dev).to(memory_format=torch.channels_last).eval()
            bn = _bn(dev, c)
            assert C.conv3x3_bn_eval_ok(x, conv, bn), (hw, c)
            wb = conv.weight.detach().to(torch.bfloat16)
            arms = {"fused": lambda: C.conv3x3_bn_act_hip(x, wb, bn.running_mean, bn.running_var, bn.weight.detach(),
                                                          bn.bias.detach(), bn.eps, True),
                    "split": lambda: bn(conv(x))}
            _race({"layer": "conv3x3", "hw": hw, "cin": c, "cout": c}, arms,
                  plan=list(m_.conv3x3_plan(B, hw, hw, c, c)))
            C.conv3x3_bn_eval(x, conv, bn)  # the dispatch's own timed pick
        x = torch.randn(B, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
        conv = ConvBF16(3, 64, 7, 2, 3, bias=False).to(dev).to(memory_format=torch.channels_last).eval()
        bn, pool = _bn(dev, 64), MaxPool2dNHWC(3, 2, 1)
        assert C.stem_bn_eval(x, conv, bn, pool) is not None
        _race({"layer": "stem", "hw": 224, "cin": 3, "cout": 64},
              {"fused": lambda: C.stem_bn_eval(x, conv, bn, pool), "split": lambda: pool(bn(conv(x)))})
    print(json.dumps({"choices": {k: v for k, v in C.choices().items() if k.startswith("fwd_kxk_bn_eval")}}),
          flush=True)


if __name__ == "__main__":
    torch.backends.cudnn.benchmark = True  # MIOpen find, as the ResNet-50 bench runs it
    torch.manual_seed(0)
    probe(torch.device("cuda", 0))
