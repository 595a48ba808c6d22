"""Every distinct stride-1 1x1 conv + eval-mode BatchNorm of ResNet-50 at batch 128 (bf16, NHWC)
on the two arms of the ``fwd_bn_eval`` dispatch: ``fused`` (csrc/conv1x1_bn_act.hip: BatchNorm,
ReLU and the shortcut add in the GEMM's epilogue) and ``split`` (the 1x1 forward's own timed
pick, the coefficient ops and ``bn_apply``), each layer with the epilogue it has in the model.
The arms are timed the way the dispatch times them (``_time``: device events behind a spin
kernel), interleaved over ROUNDS rounds; one JSON line per (shape, arm) with the best and the
median round, then the dispatch's own picks (``choices()``).  ``--forward``: instead, the whole
ResNet-50 eval forward (``no_grad``, bf16 autocast) under the switch given in the environment."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_lightning_accelerators_amd import ops  # noqa: E402
from ray_lightning_accelerators_amd.ops import conv as C  # noqa: E402
from ray_lightning_accelerators_amd.ops.bn import BatchNormAct2d  # noqa: E402

B = int(os.environ.get("BATCH", "128"))
# (H = W, Cin, Cout, epilogue): conv1 -> bn1 relu, conv3 -> bn3 relu + residual, layer1.0.downsample affine
SHAPES = [(56, 64, 64, "relu"), (56, 64, 256, "relu_res"), (56, 64, 256, "affine"), (56, 256, 64, "relu"),
          (56, 256, 128, "relu"), (28, 128, 512, "relu_res"), (28, 512, 128, "relu"), (28, 512, 256, "relu"),
          (14, 256, 1024, "relu_res"), (14, 1024, 256, "relu"), (14, 1024, 512, "relu"), (7, 512, 2048, "relu_res"),
          (7, 2048, 512, "relu")]
REPS, ROUNDS = 20, 7


def _layer(dev, hw, cin, cout, epi):
    x = torch.randn(B, cin, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    conv = C.Conv1x1NHWC(cin, cout).to(dev).eval()
    bn = BatchNormAct2d(cout, act=None if epi == "affine" else "relu").to(dev).eval()
    bn.running_mean.normal_(0, 0.5)
    bn.running_var.uniform_(0.25, 4.0)
    res = None
    if epi == "relu_res":
        res = torch.randn(B, cout, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    return x, conv, bn, res


def probe(dev):
    m_ = ops.require()
    for hw, cin, cout, epi in SHAPES:
        x, conv, bn, res = _layer(dev, hw, cin, cout, epi)
        wb = conv.weight.detach().to(torch.bfloat16).reshape(cout, cin)
        arms = {
            "fused": lambda: C.conv1x1_bn_act_hip(x, wb, bn.running_mean, bn.running_var, bn.weight.detach(),
                                                  bn.bias.detach(), bn.eps, bn.act == "relu", res),
            "split": lambda: bn(conv(x), residual=res),
        }
        with torch.no_grad():
            ref = arms["split"]().float()
            err = float((arms["fused"]().float() - ref).norm() / ref.norm())
            t = {name: [] for name in arms}
            for _ in range(ROUNDS):
                for name, fn in arms.items():
                    t[name].append(C._time(fn, REPS) * 1e3 / REPS)
            C.conv1x1_bn_eval(x, conv, bn, res)  # the dispatch's own timed pick
        best = min(t, key=lambda k: statistics.median(t[k]))
        for name, v in t.items():
            print(json.dumps({"hw": hw, "cin": cin, "cout": cout, "epi": epi, "batch": B, "arm": name,
                              "us_best": round(min(v), 1), "us_median": round(statistics.median(v), 1),
                              "won": name == best, "rel_diff_vs_split": round(err, 6),
                              "plan": dict(m_.conv1x1_bn_act_plan(B * hw * hw, cin, cout))}), flush=True)
    print(json.dumps({"choices": {k: v for k, v in C.choices().items() if k.startswith("fwd_bn_eval")}}), flush=True)


def forward(dev, steps=20, rounds=3):
    from ray_lightning_accelerators_amd.models.resnet import resnet50

    model = resnet50(fused_bn=True).to(dev).to(memory_format=torch.channels_last).eval()
    x = torch.randn(B, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    ms = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(3):  # warm: every timed pick
            y = model(x)
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                y = model(x)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
    print(json.dumps({"eval_forward_ms": [round(v, 3) for v in ms], "batch": B,
                      "switch": os.environ.get("RLA_CONV1X1_BN_EVAL", "auto"),
                      "bn_eval_fused": C.stats.get("bn_eval_fused"), "checksum": float(y.float().abs().mean())}),
          flush=True)


if __name__ == "__main__":
    torch.backends.cudnn.benchmark = True  # MIOpen find, as the ResNet-50 bench runs it
    torch.manual_seed(0)
    (forward if "--forward" in sys.argv else probe)(torch.device("cuda", 0))
