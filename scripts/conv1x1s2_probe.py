"""ResNet-50's three stride-2 1x1 downsample forwards at batch 128 (bf16, NHWC) on the arms of
the ``fwd_1x1s2`` / ``fwd_1x1s2_st`` dispatch tables: MIOpen alone, MIOpen + the downsample
BatchNorm's partial pass (what ran before csrc/conv1x1s2.hip), the in-tree kernel and its
statistics instance.  The arms are timed the way the dispatch times them (``_time``: device
events behind a spin kernel), interleaved over ROUNDS rounds; one JSON line per (shape, arm)
with the best and the median round, then the dispatch's own picks (``choices()``)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_lightning_accelerators_amd import ops  # noqa: E402
from ray_lightning_accelerators_amd.ops import conv as C  # noqa: E402

B = int(os.environ.get("BATCH", "128"))
SHAPES = [(56, 256, 512), (28, 512, 1024), (14, 1024, 2048)]  # (H = W, Cin, Cout)
REPS, ROUNDS = 20, 7


def main():
    torch.backends.cudnn.benchmark = True  # MIOpen find, as the ResNet-50 bench runs it
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m_ = ops.require()
    for hw, cin, cout in SHAPES:
        x = torch.randn(B, cin, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wb = (torch.randn(cout, cin, 1, 1, device=dev) / cin ** 0.5).to(torch.bfloat16)
        wb = wb.contiguous(memory_format=torch.channels_last)
        arms = {
            "miopen": lambda: C._miopen_fwd(x, wb, (2, 2), (0, 0)),
            "miopen+partial": lambda: C._bn_partial(C._miopen_fwd(x, wb, (2, 2), (0, 0))),
            "hip": lambda: C.conv1x1s2_hip(x, wb),
            "hip_st": lambda: C.conv1x1s2_stats_hip(x, wb),
        }
        ref = arms["miopen"]().float()
        y, part = arms["hip_st"]()
        err = float((y.float() - ref).norm() / ref.norm())
        perr = float((part.sum(0)[0] - y.float().sum((0, 2, 3))).abs().max() / y.float().abs().sum((0, 2, 3)).max())
        t = {name: [] for name in arms}
        for _ in range(ROUNDS):
            for name, fn in arms.items():
                t[name].append(C._time(fn, REPS) * 1e3 / REPS)
        for name, v in t.items():
            print(json.dumps({"hw": hw, "cin": cin, "cout": cout, "batch": B, "arm": name, "us_best": round(min(v), 1),
                              "us_median": round(statistics.median(v), 1), "rel_err_vs_miopen": round(err, 6),
                              "part_rel_err": round(perr, 9),
                              "plan": list(m_.conv1x1s2_plan(B, hw, hw, cin, cout))}), flush=True)
        # the dispatch's own timed picks, plain and with a BatchNorm consumer
        conv = torch.nn.Conv2d(cin, cout, 1, 2, bias=False).to(dev)
        with torch.no_grad():
            C.conv_nhwc(x, conv, wb)
            C.conv_nhwc(x, conv, wb, bn_stats=C.BNStats())
    print(json.dumps({"choices": {k: v for k, v in C.choices().items() if k.startswith("fwd_1x1s2")}}), flush=True)


if __name__ == "__main__":
    main()
