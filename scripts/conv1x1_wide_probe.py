"""Per-shape sweep of the wide-tile split-K 1x1 forward (csrc/conv1x1_wide.hip) over
ResNet-50's K >= 256 layers at batch 128 (bf16, NHWC): every (bn, splits) instance the
shape admits and the planner's own pick, beside the existing statistics kernel
(csrc/conv1x1.hip) and hipBLASLt / MIOpen + the separate BatchNorm partial pass -- the
arms of the ``fwd_st`` dispatch table, timed the way the dispatch times them.  One JSON
line per (shape, arm); the planner's rule for bn and splits is read off this table."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ray_lightning_accelerators_amd import ops  # noqa: E402
from ray_lightning_accelerators_amd.ops.conv import _bn_partial, _from2d, _time, conv1x1_stats_hip  # noqa: E402

B = int(os.environ.get("BATCH", "128"))
# (H = W, Cin, Cout): the stride-1 1x1 layers with Cin >= 256 and Cout % 128 == 0
SHAPES = [(56, 256, 128), (28, 512, 128), (28, 512, 256), (14, 1024, 256), (14, 256, 1024), (14, 1024, 512),
          (7, 512, 2048), (7, 2048, 512)]
REPS = 20


def main():
    torch.backends.cudnn.benchmark = True  # MIOpen find, as the ResNet-50 bench runs it
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m_ = ops.require()
    conv = torch.ops.aten.convolution
    for hw, cin, cout in SHAPES:
        x = torch.randn(B, cin, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wb = (torch.randn(cout, cin, device=dev) / cin ** 0.5).to(torch.bfloat16)
        x2 = x.permute(0, 2, 3, 1).reshape(-1, cin)
        w4 = wb.view(cout, cin, 1, 1)
        m = x2.size(0)
        ref = torch.mm(x2, wb.t()).float()
        plan = list(m_.conv1x1_wide_plan(m, cin, cout))
        arms = {
            "hip": lambda: conv1x1_stats_hip(x, wb),
            "gemm+partial": lambda: _bn_partial(_from2d(torch.mm(x2, wb.t()), B, hw, hw)),
            "miopen+partial": lambda: _bn_partial(conv(x, w4, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1)),
            "wide_plan": lambda: m_.conv1x1_wide(x2, wb),
        }
        for bn in (256, 128):
            for splits in (1, 2, 4):
                if cout % bn == 0:
                    arms[f"wide_{bn}x{splits}"] = lambda bn=bn, splits=splits: m_.conv1x1_wide(x2, wb, bn, splits)
        for name, fn in arms.items():
            try:
                out = fn()
            except RuntimeError:  # an instance the shape does not admit on this device
                continue
            err = None
            if name.startswith("wide"):
                err = round(float((out[0].float() - ref).norm() / ref.norm()), 6)
            t = min(_time(fn, REPS), _time(fn, REPS)) * 1e3 / REPS
            print(json.dumps({"hw": hw, "cin": cin, "cout": cout, "batch": B, "arm": name, "us": round(t, 1),
                              "plan": plan, "rel_err_vs_gemm": err}), flush=True)


if __name__ == "__main__":
    main()
