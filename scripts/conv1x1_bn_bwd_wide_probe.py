"""Device time of the fused 1x1 input gradient + BatchNorm backward partial at K = 256 / 512
(csrc/conv1x1_bn_bwd_wide.hip) against the split route it replaces: a library input gradient
(GEMM or MIOpen) followed by bn_partial with the residual write.

The arms run interleaved in one session, ``--rounds`` rounds of ``--reps`` back-to-back calls
each; best and median per arm are printed as one JSON line per shape.

    python scripts/conv1x1_bn_bwd_wide_probe.py [--batch 128] [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import json
import statistics

import torch

from ray_lightning_accelerators_amd.ops import conv as C
from ray_lightning_accelerators_amd.ops import require

# ResNet-50 identity blocks: (name, Cin = N, Cout = K, H = W)
SHAPES = [("layer3.x.conv1", 1024, 256, 14), ("layer4.x.conv1", 2048, 512, 7)]


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(2_000_000)  # the host enqueues behind a busy device: calls run back to back
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mod, dev = require(), torch.device("cuda", 0)
    lines = []
    for name, cin, cout, hw in SHAPES:
        torch.manual_seed(0)
        nhwc = lambda c: torch.randn(args.batch, c, hw, hw, device=dev).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last)
        dy, x, dres, x3 = nhwc(cout), nhwc(cin), nhwc(cin), nhwc(cin)
        wb = (torch.randn(cout, cin, device=dev) * cin ** -0.5).to(torch.bfloat16)
        w4, dy2 = wb.view(cout, cin, 1, 1), C._nhwc2d(dy)
        dgrad = {
            "gemm": lambda: C._from2d(C._gemm_dgrad(dy2, wb), args.batch, hw, hw),
            "miopen": lambda: C._miopen_bwd(dy, x, w4, (1, 1), (0, 0), True, False)[0],
        }

        def split(be):
            da = dgrad[be]()
            dout = torch.empty_like(x3, memory_format=torch.channels_last)
            return mod.bn_partial(x3.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1), da.permute(0, 2, 3, 1), cin, 1, True,
                                  None, dres.permute(0, 2, 3, 1), None, dout.permute(0, 2, 3, 1))

        arms = {"fused": lambda: C.conv1x1_bn_bwd_wide_hip(dy, wb, dres, x, x3),
                "split_gemm": lambda: split("gemm"), "split_miopen": lambda: split("miopen")}
        for fn in arms.values():
            fn()  # warm: kernel load, solver search
        torch.cuda.synchronize()
        t = {a: [] for a in arms}
        for _ in range(args.rounds):
            for a, fn in arms.items():
                t[a].append(_time(fn, args.reps))
        m = args.batch * hw * hw
        row = {"layer": name, "M": m, "K": cout, "N": cin, "plan": dict(mod.conv1x1_bn_bwd_wide_plan(m, cout, cin),
                                                                        row_ranges=None)}
        for a, v in t.items():
            row[a] = {"best_us": round(min(v), 1), "median_us": round(statistics.median(v), 1)}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
