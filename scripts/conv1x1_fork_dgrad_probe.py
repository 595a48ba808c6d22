"""Device time of the fused input gradient of ResNet-50's four forked 1x1 pairs (conv1 +
downsample, csrc/conv1x1_fork_dgrad.hip) against the parked-dgrad route in both arrival orders,
at batch 128: 7 interleaved rounds of 20 back-to-back calls each (ops.conv._time: the device is
held busy while the host enqueues), median and best round in device microseconds per call.

  python scripts/conv1x1_fork_dgrad_probe.py [--batch 128] [--out profiles/r29_fork_dgrad]
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_lightning_accelerators_amd.ops import conv as C

# (H = W, Cin, C1, Cd, s): layer1.0 .. layer4.0
SHAPES = [(56, 64, 64, 256, 1), (56, 256, 128, 512, 2), (28, 512, 256, 1024, 2), (14, 1024, 512, 2048, 2)]
ROUNDS, CALLS = 7, 20


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default="profiles/r29_fork_dgrad")
    args = ap.parse_args()
    n, rows = args.batch, []
    for hw, cin, c1, cd, s in SHAPES:
        oh = (hw - 1) // s + 1
        rnd = lambda *d: torch.randn(*d, device="cuda", dtype=torch.bfloat16)
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        x, dy1, dyd = cl(rnd(n, cin, hw, hw)), cl(rnd(n, c1, hw, hw)), cl(rnd(n, cd, oh, oh))
        w1, wd = rnd(c1, cin) / cin ** 0.5, rnd(cd, cin) / cin ** 0.5
        cands = {
            "fused": lambda: C.conv1x1_fork_dgrad_hip(dy1, w1, dyd, wd, s),
            "split_conv1_first": lambda: C._fork_split(dy1, w1, dyd, wd, x, s, True),
            "split_downsample_first": lambda: C._fork_split(dy1, w1, dyd, wd, x, s, False),
        }
        ref = cands["split_conv1_first"]().float()
        err = (cands["fused"]().float() - ref).abs().max().item() / ref.abs().max().item()
        t = {name: [] for name in cands}
        for _ in range(ROUNDS):
            for name, fn in cands.items():
                t[name].append(C._time(fn, CALLS) * 1e3 / CALLS)
        row = {"shape": [n, hw, hw, cin, c1, cd, s], "max_rel_diff_vs_split": err}
        for name, v in t.items():
            row[name] = {"median_us": round(statistics.median(v), 1), "best_us": round(min(v), 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "probe.json").write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                                                "calls": CALLS, "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
