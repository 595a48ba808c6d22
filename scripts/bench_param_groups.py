"""Cost of param groups that interleave in the arena (one GPU, ResNet-50's real arena).

``--only kernel`` (default) prints one JSON line with us / launch, per run, of
  sgd_groups     ONE table-driven launch over the two-group table of "weight decay on the
                 dim > 1 parameters, none on BatchNorm parameters and biases" (108 runs)
  sgd_single     the single-group sgd_kernel over the same buffers: it moves the same bytes
``--runs`` runs of each, interleaved, every run ``--iters`` launches after ``--warmup`` between two
device events; momentum 0.9 and the bf16 shadow on, as the Trainer's ResNet-50 step runs them.

``--only trainer`` times ``Trainer.fit`` of LightningResNet50 with those two param groups (set in
a subclass here, so a tree without the ``no_decay_norm_bias`` option runs the same optimizer: give
that tree on PYTHONPATH) and prints whether the step was graph-captured and ms / step of the epochs
after the first.
"""
import argparse
import json
import os
import sys
import time

try:
    import ray_lightning_accelerators_amd  # noqa: F401  (a tree given on PYTHONPATH wins)
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def timed_us(run, iters: int) -> float:
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def resnet50_layout():
    """(arena offsets, group of each member) of resnet50(1000) in parameters() order."""
    from ray_lightning_accelerators_amd.models.resnet import resnet50

    with torch.device("meta"):
        params = list(resnet50(1000).parameters())
    offsets, off = [], 0
    for p in params:
        offsets.append((off, p.numel()))
        off += (p.numel() + 3) // 4 * 4
    return offsets, [0 if p.dim() > 1 else 1 for p in params], off


def bench_kernel(args) -> dict:
    from ray_lightning_accelerators_amd.ops.optim import build_group_table, fused_sgd_, fused_sgd_groups_

    dev = torch.device("cuda", 0)
    offsets, group_of, numel = resnet50_layout()
    table = build_group_table(offsets, group_of, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = 0.05 * torch.randn(numel, device=dev, generator=gen)
    g = 0.01 * torch.randn(numel, device=dev, generator=gen)
    buf = torch.zeros(numel, device=dev)
    bf = torch.empty(numel, dtype=torch.bfloat16, device=dev)
    hyper = [dict(lr=args.lr, momentum=0.9, weight_decay=5e-5), dict(lr=args.lr, momentum=0.9, weight_decay=0.0)]

    def groups():
        fused_sgd_groups_(p, g, buf, table, hyper, steps=[2, 2], p_bf16=bf)

    def single():
        fused_sgd_(p, g, buf, lr=args.lr, momentum=0.9, weight_decay=5e-5, step=2, p_bf16=bf)

    res = {"numel": numel, "rows": int(table.size(0)), "iters": args.iters, "sgd_groups_us": [], "sgd_single_us": []}
    for run in (groups, single):
        for _ in range(args.warmup):
            run()
    for _ in range(args.runs):
        res["sgd_groups_us"].append(round(timed_us(groups, args.iters), 2))
        res["sgd_single_us"].append(round(timed_us(single, args.iters), 2))
    # p, g, buf read, p, buf written (fp32), the shadow written (bf16)
    res["bytes_per_launch"] = numel * (5 * 4 + 2)
    return res


def bench_trainer(args) -> dict:
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.lightning.callbacks import Callback
    from ray_lightning_accelerators_amd.models.resnet import LightningResNet50

    marks = []

    class Clock(Callback):
        def on_train_epoch_start(self, trainer, pl_module):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        def on_train_end(self, trainer, pl_module):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

    class NoDecayNormBias(LightningResNet50):
        def configure_optimizers(self):
            params = list(self.parameters())
            groups = [{"params": [q for q in params if q.dim() > 1], "weight_decay": self.cfg["weight_decay"]},
                      {"params": [q for q in params if q.dim() <= 1], "weight_decay": 0.0}]
            return torch.optim.SGD(groups, lr=self.cfg["lr"], momentum=self.cfg["momentum"])

    pl.seed_everything(0)
    model = NoDecayNormBias({"batch_size": args.batch, "n_train": args.batch * args.trainer_steps})
    trainer = pl.Trainer(gpus=1, max_epochs=args.trainer_epochs, callbacks=[Clock()], default_root_dir=args.root,
                         checkpoint_callback=False, logger=False, progress_bar_refresh_rate=0)
    trainer.fit(model)
    steps = args.trainer_steps * (args.trainer_epochs - 1)
    fused = getattr(trainer, "_fused", None)
    opt = trainer.optimizers[0]
    return {"ms_per_step": round((marks[-1] - marks[1]) / steps * 1e3, 3),   # epoch 0 warms up (capture, allocator)
            "trainer_step": type(fused).__name__ if fused is not None else None,
            "graph_replays": getattr(fused, "replays", None), "graph_failed": getattr(fused, "failed", None),
            "graph_step_reason": getattr(trainer, "_graph_step_reason", None) or getattr(fused, "reason", None),
            "optimizer_fused": bool(getattr(opt, "_rla_fused", False)), "param_groups": len(opt.param_groups),
            "batch": args.batch, "steps_timed": steps}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernel", "trainer"], default="kernel")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--trainer-steps", type=int, default=24, help="batches per Trainer epoch")
    ap.add_argument("--trainer-epochs", type=int, default=3)
    ap.add_argument("--root", default="/tmp/bench_param_groups")
    args = ap.parse_args()
    res = bench_kernel(args) if args.only == "kernel" else bench_trainer(args)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
