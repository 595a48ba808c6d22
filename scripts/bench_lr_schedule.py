"""Cost of a step-interval LR scheduler on the fused MNIST step (one GPU, 784-32-64-10, batch 32).

``Trainer.fit`` of ``LightningMNISTClassifier`` on the synthetic split, epochs after the first
(the first captures the graphs), timed between two synchronisations.  Prints one JSON line
with us/step of
  scheduled    Adam + ``OneCycleLR(cycle_momentum=False)`` at step interval
  unscheduled  the same fit without a scheduler (``--only unscheduled`` / in ``all``)
On a tree with the rate ring the scheduled fit keeps chunked dispatch (hipGraph replays that
read each step's rate from the ring); on a tree without it the Trainer dispatches per batch.
The two trees are compared by running this script with the other tree first on PYTHONPATH.
(``cycle_momentum`` is off: a scheduler that also rewrites beta1 per step goes out per batch
on either tree, a captured graph bakes the betas.)
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


def fit_us_per_step(args, scheduled: bool) -> dict:
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.lightning.callbacks import Callback
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier

    marks = []

    class Clock(Callback):
        def on_train_epoch_start(self, trainer, pl_module):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        def on_train_end(self, trainer, pl_module):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

    total = args.steps * args.epochs

    class Model(LightningMNISTClassifier):
        def configure_optimizers(self):
            opt = torch.optim.Adam(self.parameters(), lr=args.lr)
            if not scheduled:
                return opt
            sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5 * args.lr, total_steps=total,
                                                      cycle_momentum=False)
            return [opt], [{"scheduler": sch, "interval": "step"}]

    pl.seed_everything(0)
    model = Model({"layer_1": 32, "layer_2": 64, "lr": args.lr, "batch_size": 32})
    trainer = pl.Trainer(gpus=1, max_epochs=args.epochs, limit_train_batches=args.steps, limit_val_batches=1,
                         callbacks=[Clock()], default_root_dir=args.root, checkpoint_callback=False, logger=False)
    trainer.fit(model)
    us = (marks[-1] - marks[1]) / (args.steps * (args.epochs - 1)) * 1e6  # epoch 0 warms up (capture, allocator)
    f = getattr(trainer, "_fused", None)
    eng = getattr(f, "eng", None)
    return {"us_per_step": round(us, 3), "fused": type(f).__name__ if f is not None else None,
            "graph_steps": getattr(eng, "_graph_steps", 0) if getattr(eng, "_graph", None) is not None else 0,
            "lr_ring": int(getattr(eng, "lr_ring", 0) or 0),
            "last_lr": trainer.optimizers[0].param_groups[0]["lr"]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["all", "scheduled", "unscheduled"], default="all")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--steps", type=int, default=1000, help="batches per epoch")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--root", default="/tmp/bench_lr_schedule")
    args = ap.parse_args()
    res = {"steps_per_epoch": args.steps, "epochs": args.epochs}
    if args.only in ("all", "scheduled"):
        res["scheduled"] = fit_us_per_step(args, True)
    if args.only in ("all", "unscheduled"):
        res["unscheduled"] = fit_us_per_step(args, False)
    if "scheduled" in res and "unscheduled" in res:
        res["scheduled_over_unscheduled"] = round(res["scheduled"]["us_per_step"] / res["unscheduled"]["us_per_step"], 3)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
