"""Epoch time of MNISTClassifier under the Trainer with the loaders the upstream module
builds: ``DataLoader(..., batch_size=32)`` with PyTorch's default ``drop_last=False`` over the
55,000 / 5,000 synthetic split (1,718 x 32 + 24 training and 156 x 32 + 8 validation samples).

Prints one JSON line: ms per epoch (training + validation, epochs after the first, which
captures graphs and warms the allocator), optimizer steps per epoch, how many validation
passes the fused ``eval_epoch`` served, and the rows of the last training step.  Timed with
a host clock between device synchronisations at the epoch starts.  ``--drop-last`` times the
in-tree loaders' setting for comparison.  A tree given on PYTHONPATH wins, which is how a
tree without the short-batch path (it drops the training batch and validates per batch) is
compared: run it with that tree first on PYTHONPATH.
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
from torch.utils.data import DataLoader  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--drop-last", action="store_true")
    ap.add_argument("--root", default="/tmp/bench_short_batch")
    args = ap.parse_args()

    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.lightning.callbacks import Callback
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep, MNISTClassifier

    class Upstream(MNISTClassifier):
        def train_dataloader(self):
            self.prepare_data()
            return DataLoader(self._train_set, batch_size=self.batch_size, drop_last=args.drop_last)

        def val_dataloader(self):
            self.prepare_data()
            return DataLoader(self._val_set, batch_size=self.batch_size, drop_last=args.drop_last)

    marks = []

    class Clock(Callback):
        def on_train_epoch_start(self, trainer, pl_module):
            torch.cuda.synchronize()
            marks.append((time.perf_counter(), trainer.global_step))

        def on_train_end(self, trainer, pl_module):
            torch.cuda.synchronize()
            marks.append((time.perf_counter(), trainer.global_step))

    fused_val = []
    orig = FusedMNISTStep.eval_epoch

    def counting(self, dl, n):
        res = orig(self, dl, n)
        fused_val.append(res is not None)
        return res

    FusedMNISTStep.eval_epoch = counting
    pl.seed_everything(0)
    model = Upstream({"layer_1": 32, "layer_2": 64, "lr": args.lr, "batch_size": 32})
    trainer = pl.Trainer(gpus=1, max_epochs=args.epochs, callbacks=[Clock()], default_root_dir=args.root,
                         checkpoint_callback=False, logger=False, num_sanity_val_steps=0)
    trainer.fit(model)
    ms = [(b[0] - a[0]) * 1e3 for a, b in zip(marks[1:-1], marks[2:])]  # epoch 0 warms up
    steps = [b[1] - a[1] for a, b in zip(marks[1:-1], marks[2:])]
    f = trainer._fused
    eng = getattr(f, "eng", None)
    print(json.dumps({
        "drop_last": args.drop_last, "epochs_timed": len(ms), "ms_per_epoch_min": round(min(ms), 3),
        "ms_per_epoch_median": round(sorted(ms)[len(ms) // 2], 3), "ms_per_epoch_max": round(max(ms), 3),
        "steps_per_epoch": steps[0], "fused_step": type(f).__name__ if f is not None else None,
        "validation_passes": len(fused_val), "validation_passes_fused": sum(fused_val),
        "last_train_rows": float(eng.recent_stats(1)[0, 2]) if eng is not None else None,
        "val_loss": float(trainer.callback_metrics["ptl/val_loss"]),
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
