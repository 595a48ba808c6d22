"""Cost of SGD on the fused MNIST step (one GPU, 784-L1-L2-10).

Prints one JSON line with us/step of
  engine_sgd_two_launch    FusedMLPEngine(optimizer="sgd", momentum=m): head, tail(sgd)
  engine_adam_two_launch   the Adam engine with RLA_MLP_ONE_LAUNCH=0: head, tail(adam)
  engine_sgd_split         the SGD engine on the split route (head, tail(grad), tail(sgd):
                           world size 2 faked after set_data, no allreduce)
  engine_adam_split        the Adam engine on the same route
  engine_adam_one_launch   the default one-launch step, for scale (batch <= 32)
  trainer_sgd              Trainer.fit of an MNISTClassifier whose configure_optimizers
                           returns torch.optim.SGD(lr, momentum=m), epochs after the first
each over ``--steps`` steps after ``--warmup``, graphs of ``--graph-steps`` steps, timed
with device events between two synchronisations (bench.py brackets its window the same
way).  ``--only trainer`` runs on a tree whose fused step knows only Adam (there the
Trainer falls back to autograd + the arena SGD), which is how the two Trainer routes are
compared: run it with the other tree first on PYTHONPATH.
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


def timed_us(run, steps: int) -> float:
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def bench_engine(args, optimizer: str, route: str) -> float:
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist
    from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

    x, y = synthetic_mnist(args.n_data, seed=0)
    kw = {"optimizer": "sgd", "momentum": args.momentum} if optimizer == "sgd" else {}
    old = os.environ.get("RLA_MLP_ONE_LAUNCH")
    if route != "one_launch":
        os.environ["RLA_MLP_ONE_LAUNCH"] = "0"  # read when the engine is built
    try:
        eng = FusedMLPEngine(args.l1, args.l2, args.batch, lr=args.lr, device=torch.device("cuda", 0), **kw)
    finally:
        if old is None:
            os.environ.pop("RLA_MLP_ONE_LAUNCH", None)
        else:
            os.environ["RLA_MLP_ONE_LAUNCH"] = old
    eng.set_data(x, y)
    assert eng.one_launch == (route == "one_launch")
    if route == "split":
        eng.world_size = 2  # same shard, three launches: head, tail(grad), tail(optimizer, grad_scale 1/2)
        fill = eng._fill_order

        def fill_world1(epoch):  # later epochs keep the world-1 shard the buffers were sized for
            eng.world_size = 1
            try:
                fill(epoch)
            finally:
                eng.world_size = 2

        eng._fill_order = fill_world1
    assert eng.capture(args.graph_steps)
    eng.run(args.warmup)
    us = timed_us(eng.run, args.steps)
    eng.check()
    h = eng.health()
    assert h["saturated"] == 0 and h["nonfinite"] == 0, h
    return us


def bench_trainer(args) -> dict:
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

    class SGDClassifier(LightningMNISTClassifier):
        def configure_optimizers(self):
            return torch.optim.SGD(self.parameters(), lr=self.lr, momentum=args.momentum)

    pl.seed_everything(0)
    model = SGDClassifier({"layer_1": args.l1, "layer_2": args.l2, "lr": args.lr, "batch_size": args.batch})
    per_epoch = args.trainer_steps
    trainer = pl.Trainer(gpus=1, max_epochs=args.trainer_epochs, limit_train_batches=per_epoch, limit_val_batches=1,
                         callbacks=[Clock()], default_root_dir=args.root, checkpoint_callback=False, logger=False)
    trainer.fit(model)
    steps = per_epoch * (args.trainer_epochs - 1)
    us = (marks[-1] - marks[1]) / steps * 1e6  # epoch 0 warms up (capture, allocator)
    fused = type(trainer._fused).__name__ if getattr(trainer, "_fused", None) is not None else None
    return {"trainer_sgd_us_per_step": round(us, 3), "trainer_step": fused,
            "trainer_health": getattr(trainer, "fused_step_health", None)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["all", "engine", "trainer"], default="all")
    ap.add_argument("--l1", type=int, default=32)
    ap.add_argument("--l2", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--graph-steps", type=int, default=8)
    ap.add_argument("--n-data", type=int, default=55000)
    ap.add_argument("--trainer-steps", type=int, default=1000, help="batches per Trainer epoch")
    ap.add_argument("--trainer-epochs", type=int, default=3)
    ap.add_argument("--root", default="/tmp/bench_sgd")
    args = ap.parse_args()
    res = {"l1": args.l1, "l2": args.l2, "batch": args.batch, "momentum": args.momentum, "steps": args.steps,
           "warmup": args.warmup, "graph_steps": args.graph_steps}
    if args.only in ("all", "engine"):
        for optimizer, route in (("sgd", "two_launch"), ("adam", "two_launch"), ("sgd", "split"), ("adam", "split")):
            res[f"engine_{optimizer}_{route}_us_per_step"] = round(bench_engine(args, optimizer, route), 3)
        if args.batch <= 32:
            res["engine_adam_one_launch_us_per_step"] = round(bench_engine(args, "adam", "one_launch"), 3)
        res["sgd_over_adam_two_launch"] = round(res["engine_sgd_two_launch_us_per_step"]
                                                / res["engine_adam_two_launch_us_per_step"], 3)
    if args.only in ("all", "trainer"):
        res.update(bench_trainer(args))
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
