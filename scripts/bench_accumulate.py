"""Cost of gradient accumulation on the fused MNIST step (one GPU, 784-32-64-10, batch 32).

Prints one JSON line with us per micro-batch (and per optimizer step, K times that) of
  engine_acc_eager   FusedMLPEngine(accumulate=K), every launch issued from Python
  engine_acc_graph   the same engine replaying graphs of ``--graph-steps`` batches
  engine_split       the yardstick on the same tree: no accumulation, split route (head,
                     tail(grad), tail(adam): world size 2 faked after set_data, no allreduce)
  trainer_acc        Trainer.fit(accumulate_grad_batches=K) on MNISTClassifier, epochs after
                     the first
each over ``--steps`` batches after ``--warmup``, timed with device events between two
synchronisations (scripts/bench_clip.py brackets its window the same way).  ``--only
trainer`` runs on a tree whose engine has no ``accumulate`` (there the Trainer falls back
to autograd), which is how the two Trainer routes are compared: run it with the other
tree first on PYTHONPATH, parent and branch interleaved in one session.
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


def bench_engine(args, mode: str) -> float:
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist
    from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

    x, y = synthetic_mnist(args.n_data, seed=0)
    kw = {"accumulate": args.k} if mode.startswith("acc") else {}
    eng = FusedMLPEngine(32, 64, 32, lr=args.lr, device=torch.device("cuda", 0), **kw)
    eng.set_data(x, y)
    if mode == "split":
        eng.world_size = 2  # same shard, three launches: head, tail(grad), tail(adam, grad_scale 1/2)
        fill = eng._fill_order

        def fill_world1(epoch):  # later epochs keep the world-1 shard the buffers were sized for
            eng.world_size = 1
            try:
                fill(epoch)
            finally:
                eng.world_size = 2

        eng._fill_order = fill_world1
    if mode != "acc_eager":
        assert eng.capture(args.graph_steps)
    eng.run(args.warmup)
    us = timed_us(eng.run, args.steps)
    eng.check()
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

    pl.seed_everything(0)
    model = LightningMNISTClassifier({"layer_1": 32, "layer_2": 64, "lr": args.lr, "batch_size": 32})
    per_epoch = args.trainer_steps
    trainer = pl.Trainer(gpus=1, max_epochs=args.trainer_epochs, limit_train_batches=per_epoch, limit_val_batches=1,
                         accumulate_grad_batches=args.k, callbacks=[Clock()], default_root_dir=args.root,
                         checkpoint_callback=False, logger=False)
    trainer.fit(model)
    batches = per_epoch * (args.trainer_epochs - 1)
    us = (marks[-1] - marks[1]) / batches * 1e6  # epoch 0 warms up (allocator, code objects)
    fused = type(trainer._fused).__name__ if getattr(trainer, "_fused", None) is not None else None
    return {"trainer_acc_us_per_batch": round(us, 3), "trainer_acc_us_per_optimizer_step": round(us * args.k, 3),
            "trainer_step": fused, "trainer_global_step": int(trainer.global_step)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["all", "engine", "trainer"], default="all")
    ap.add_argument("-k", type=int, default=4, help="micro-batches per optimizer step")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--graph-steps", type=int, default=8)
    ap.add_argument("--n-data", type=int, default=55000)
    ap.add_argument("--trainer-steps", type=int, default=1000, help="batches per Trainer epoch")
    ap.add_argument("--trainer-epochs", type=int, default=3)
    ap.add_argument("--root", default="/tmp/bench_accumulate")
    args = ap.parse_args()
    res = {"k": args.k, "steps": args.steps, "warmup": args.warmup, "graph_steps": args.graph_steps}
    if args.only in ("all", "engine"):
        for mode in ("acc_eager", "acc_graph", "split"):
            us = bench_engine(args, mode)
            res[f"engine_{mode}_us_per_batch"] = round(us, 3)
            if mode != "split":
                res[f"engine_{mode}_us_per_optimizer_step"] = round(us * args.k, 3)
    if args.only in ("all", "trainer"):
        res.update(bench_trainer(args))
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
