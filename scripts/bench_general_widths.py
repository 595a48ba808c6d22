"""Cost of the general-width fused MNIST step (one GPU, csrc/mlp_step_general.hip).

Two arms, one JSON line per configuration and round:

  --arm trainer   ``Trainer.fit`` of ``MNISTClassifier`` at each ``--widths`` x ``--batches``:
                  us per step as (wall time of a fit of ``--hi`` batches - one of ``--lo``
                  batches) / (hi - lo), each fit ending in a device synchronise -- set-up, graph
                  capture and teardown cancel.  ``route`` says what the Trainer ran: "fused"
                  (``FusedMNISTStep`` with an engine) or "autograd" (the fallback, which is what
                  a tree without the general kernels runs at these widths).  Uses the public
                  Trainer interface only, so the same file times any tree given on PYTHONPATH.
                  ``--fused-step off`` passes ``Trainer(fused_step=False)``: the autograd path of
                  this tree, which is the fallback itself wherever a tree has no kernel.
  --arm routes    ``FusedMLPEngine(128, 256, B, route=...)`` in captured graphs of
                  ``--graph-steps`` steps: "general" (the general-width kernels forced on a table
                  pair) against "auto" (B = 32 the one-launch step, 256 the two-launch step, 512
                  the wide step), device events around ``--steps`` steps after ``--warmup``.

``--rounds`` interleaved rounds, so every line of a round saw the same machine.
"""
import argparse
import json
import os
import sys
import tempfile
import time

try:
    import ray_lightning_accelerators_amd  # noqa: F401  (a tree given on PYTHONPATH wins)
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def fit_seconds(l1: int, l2: int, B: int, n: int, root: str, fused_step=None):
    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.models.mnist import MNISTClassifier

    pl.seed_everything(0)
    model = MNISTClassifier({"layer_1": l1, "layer_2": l2, "lr": 1e-3, "batch_size": B})
    model.prepare_data()  # the synthetic dataset is built outside the timed window
    tr = pl.Trainer(default_root_dir=root, gpus=1, max_epochs=1, limit_train_batches=n, limit_val_batches=0,
                    checkpoint_callback=False, progress_bar_refresh_rate=0, num_sanity_val_steps=0, logger=False,
                    fused_step=fused_step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.fit(model)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert tr.global_step == n, (tr.global_step, n)
    fused = getattr(tr, "_fused", None)
    return dt, "fused" if fused is not None and getattr(fused, "eng", None) is not None else "autograd"


def arm_trainer(args) -> None:
    cfgs = [(w, B) for w in args.widths.split(",") for B in (int(b) for b in args.batches.split(","))]
    fs = False if args.fused_step == "off" else None
    with tempfile.TemporaryDirectory() as root:
        for w, B in cfgs:  # warm every shape: code objects, allocator
            l1, l2 = (int(v) for v in w.split("-"))
            fit_seconds(l1, l2, B, args.lo, root, fs)
        for rnd in range(args.rounds):
            for w, B in cfgs:
                l1, l2 = (int(v) for v in w.split("-"))
                lo, route = fit_seconds(l1, l2, B, args.lo, root, fs)
                hi, route2 = fit_seconds(l1, l2, B, args.hi, root, fs)
                assert route == route2
                print(json.dumps({"arm": "trainer", "tag": args.tag, "round": rnd, "widths": w, "batch": B,
                                  "route": route, "us_per_step": round((hi - lo) / (args.hi - args.lo) * 1e6, 2),
                                  "fit_lo_s": round(lo, 4), "fit_hi_s": round(hi, 4)}), flush=True)


def timed_us(run, steps: int) -> float:
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def arm_routes(args) -> None:
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist
    from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

    data = synthetic_mnist(16384, seed=0)
    l1, l2 = 128, 256
    runs = []
    for B in (int(b) for b in args.batches.split(",")):
        for route in ("auto", "general"):
            eng = FusedMLPEngine(l1, l2, B, lr=1e-3, device=torch.device("cuda", 0), route=route)
            eng.set_data(*data)
            assert eng.capture(args.graph_steps)
            eng.run(args.warmup)
            kind = "general" if eng.general else "wide" if eng.wide else "one_launch" if eng.one_launch else "two_launch"
            runs.append((B, route, kind, eng))
    for rnd in range(args.rounds):
        for B, route, kind, eng in runs:
            print(json.dumps({"arm": "routes", "round": rnd, "widths": f"{l1}-{l2}", "batch": B, "route": route,
                              "kernels": kind, "us_per_step": round(timed_us(eng.run, args.steps), 3)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["trainer", "routes"], required=True)
    ap.add_argument("--tag", default="this_tree")
    ap.add_argument("--widths", default="256-256,512-512")
    ap.add_argument("--batches", default="32,512")
    ap.add_argument("--lo", type=int, default=16)
    ap.add_argument("--hi", type=int, default=96)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--graph-steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused-step", choices=["auto", "off"], default="auto")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_general_widths needs a GPU")
    (arm_trainer if args.arm == "trainer" else arm_routes)(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
