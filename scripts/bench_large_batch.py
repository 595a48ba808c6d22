"""Cost of the wide-batch fused MNIST step (one GPU, 784-L1-L2-10, 256 < B <= 4096).

Prints one JSON line per (widths, B) and round with us/step and samples/s of
  wide          FusedMLPEngine(L1, L2, B): the wide step (csrc/mlp_step_wide.hip), three
                launches per step, in a captured graph of ``--graph-steps`` steps
  two_launch_256  the same widths at B = 256 on the pipelined two-launch step: the fastest
                configuration that existed before the wide step (it could not run these batches)
  torch_graph   nn.Linear x 3 + torch.optim.Adam(capturable) on a resident fp32 batch under
                torch.cuda.graph at the same B
each over ``--steps`` steps after ``--warmup``, timed with device events between two
synchronisations; ``--rounds`` interleaved rounds, so every line of a round saw the same machine.
"""
import argparse
import json
import os
import sys

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


def make_engine(args, l1, l2, B, data):
    from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine

    eng = FusedMLPEngine(l1, l2, B, lr=args.lr, device=torch.device("cuda", 0))
    eng.set_data(*data)
    assert eng.capture(args.graph_steps)
    eng.run(args.warmup)
    return eng.run


def make_torch(args, l1, l2, B, data):
    dev = torch.device("cuda", 0)
    net = torch.nn.Sequential(torch.nn.Linear(784, l1), torch.nn.ReLU(), torch.nn.Linear(l1, l2), torch.nn.ReLU(),
                              torch.nn.Linear(l2, 10)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=args.lr, capturable=True)
    x = (data[0][:B].float() / 255.0).to(dev)
    y = data[1][:B].to(dev)

    def one():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(net(x), y).backward()
        opt.step()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            one()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(args.graph_steps):
            one()

    def run(n):
        for _ in range(max(1, n // args.graph_steps)):
            g.replay()

    run.keep = (net, opt, x, y)  # the graph replays on their memory: they live as long as it does
    run(args.warmup)
    return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="128-256,32-64")
    ap.add_argument("--batches", default="512,1024,2048,4096")
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--graph-steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-data", type=int, default=16384)
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_large_batch needs a GPU")
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist
    from ray_lightning_accelerators_amd.ops import fused_mlp

    data = synthetic_mnist(args.n_data, seed=0)
    runs = []
    for w in args.widths.split(","):
        l1, l2 = (int(v) for v in w.split("-"))
        runs.append((w, "two_launch_256", 256, make_engine(args, l1, l2, 256, data), None))
        for B in (int(b) for b in args.batches.split(",")):
            lay = fused_mlp.mlp_wide_layout(l1, l2, B)
            split = {"slabs": lay["nslab"], "slices": lay["slices"], "reduction": "third launch"}
            runs.append((w, "wide", B, make_engine(args, l1, l2, B, data), split))
            try:
                runs.append((w, "torch_graph", B, make_torch(args, l1, l2, B, data), None))
            except Exception as exc:  # reported, never replaced by another route
                print(json.dumps({"widths": w, "route": "torch_graph", "batch": B, "error": repr(exc)[:200]}), flush=True)
    for rnd in range(args.rounds):
        for w, name, B, run, split in runs:
            us = timed_us(run, args.steps)
            print(json.dumps({"round": rnd, "widths": w, "route": name, "batch": B, "us_per_step": round(us, 3),
                              "samples_per_s": round(B / us * 1e6), **(split or {})}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
