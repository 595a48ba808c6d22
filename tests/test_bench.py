"""The benchmark entry point (``bench.py``) launches its own ranks.

``python bench.py --gpus N`` must start N ranks itself -- as runtime actors,
the RayAccelerator worker path -- and print ONE JSON line with the contract's
fields (it used to exit rc=1 without torchrun).  On CPU the ranks
run the engine's fp32 reference step over gloo.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
          "vs_baseline", "dtype", "data", "config")


def _bench(*args, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd="/tmp", env=e,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for k in FIELDS:
        assert k in out, k
    return out, p.stderr


@pytest.mark.parametrize("launcher", ["ray", "spawn"])
def test_bench_launches_two_cpu_ranks(launcher):
    out, err = _bench("--device", "cpu", "--gpus", "2", "--steps", "10", "--warmup", "2", "--launcher", launcher)
    assert out["n_gpus"] == 2 and out["steps"] == 10 and out["warmup"] == 2
    assert out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 64
    assert out["config"]["launch"] == ("ray-actors" if launcher == "ray" else "spawn")
    assert out["value"] > 0
    if launcher == "spawn":  # actor ranks log to the runtime session, not this stderr
        assert "world=2" in err
    # N > 1 diagnostics for the driver's multi-GPU run
    dp = out["dp"]
    assert dp["per_rank_us_per_step"]["min"] <= dp["per_rank_us_per_step"]["max"]
    assert abs(dp["per_rank_us_per_step"]["max"] - out["ms_per_step"] * 1e3) < 1e-2
    assert dp["process_group"] == {"backend": "gloo", "world": 2}
    assert out["config"]["route"] == "split-c10d-gloo"


def test_bench_compare_stock_cpu_fields():
    """--compare-stock: the stock torch step timed in the same job (both scaling curves
    from one command); on CPU only the plumbing is exercised -- the stock leg needs a GPU."""
    out, _ = _bench("--device", "cpu", "--gpus", "2", "--steps", "10", "--warmup", "2", "--compare-stock",
                    "--launcher", "spawn")
    assert out["n_gpus"] == 2 and "dp" in out and "stock" not in out


def test_bench_horovod_mode_cpu():
    out, _ = _bench("--device", "cpu", "--gpus", "2", "--steps", "10", "--warmup", "2", "--accelerator", "horovod")
    assert out["n_gpus"] == 2 and out["config"]["accelerator"] == "horovod"


def test_bench_single_rank_cpu():
    out, _ = _bench("--device", "cpu", "--steps", "10", "--warmup", "2")
    assert out["n_gpus"] == 1 and out["vs_baseline"] is None and out["dtype"] == "fp32"


def _load_dump(path):
    import numpy as np

    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".npy")}


def _dump_twice(tmp_path, *args, timeout=300):
    """Two runs of the same command line with --dump-outputs; asserts that the two
    dumps hold the same finite float32 arrays, bit for bit.  Returns (arrays, result line)."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        out, _ = _bench(*args, "--dump-outputs", str(tmp_path / name), timeout=timeout)
        dumps.append(_load_dump(tmp_path / name))
    a, b = dumps
    assert a and set(a) == set(b)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    return a, out


N_PARAMS = 784 * 32 + 32 + 32 * 64 + 64 + 64 * 10 + 10


def test_bench_dump_outputs_cpu_repeatable(tmp_path):
    """--dump-outputs: the state the last timed step left, float32, identical from run
    to run (seeded data and weights); --steps is the number of timed steps."""
    import numpy as np

    a, out = _dump_twice(tmp_path, "--device", "cpu", "--steps", "5", "--warmup", "1", "--n-data", "512")
    assert out["steps"] == 5 and out["ms_per_step"] > 0 and "stock" not in out
    assert set(a) == {"params", "exp_avg", "exp_avg_sq", "last_step_stats"}
    assert a["params"].shape == a["exp_avg"].shape == a["exp_avg_sq"].shape == (N_PARAMS,)
    # (loss, correct, count, step) of the last of the 1 + 5 steps
    assert a["last_step_stats"][2] == 32 and a["last_step_stats"][3] == 6
    assert np.abs(a["exp_avg"]).max() > 0


def test_bench_dump_outputs_stock_cpu_repeatable(tmp_path):
    """The stock step's dump (--impl torch): flattened parameters and the last loss."""
    a, out = _dump_twice(tmp_path, "--device", "cpu", "--impl", "torch", "--steps", "5", "--warmup", "1",
                         "--n-data", "512")
    assert out["config"]["impl"] == "torch" and set(a) == {"params", "loss"}
    assert a["params"].shape == (N_PARAMS,) and a["loss"].shape == (1,)
    assert abs(float(a["loss"][0]) - out["config"]["final_train_loss"]) < 1e-3


def test_bench_dump_outputs_via_trainer_cpu_repeatable(tmp_path):
    """--via trainer: the fit is seeded (initial weights in this process, the batch order
    in the workers through PL_GLOBAL_SEED), so the fitted weights it dumps repeat."""
    a, out = _dump_twice(tmp_path, "--device", "cpu", "--via", "trainer", "--trainer-epochs", "1", timeout=600)
    assert out["config"]["via"] == "trainer"
    assert {k: v.shape for k, v in a.items()} == {
        "layer_1.weight": (32, 784), "layer_1.bias": (32,), "layer_2.weight": (64, 32), "layer_2.bias": (64,),
        "layer_3.weight": (10, 64), "layer_3.bias": (10,)}


def test_dump_outputs_samples_large_arrays(tmp_path):
    """More than 64 MB: arrays above their share are cut to a sample of distinct elements
    that depends on nothing but the array's size and share (the same in every run, whatever
    else is dumped before it); small ones stay whole, float64 stays float64; the files
    together, headers included, stay within 64e6 bytes."""
    import importlib

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    assert bench.DUMP_LIMIT == 64_000_000
    big = torch.arange(20 << 20, dtype=torch.float32)  # 80 MiB; exact integers below 2^24
    arrays = {"big": big, "small": torch.ones(3, dtype=torch.bfloat16), "f64": torch.ones(2, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), dict(reversed(list(arrays.items()))))
    a, b = _load_dump(tmp_path / "a"), _load_dump(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64_000_000
    assert a["small"].dtype == np.float32 and a["small"].shape == (3,) and a["f64"].dtype == np.float64
    assert a["big"].dtype == np.float32 and 0 < a["big"].size < big.numel()
    assert np.array_equal(a["big"], b["big"]) and (np.diff(a["big"]) >= 0).all()
    exact = a["big"][a["big"] < 2 ** 24]
    assert exact.size > a["big"].size // 2 and (np.diff(exact) > 0).all()  # no element twice


def test_bench_refuses_non_finite_training():
    """a run whose training state goes non-finite (an injected NaN
    learning rate) is not a result -- bench.py exits non-zero and prints no JSON line."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--steps", "3",
                        "--warmup", "1", "--n-data", "512", "--lr", "nan"], cwd="/tmp", capture_output=True,
                       text=True, timeout=300)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")], p.stdout
    assert "non-finite" in p.stderr, p.stderr[-2000:]


def test_bench_via_trainer_cpu():
    out, _ = _bench("--device", "cpu", "--gpus", "2", "--via", "trainer", "--trainer-epochs", "2", timeout=600)
    assert out["n_gpus"] == 2 and out["config"]["accelerator"] == "RayAccelerator"
    assert len(out["epoch_wall_s"]) == 2 and out["config"]["checkpointing"]
    assert out["steps"] == 859  # one steady epoch of 27,500 / 32 batches per rank


@pytest.mark.gpu
def test_bench_two_ranks_share_gpu():
    """The N>1 GPU path (fused xGMI tail exchange, hipGraph) with two actor ranks on
    the box's one GPU (same-device IPC stands in for the xGMI link)."""
    out, err = _bench("--gpus", "2", "--steps", "200", "--warmup", "50", env={"RLA_BENCH_SHARE_GPU": "1"})
    assert out["n_gpus"] == 2 and out["config"]["route"] == "xgmi-fused", (out, err[-2000:])
    assert out["config"]["launch"] == "ray-actors"
    assert out["dp"]["comm_failed_validation"] == [] and out["dp"]["comm_error_state"] == 0


@pytest.mark.gpu
def test_bench_compare_stock_one_gpu():
    out, _ = _bench("--steps", "200", "--warmup", "20", "--compare-stock")
    assert out["stock"]["impl"] == "torch" and 0 < out["stock"]["value"] < out["value"]


@pytest.mark.gpu
def test_bench_full_and_dump_outputs_one_gpu(tmp_path):
    """The native step's dump on the GPU repeats bit for bit over two runs; --steps sets the
    number of steps the graph replays execute; --full adds the in-job stock comparison."""
    import numpy as np

    d, out = _dump_twice(tmp_path, "--steps", "40", "--warmup", "10", "--full")
    assert out["steps"] == 40 and out["ms_per_step"] > 0 and out["dtype"] == "bf16"
    assert out["stock"]["impl"] == "torch" and out["stock"]["value"] > 0
    assert set(d) == {"params", "exp_avg", "exp_avg_sq", "last_step_stats"}
    assert d["params"].shape == (N_PARAMS,) and np.abs(d["exp_avg"]).max() > 0
    # optimizer steps executed: the capture's eager step and first replay, the warm-up, the 40 timed
    g = out["config"]["hip_graph_steps"]
    assert g == 20 and d["last_step_stats"][2] == 32 and d["last_step_stats"][3] == 1 + g + 10 + 40


@pytest.mark.gpu
def test_bench_horovod_two_ranks_share_gpu_fused():
    """Config 3 (HorovodRayAccelerator) takes the fused in-kernel exchange by default
    (VERDICT r2 missing 2: it defaulted to the head/tail/allreduce/tail split)."""
    out, err = _bench("--gpus", "2", "--steps", "200", "--warmup", "50", "--accelerator", "horovod",
                      env={"RLA_BENCH_SHARE_GPU": "1"})
    assert out["config"]["accelerator"] == "horovod" and out["config"]["route"] == "xgmi-fused", (out, err[-2000:])
    assert out["config"]["step_kernel"] == "one-launch"


@pytest.mark.gpu
def test_bench_torch_graph_baseline():
    out, _ = _bench("--impl", "torch-graph", "--steps", "200", "--warmup", "20")
    assert out["n_gpus"] == 1 and out["config"]["impl"] == "torch-graph" and out["value"] > 0


@pytest.mark.gpu
def test_bench_resnet50_two_ranks_share_gpu_graph_captured():
    """ResNet-50 (config 5) at world 2 runs its data-parallel step as ONE hipGraph
    replay: forward, backward, the DDP buffer broadcast, every bucket's allreduce on
    the reducer's comm stream and the fused SGD (VERDICT r3 missing 2).  bench.py
    raises if the replicas differ after the timed steps."""
    out, err = _bench("--model", "resnet50", "--gpus", "2", "--steps", "6", "--warmup", "4", "--batch-size", "16",
                      "--bucket-mb", "4", env={"RLA_BENCH_SHARE_GPU": "1"}, timeout=600)
    assert out["n_gpus"] == 2 and out["config"]["route"] == "native-reducer", (out, err[-2000:])
    assert out["config"]["hip_graph"] is True, out
    assert out["dp"]["comm_error_state"] == 0 and out["dp"]["comm_failed_validation"] == [], out


@pytest.mark.gpu
def test_bench_resnet50_via_trainer_two_ranks_share_gpu():
    """Config 5 through RayAccelerator + Trainer.fit at world 2 (ranks sharing the
    GPU): the Trainer captures the autograd step (forward, backward, bucket
    allreduce, fused SGD) and replays it; replicas end bitwise equal."""
    out, err = _bench("--via", "trainer", "--model", "resnet50", "--gpus", "2", "--steps", "4", "--batch-size", "16",
                      "--trainer-epochs", "2", env={"RLA_BENCH_SHARE_GPU": "1"}, timeout=900)
    g = out["config"]["graph_step"]
    assert out["n_gpus"] == 2 and g["captured"] and g["resident_data"] and g["fallback"] is None, (out, err[-2000:])
    assert g["replays"] == g["steps"] - g["warmup_steps"], g
    assert out["replicas_equal"] is True, out


@pytest.mark.gpu
def test_bench_resnet50_torch_graph_baseline():
    out, _ = _bench("--model", "resnet50", "--impl", "torch-graph", "--steps", "4", "--warmup", "4",
                    "--batch-size", "16", timeout=600)
    assert out["config"]["impl"] == "torch-graph" and out["config"]["hip_graph"] is True and out["value"] > 0


def test_graph_steps_divide_the_timed_window():
    import importlib
    import sys

    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    assert bench.graph_steps_for(8, 20) == 20  # one replay covers the driver's 20-step window
    assert bench.graph_steps_for(8, 2000) == 25
    assert 2000 % bench.graph_steps_for(8, 2000) == 0
    assert bench.graph_steps_for(8, 2003) == 8  # prime window: fall back to the requested size
    assert bench.graph_steps_for(0, 20) == 0  # eager launches requested
