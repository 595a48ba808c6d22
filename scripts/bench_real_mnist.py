"""``Trainer.fit`` on MNIST read from IDX files with ``Normalize`` (one GPU, 784-32-64-10).

Writes ``--n`` synthetic MNIST-shaped images as torchvision-layout IDX files (real MNIST
cannot be downloaded here; the files have MNIST's format, size and dtype), then fits an
``MNISTClassifier`` whose loaders serve ``IdxMNIST(root, transform=Compose([Normalize((0.1307,),
(0.3081,))]))`` split 55,000 / 5,000, batch 32, and prints one JSON line: the route every
training batch and validation pass took, us/step and seconds per epoch (training + validation,
between two device synchronisations) of the epochs after the first.

On this tree the dataset stays resident (uint8 in HBM, the normalisation folded into the
kernels).  ``--loader`` wraps the transform in a way the resident path refuses, which is the
route every tree before the IDX reader took: per-batch DataLoader, fp32-input kernel, a Python
validation loop.  A tree given on PYTHONPATH wins, so the parent commit is measured with
``PYTHONPATH=<parent tree> python scripts/bench_real_mnist.py`` (it has no IDX reader: the
script then reads the files it wrote with the small dataset class below).
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

try:
    import ray_lightning_accelerators_amd  # noqa: F401  (a tree given on PYTHONPATH wins)
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader, Dataset, random_split  # noqa: E402

MEAN, STD = 0.1307, 0.3081


def write_idx(root: str, n: int) -> None:
    from ray_lightning_accelerators_amd.models.data import synthetic_mnist

    x, y = synthetic_mnist(n, seed=0)
    raw = os.path.join(root, "MNIST", "raw")
    os.makedirs(raw, exist_ok=True)
    with open(os.path.join(raw, "train-images-idx3-ubyte"), "wb") as f:
        f.write(struct.pack(">IIII", 0x00000803, n, 28, 28) + x.numpy().tobytes())
    with open(os.path.join(raw, "train-labels-idx1-ubyte"), "wb") as f:
        f.write(struct.pack(">II", 0x00000801, n) + y.to(torch.uint8).numpy().tobytes())


class _FileMNIST(Dataset):
    """The files above on a tree without ``models.data.IdxMNIST``: torchvision's attributes,
    ToTensor and Normalize in ``__getitem__``."""

    def __init__(self, root: str):
        raw = os.path.join(root, "MNIST", "raw")
        img = np.fromfile(os.path.join(raw, "train-images-idx3-ubyte"), dtype=np.uint8, offset=16)
        self.data = torch.from_numpy(img.reshape(-1, 28, 28).copy())
        self.targets = torch.from_numpy(
            np.fromfile(os.path.join(raw, "train-labels-idx1-ubyte"), dtype=np.uint8, offset=8).astype(np.int64))

    def __len__(self):
        return self.targets.numel()

    def __getitem__(self, i):
        return (self.data[i].view(1, 28, 28).float() / 255.0 - MEAN) / STD, int(self.targets[i])


class _Opaque:
    """A transform the resident path does not know (``--loader``)."""

    def __call__(self, x):
        return x


def make_dataset(root: str, loader: bool):
    try:
        from ray_lightning_accelerators_amd.models.data import Compose, IdxMNIST, Normalize
    except ImportError:
        return _FileMNIST(root), "tree without an IDX reader"
    chain = [Normalize((MEAN,), (STD,))] + ([_Opaque()] if loader else [])
    return IdxMNIST(root, train=True, transform=Compose(chain)), "IdxMNIST"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="where the IDX files go (default: a temporary directory)")
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--val", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=3, help="the first is warm-up")
    ap.add_argument("--loader", action="store_true", help="force the per-batch loader route")
    args = ap.parse_args()

    import ray_lightning_accelerators_amd.lightning as pl
    from ray_lightning_accelerators_amd.lightning import Callback
    from ray_lightning_accelerators_amd.models.mnist import LightningMNISTClassifier
    from ray_lightning_accelerators_amd.ops import fused_mlp

    tmp = None
    root = args.dir
    if root is None:
        tmp = tempfile.TemporaryDirectory()
        root = tmp.name
    write_idx(root, args.n)
    dataset, kind = make_dataset(root, args.loader)

    class Model(LightningMNISTClassifier):
        def prepare_data(self):
            if not hasattr(self, "_train_set"):
                self._train_set, self._val_set = random_split(
                    dataset, [args.n - args.val, args.val], generator=torch.Generator().manual_seed(0))

        def train_dataloader(self):
            self.prepare_data()
            return DataLoader(self._train_set, batch_size=args.batch, shuffle=True, drop_last=True)

        def val_dataloader(self):
            self.prepare_data()
            return DataLoader(self._val_set, batch_size=args.batch, drop_last=True)

    class Clock(Callback):
        def __init__(self):
            self.t0, self.epochs = None, []

        def on_train_epoch_start(self, trainer, pl_module):
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()

        def on_validation_end(self, trainer, pl_module):
            if trainer.running_sanity_check or self.t0 is None:
                return
            torch.cuda.synchronize()
            self.epochs.append(time.perf_counter() - self.t0)
            self.t0 = None

    counts = {"x_f32": 0}
    orig_step = fused_mlp.mlp_train_step

    def train_step(*a, **k):
        counts["x_f32"] += k.get("x_f32") is not None
        return orig_step(*a, **k)

    fused_mlp.mlp_train_step = train_step
    pl.seed_everything(0)
    model = Model({"layer_1": 32, "layer_2": 64, "lr": 1e-3, "batch_size": args.batch})
    clock = Clock()
    trainer = pl.Trainer(default_root_dir=os.path.join(root, "run"), gpus=1, max_epochs=args.epochs,
                         checkpoint_callback=False, progress_bar_refresh_rate=0, num_sanity_val_steps=0,
                         callbacks=[clock])
    assert trainer.fit(model) == 1
    torch.cuda.synchronize()
    f = trainer._fused
    eng = getattr(f, "eng", None)
    steps = (args.n - args.val) // args.batch
    timed = clock.epochs[1:] or clock.epochs
    epoch_s = sum(timed) / len(timed)
    print(json.dumps({
        "bench": "real_mnist_trainer", "dataset": kind, "n": args.n, "batch": args.batch, "normalize": [MEAN, STD],
        "route": "resident" if eng is not None and eng.global_step > 0 and counts["x_f32"] == 0 else "loader",
        "resident_steps": 0 if eng is None else int(eng.global_step), "loader_fed_steps": counts["x_f32"],
        "steps_per_epoch": steps, "epochs_timed": len(timed), "epoch_s": round(epoch_s, 4),
        "us_per_step_incl_validation": round(epoch_s / steps * 1e6, 2),
        "val_loss": float(trainer.callback_metrics["ptl/val_loss"]),
        "val_accuracy": float(trainer.callback_metrics["ptl/val_accuracy"]),
        "device": torch.cuda.get_device_name(0)}))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
