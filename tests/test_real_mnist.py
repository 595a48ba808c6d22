"""Real MNIST files and ``Normalize`` on the resident path -- the parts a CPU can check.

The IDX reader and ``IdxMNIST`` (models/data.py), ``input_affine`` (the one place that turns
a ``Normalize(mean, std)`` into the kernels' ``bf16(fmaf(u8, x_scale, x_shift))``), the
dataset / transform rules of ``models.mnist._u8_source``, ``MNISTDataModule`` over IDX files
and the CPU reference engine under ``normalize=``.  The GPU side is tests/test_real_mnist_gpu.py.
"""
import gzip
import math
import pickle
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import Subset, random_split

from ray_lightning_accelerators_amd.models.data import (Compose, IdxMNIST, Normalize, SyntheticMNIST, read_idx,
                                                        synthetic_mnist)
from ray_lightning_accelerators_amd.models.datamodules import MNISTDataModule
from ray_lightning_accelerators_amd.models.mnist import _u8_source
from ray_lightning_accelerators_amd.ops import fused_mlp
from ray_lightning_accelerators_amd.parallel.mlp_engine import FusedMLPEngine, shard_indices

MNIST_NORM = (0.1307, 0.3081)


# ------------------------------------------------------------------ helpers
def _idx_bytes(arr: np.ndarray) -> bytes:
    """``arr`` (uint8, [n] labels or [n, r, c] images) as an IDX file's bytes."""
    magic = 0x00000800 | arr.ndim
    return struct.pack(">I", magic) + b"".join(struct.pack(">I", d) for d in arr.shape) + arr.tobytes()


def _write(path, data: bytes, gz: bool = False):
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(data)
    return str(path)


def write_mnist(root, n_train=48, n_test=16, gz=False, nested=True, seed=0):
    """Tiny MNIST-layout IDX files under ``root`` (torchvision's MNIST/raw when ``nested``)
    from the synthetic generator; returns {split: (images [n, 784], labels [n])}."""
    d = root / "MNIST" / "raw" if nested else root
    d.mkdir(parents=True, exist_ok=True)
    ext = ".gz" if gz else ""
    out = {}
    for stem, n, s in (("train", n_train, seed), ("t10k", n_test, seed + 1)):
        x, y = synthetic_mnist(n, seed=s)
        _write(d / f"{stem}-images-idx3-ubyte{ext}", _idx_bytes(x.view(n, 28, 28).numpy()), gz)
        _write(d / f"{stem}-labels-idx1-ubyte{ext}", _idx_bytes(y.to(torch.uint8).numpy()), gz)
        out[stem] = (x, y)
    return out


# ------------------------------------------------------------------ IDX reader
@pytest.mark.parametrize("gz", [False, True])
def test_read_idx_round_trip(tmp_path, gz):
    g = np.random.default_rng(0)
    img = g.integers(0, 256, (5, 28, 28), dtype=np.uint8)
    lab = g.integers(0, 10, (5,), dtype=np.uint8)
    ext = ".gz" if gz else ""
    xi = read_idx(_write(tmp_path / f"i-idx3-ubyte{ext}", _idx_bytes(img), gz))
    yi = read_idx(_write(tmp_path / f"l-idx1-ubyte{ext}", _idx_bytes(lab), gz))
    assert xi.dtype == torch.uint8 and tuple(xi.shape) == (5, 28, 28) and np.array_equal(xi.numpy(), img)
    assert yi.dtype == torch.uint8 and tuple(yi.shape) == (5,) and np.array_equal(yi.numpy(), lab)


def test_read_idx_refusals(tmp_path):
    img = np.zeros((3, 28, 28), dtype=np.uint8)
    good = _idx_bytes(img)
    cases = {
        "bad magic": struct.pack(">I", 0x00000802) + good[4:],
        "float magic": struct.pack(">I", 0x00000D03) + good[4:],
        "other size": _idx_bytes(np.zeros((3, 32, 32), dtype=np.uint8)),
        "truncated": good[:-1],
        "truncated header": good[:10],
        "empty": b"",
        "over-long": good + b"\0",
        "labels over-long": _idx_bytes(np.zeros(4, dtype=np.uint8)) + b"\1",
        "labels truncated": _idx_bytes(np.zeros(4, dtype=np.uint8))[:-2],
    }
    for name, data in cases.items():
        for gz in (False, True):
            p = _write(tmp_path / (name.replace(" ", "_") + (".gz" if gz else "")), data, gz)
            with pytest.raises(ValueError):
                read_idx(p)


@pytest.mark.parametrize("gz,nested", [(False, True), (True, True), (False, False), (True, False)])
def test_idx_mnist_layouts_and_items(tmp_path, gz, nested):
    data = write_mnist(tmp_path, gz=gz, nested=nested)
    for train, stem in ((True, "train"), (False, "t10k")):
        x, y = data[stem]
        ds = IdxMNIST(str(tmp_path), train=train)
        assert ds.data.dtype == torch.uint8 and tuple(ds.data.shape) == (x.size(0), 28, 28)
        assert ds.targets.dtype == torch.int64 and torch.equal(ds.targets, y)
        assert torch.equal(ds.data.view(-1, 784), x) and len(ds) == x.size(0)
        xi, yi = ds[3]
        assert isinstance(yi, int) and yi == int(y[3])
        assert xi.dtype == torch.float32 and tuple(xi.shape) == (1, 28, 28)
        assert torch.equal(xi, x[3].view(1, 28, 28).float() / 255.0)
    tf = Compose([Normalize((0.1307,), (0.3081,))])
    ds = IdxMNIST(str(tmp_path), train=True, transform=tf, target_transform=lambda t: t + 1)
    xi, yi = ds[5]
    assert torch.equal(xi, (data["train"][0][5].view(1, 28, 28).float() / 255.0 - 0.1307) / 0.3081)
    assert yi == int(data["train"][1][5]) + 1


def test_idx_mnist_refuses_missing_and_mismatched_files(tmp_path):
    with pytest.raises(FileNotFoundError):
        IdxMNIST(str(tmp_path))
    write_mnist(tmp_path, n_train=8)
    raw = tmp_path / "MNIST" / "raw"
    _write(raw / "train-labels-idx1-ubyte", _idx_bytes(np.zeros(7, dtype=np.uint8)))
    with pytest.raises(ValueError, match="8 images.*7 labels"):
        IdxMNIST(str(tmp_path))
    # an image file where the labels belong
    _write(raw / "train-labels-idx1-ubyte", _idx_bytes(np.zeros((8, 28, 28), dtype=np.uint8)))
    with pytest.raises(ValueError):
        IdxMNIST(str(tmp_path))


# ------------------------------------------------------------------ input_affine
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_input_affine_default_is_the_old_product_bitwise():
    u = torch.arange(256, dtype=torch.uint8)
    old = u.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)  # the kernels' u8 * (1.0f / 255.0f)
    assert np.float32(1.0) / np.float32(255.0) == np.float32(1.0 / 255.0)  # either constant
    for norm in (None, (0.0, 1.0), ((0.0,), (1.0,))):
        sc, sh = fused_mlp.input_affine(norm)
        assert sc == float(np.float32(1.0 / 255.0)) and sh == 0.0 and math.copysign(1.0, sh) == 1.0
        new = fused_mlp.u8_to_input(u, sc, sh)
        assert new.dtype == torch.float32 and torch.equal(_bits(new), _bits(old))
    assert fused_mlp.input_affine(None) == (fused_mlp.X_SCALE_DEFAULT, 0.0)


@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (0.5, 0.5), MNIST_NORM])
def test_input_affine_equals_torch_normalize_in_bf16(mean, std):
    """The FMA form, rounded to bf16 as the kernels do, is torch's ((u8 / 255) - m) / s -> bf16
    for every byte value."""
    u = torch.arange(256, dtype=torch.uint8)
    sc, sh = fused_mlp.input_affine((mean, std))
    fma = fused_mlp.u8_to_input(u, sc, sh).to(torch.bfloat16)
    ref = ((u.float() / 255.0 - mean) / std).to(torch.bfloat16)
    assert int((_bits(fma) != _bits(ref)).sum()) == 0
    via_transform = Normalize((mean,), (std,))((u.float() / 255.0).view(1, 16, 16)).to(torch.bfloat16).view(-1)
    assert int((_bits(fma) != _bits(via_transform)).sum()) == 0


@pytest.mark.parametrize("mean,std", [(0.2, 0.7), (-1.5, 3.0), (0.4567, 0.0123), (123.0, 456.0)])
def test_input_affine_is_its_formula(mean, std):
    sc, sh = fused_mlp.input_affine(((mean,), [std]))
    assert sc == float(np.float32(1.0 / (255.0 * std))) and sh == float(np.float32(-mean / std))
    u = torch.arange(256, dtype=torch.uint8)
    want = torch.from_numpy((u.numpy().astype(np.float64) * sc + sh).astype(np.float32))
    assert torch.equal(_bits(fused_mlp.u8_to_input(u, sc, sh)), _bits(want))
    assert fused_mlp.input_affine((torch.tensor([mean]), torch.tensor([std])))[0] == pytest.approx(sc, rel=1e-6)


@pytest.mark.parametrize("norm", [(0.1, 0.0), (0.1, -1.0), (0.1, float("nan")), (0.1, float("inf")),
                                  (float("nan"), 1.0), (float("inf"), 1.0), ((0.1, 0.2, 0.3), (1.0, 1.0, 1.0)),
                                  (0.0, 1e-45), (1e38, 1e-3)])
def test_input_affine_refuses(norm):
    with pytest.raises(ValueError):
        fused_mlp.input_affine(norm)


@pytest.mark.parametrize("sc,sh", [(float("nan"), 0.0), (float("inf"), 0.0), (0.0, 0.0), (-1.0, 0.0),
                                   (1.0, float("nan")), (1.0, float("inf")), (1e300, 0.0), (1e-300, 0.0)])
def test_reference_launches_refuse_a_bad_pixel_map(sc, sh):
    """The CPU reference paths apply the kernels' rule (finite positive fp32 scale, finite shift)."""
    x, y = synthetic_mnist(8, seed=0)
    p = fused_mlp.init_mlp_params(32, 32, torch.Generator().manual_seed(0))
    with pytest.raises(ValueError):
        fused_mlp.mlp_eval(p, L1=32, L2=32, B=8, labels=y, out=torch.zeros(2), x_u8=x, index=torch.arange(8),
                           x_scale=sc, x_shift=sh)
    with pytest.raises(ValueError):
        fused_mlp.mlp_train_step(p, torch.zeros_like(p), L1=32, L2=32, B=8, labels=y, x_u8=x, order=torch.arange(8),
                                 counters=torch.zeros(2, dtype=torch.int64), n_batches=1, x_scale=sc, x_shift=sh)


# ------------------------------------------------------------------ _u8_source
class ToTensor:  # matched by class name, as torchvision's
    pass


class TVNormalize:
    """A stand-in for torchvision's Normalize: another class of the same NAME."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std


TVNormalize.__name__ = "Normalize"


class TVCompose:
    def __init__(self, transforms):
        self.transforms = transforms


class Foreign:
    """torchvision.datasets.MNIST's attributes without torchvision."""

    def __init__(self, n=40, transform=None, target_transform=None, flat=False, list_targets=False):
        x, y = synthetic_mnist(n, seed=3)
        self.data = x if flat else x.view(n, 28, 28)
        self.targets = y.tolist() if list_targets else y
        self.transform, self.target_transform = transform, target_transform


class RandomErasing:
    pass


def test_u8_source_accepts():
    x, y = synthetic_mnist(40, seed=3)
    # .images, as before
    src = _u8_source(SyntheticMNIST(64, seed=0))
    assert src is not None and src[0].shape == (64, 784) and src[2] is None and src[3] is None
    # torchvision layout: ToTensor alone, ToTensor + Normalize (our class and a foreign one of that name)
    for flat in (False, True):
        for lt in (False, True):
            src = _u8_source(Foreign(transform=TVCompose([ToTensor()]), flat=flat, list_targets=lt))
            assert src is not None and src[3] is None
            assert src[0].dtype == torch.uint8 and torch.equal(src[0], x) and torch.equal(src[1], y)
    assert _u8_source(Foreign(transform=ToTensor()))[3] is None  # bare, no Compose
    for norm in (TVNormalize((0.1307,), (0.3081,)), Normalize((0.1307,), (0.3081,)), TVNormalize(0.1307, 0.3081),
                 TVNormalize(torch.tensor([0.1307]), torch.tensor([0.3081]))):
        src = _u8_source(Foreign(transform=TVCompose([ToTensor(), norm])))
        assert src is not None and src[3] == pytest.approx(MNIST_NORM)
    # nested Compose flattens
    src = _u8_source(Foreign(transform=TVCompose([TVCompose([ToTensor()]), Compose([Normalize((0.5,), (0.5,))])])))
    assert src is not None and src[3] == (0.5, 0.5)
    # SyntheticMNIST with a transform: ToTensor is built in
    assert _u8_source(SyntheticMNIST(64, seed=0, transform=Normalize((0.5,), (0.5,))))[3] == (0.5, 0.5)


def test_u8_source_idx_mnist_and_subset_chains(tmp_path):
    data = write_mnist(tmp_path, n_train=48)
    ds = IdxMNIST(str(tmp_path), transform=Compose([Normalize((0.1307,), (0.3081,))]))
    images, targets, idx_map, norm = _u8_source(ds)
    assert idx_map is None and norm == MNIST_NORM
    assert images.shape == (48, 784) and images.data_ptr() == ds.data.data_ptr()  # a view, no copy
    assert torch.equal(images, data["train"][0]) and torch.equal(targets, data["train"][1])
    assert _u8_source(IdxMNIST(str(tmp_path)))[3] is None
    tr, va = random_split(ds, [40, 8], generator=torch.Generator().manual_seed(1))
    inner = Subset(tr, [5, 0, 7])
    for sub, want in ((tr, list(tr.indices)), (va, list(va.indices)), (inner, [tr.indices[i] for i in (5, 0, 7)])):
        images, targets, idx_map, norm = _u8_source(sub)
        assert norm == MNIST_NORM and idx_map.tolist() == want
        for k in range(len(sub)):
            xk, yk = sub[k]
            sc, sh = fused_mlp.input_affine(norm)
            got = fused_mlp.u8_to_input(images[idx_map[k]], sc, sh).to(torch.bfloat16)
            assert torch.equal(got, xk.reshape(-1).to(torch.bfloat16)) and int(targets[idx_map[k]]) == yk


def test_u8_source_rejects():
    ok = TVCompose([ToTensor(), TVNormalize((0.5,), (0.5,))])
    assert _u8_source(Foreign(transform=ok)) is not None
    rejected = {
        "unknown transform": Foreign(transform=TVCompose([ToTensor(), RandomErasing()])),
        "unknown transform alone": SyntheticMNIST(64, seed=0, transform=lambda t: t * 2),
        "target_transform": Foreign(transform=ok, target_transform=lambda t: t),
        "3-channel Normalize": Foreign(transform=TVCompose([ToTensor(), TVNormalize((0.5,) * 3, (0.5,) * 3)])),
        "two Normalizes": Foreign(transform=TVCompose([ToTensor(), TVNormalize((0.5,), (0.5,)),
                                                       TVNormalize((0.5,), (0.5,))])),
        "std 0": Foreign(transform=TVCompose([ToTensor(), TVNormalize((0.5,), (0.0,))])),
        "foreign without ToTensor": Foreign(transform=None),
        "foreign Normalize without ToTensor": Foreign(transform=TVNormalize((0.5,), (0.5,))),
        "foreign ToTensor not first": Foreign(transform=TVCompose([TVNormalize((0.5,), (0.5,)), ToTensor()])),
    }
    for name, ds in rejected.items():
        assert _u8_source(ds) is None, name
        assert _u8_source(Subset(ds, [0, 1])) is None, name
    f = Foreign(transform=ok)
    f.data = f.data.float()
    assert _u8_source(f) is None  # not uint8
    f = Foreign(transform=ok)
    f.data = f.data[:, :14]
    assert _u8_source(f) is None  # not 28 x 28
    assert _u8_source(object()) is None


# ------------------------------------------------------------------ MNISTDataModule
def test_datamodule_empty_dir_stays_synthetic(tmp_path):
    dm = MNISTDataModule(data_dir=str(tmp_path), n_train=256, val_split=64, n_test=32)
    dm.setup()
    full = dm._train.dataset
    assert isinstance(full, SyntheticMNIST) and full.transform is None and isinstance(dm._test, SyntheticMNIST)
    ref = SyntheticMNIST(256, seed=0, train=True)
    assert torch.equal(full.images, ref.images) and torch.equal(full.targets, ref.targets)
    want = random_split(ref, [192, 64], generator=torch.Generator().manual_seed(42))
    assert list(dm._train.indices) == list(want[0].indices) and list(dm._val.indices) == list(want[1].indices)
    x, y = dm._train[0]
    assert torch.equal(x, ref[dm._train.indices[0]][0]) and float(x.min()) >= 0.0
    assert len(dm._test) == 32
    xb, yb = next(iter(dm.train_dataloader()))
    assert tuple(xb.shape) == (32, 1, 28, 28)


def test_datamodule_reads_idx_files_and_normalizes(tmp_path):
    data = write_mnist(tmp_path, n_train=96, n_test=40)
    dm = MNISTDataModule(data_dir=str(tmp_path), val_split=32, batch_size=16)
    dm.setup()
    assert isinstance(dm._train.dataset, IdxMNIST) and dm._train.dataset is dm._val.dataset
    assert len(dm._train) == 64 and len(dm._val) == 32 and dm._train.dataset.transform is None
    assert isinstance(dm._test, IdxMNIST) and not dm._test.train and len(dm._test) == 40
    assert torch.equal(dm._test.data.view(-1, 784), data["t10k"][0])
    assert _u8_source(dm._train)[3] is None
    dn = MNISTDataModule(data_dir=str(tmp_path), val_split=32, batch_size=16, normalize=True)
    dn.setup()
    assert list(dn._train.indices) == list(dm._train.indices)  # the same split
    for k in (0, 17, 63):
        (x0, y0), (x1, y1) = dm._train[k], dn._train[k]
        assert y0 == y1 and torch.equal(x1, (x0 - 0.5) / 0.5)
    assert torch.equal(dn._test[7][0], (dm._test[7][0] - 0.5) / 0.5)
    assert _u8_source(dn._train)[3] == (0.5, 0.5) and _u8_source(dn._val)[3] == (0.5, 0.5)
    xb, _ = next(iter(dn.val_dataloader()))
    assert tuple(xb.shape) == (16, 1, 28, 28) and float(xb.min()) >= -1.0 and float(xb.max()) <= 1.0
    # synthetic data normalises the same way
    ds = MNISTDataModule(data_dir=None, n_train=128, val_split=32, normalize=True)
    ds.setup("fit")
    base = SyntheticMNIST(128, seed=0)
    i = ds._train.indices[0]
    assert torch.equal(ds._train[0][0], (base[i][0] - 0.5) / 0.5)


def test_synthetic_mnist_pickles_with_its_transform():
    ds = SyntheticMNIST(64, seed=0, transform=Normalize((0.1307,), (0.3081,)))
    blob = pickle.dumps(ds)
    assert len(blob) < 2000  # by spec, not by value
    back = pickle.loads(blob)
    assert isinstance(back.transform, Normalize)
    assert back.transform.mean == (0.1307,) and back.transform.std == (0.3081,)
    assert torch.equal(back.images, ds.images) and torch.equal(back[5][0], ds[5][0]) and back[5][1] == ds[5][1]
    plain = pickle.loads(pickle.dumps(SyntheticMNIST(64, seed=0)))
    assert plain.transform is None and torch.equal(plain[5][0], ds.images[5].view(1, 28, 28).float() / 255.0)
    assert isinstance(pickle.loads(pickle.dumps(Compose([Normalize((0.5,), (0.5,))]))).transforms[0], Normalize)


# ------------------------------------------------------------------ reference engine
def _autograd_grads(params, x, y, L1, L2):
    leaf = params.detach().clone().requires_grad_(True)
    p = fused_mlp.mlp_unpack(leaf, L1, L2)
    h = torch.relu(F.linear(x, p["layer_1.weight"], p["layer_1.bias"]))
    h = torch.relu(F.linear(h, p["layer_2.weight"], p["layer_2.bias"]))
    F.nll_loss(torch.log_softmax(F.linear(h, p["layer_3.weight"], p["layer_3.bias"]), 1), y).backward()
    return leaf.grad


@pytest.mark.parametrize("norm", [MNIST_NORM, (0.5, 0.5)])
def test_reference_engine_gradient_under_normalize(norm):
    """The CPU (non-native) engine with ``normalize=``: the gradient handed to the allreduce is
    fp32 autograd on the bf16-rounded FMA-normalised batch (what the kernels feed layer 1), to
    1e-6 absolute -- the CPU engine tests' tolerance."""
    L1, L2, B = 32, 64, 16
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (4 * B, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (4 * B,), generator=g)
    got = []
    eng = FusedMLPEngine(L1, L2, B, lr=1e-2, world_size=2, rank=0,
                         allreduce=lambda t: (got.append(t.clone()), t.mul_(2)))
    eng.set_data(x, y, normalize=norm)
    assert not eng.native and eng.normalize == norm
    assert (eng.x_scale, eng.x_shift) == fused_mlp.input_affine(norm)
    p0 = eng.params.clone()
    eng.step()
    idx = shard_indices(4 * B, 2, 0, 0, 0, True)[:B]
    xn = fused_mlp.u8_to_input(x[idx], *fused_mlp.input_affine(norm))
    n = fused_mlp.mlp_param_count(L1, L2)
    ref = _autograd_grads(p0, xn.to(torch.bfloat16).float(), y[idx], L1, L2)
    print("max |diff|", float((got[0][:n] - ref).abs().max()))
    assert torch.allclose(got[0][:n], ref, rtol=0, atol=1e-6)
    # ... and it is not the un-normalised gradient
    assert not torch.allclose(got[0][:n], _autograd_grads(p0, x[idx].float() / 255.0, y[idx], L1, L2), atol=1e-4)


def test_reference_engine_identity_normalize_is_bitwise_the_default():
    g = torch.Generator().manual_seed(6)
    x = torch.randint(0, 256, (80, 784), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 10, (80,), generator=g)
    a, b = FusedMLPEngine(32, 32, 16, lr=1e-2), FusedMLPEngine(32, 32, 16, lr=1e-2)
    a.set_data(x, y)
    b.set_data(x, y, normalize=(0.0, 1.0))
    for _ in range(7):
        a.step()
        b.step()
    for k in ("params", "exp_avg", "exp_avg_sq", "stats", "counters"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_engine_changed_normalize_drops_graphs_and_reprimes():
    x, y = synthetic_mnist(96, seed=0)
    eng = FusedMLPEngine(32, 64, 32, lr=1e-3)
    eng.attach_dataset(x, y)
    eng.begin_epoch(torch.arange(96), 3)
    eng.step()
    assert eng._primed
    eng._graph, eng._tail_graphs = object(), {1: object()}
    eng.attach_dataset(x, y)  # the same map: nothing is dropped
    assert eng._primed and eng._graph is not None
    eng.attach_dataset(x, y, normalize=MNIST_NORM)
    assert not eng._primed and eng._graph is None and eng._tail_graphs == {}
    assert (eng.x_scale, eng.x_shift) == fused_mlp.input_affine(MNIST_NORM)
    assert eng._kw3()["x_scale"] == eng.x_scale and eng._kw3()["x_shift"] == eng.x_shift
    with pytest.raises(ValueError):
        eng.attach_dataset(x, y, normalize=(0.5, 0.0))


def test_normalize_takes_the_exchange_out_of_the_one_launch_step(caplog):
    """The one-launch kernel has Normalize instances at world size 1 only: with an exchange
    context a normalised dataset runs the two-launch step, and says so once."""
    import logging

    x, y = synthetic_mnist(96, seed=0)
    eng = FusedMLPEngine(32, 64, 32, lr=1e-3)
    assert eng.one_launch and eng.dp_ctx is None and not eng.one_launch_dp
    eng.dp_ctx = [2, 0, fused_mlp.DP_AREA_FLOATS, 1000, 0, 0, 0, 0]  # what a GPU engine keeps of dp_context
    eng.set_dp_proto("packed", rearm=False)
    assert eng.one_launch_dp
    with caplog.at_level(logging.WARNING, logger="ray_lightning_accelerators_amd.parallel.mlp_engine"):
        eng.attach_dataset(x, y)  # ToTensor alone: nothing changes, nothing is said
        assert eng.one_launch_dp and not caplog.records
        eng.attach_dataset(x, y, normalize=MNIST_NORM)
        assert not eng.one_launch_dp and len(caplog.records) == 1 and "two launches" in caplog.text
        eng.attach_dataset(x, y, normalize=(0.5, 0.5))
        assert not eng.one_launch_dp and len(caplog.records) == 1
    eng.attach_dataset(x, y, normalize=(0.0, 1.0))  # the default map again
    assert eng.one_launch_dp
    with pytest.raises(ValueError, match="MLP3_STEP1_DP"):  # the launch wrapper refuses the pair outright
        fused_mlp.mlp3_launch(fused_mlp.MLP3_STEP1_DP, stats=None,
                              **{**eng._kw3(), "x_scale": 0.0127, "x_shift": -0.42})


def test_step_looks_at_a_reassigned_transform_again():
    """``FusedMNISTStep._source`` caches per dataset object, but not past a new ``transform``."""
    from ray_lightning_accelerators_amd.models.mnist import FusedMNISTStep

    step = object.__new__(FusedMNISTStep)  # _source needs no device state
    ds = SyntheticMNIST(64, seed=0)
    sub = Subset(ds, list(range(40)))
    first = step._source(sub)
    assert first[3] is None and step._source(sub) is first  # cached
    ds.transform = Normalize((0.5,), (0.5,))
    second = step._source(sub)
    assert second is not first and second[3] == (0.5, 0.5) and step._source(sub) is second
    ds.transform = lambda t: t + 1  # nothing the kernels reproduce: the loader route
    assert step._source(sub) is None
    ds.transform = None
    assert step._source(sub)[3] is None
    ds.target_transform = int
    assert step._source(sub) is None
