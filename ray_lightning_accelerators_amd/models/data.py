"""MNIST-shaped data: a synthetic generator (no downloads are possible on this platform)
and a reader of real MNIST's IDX files (``read_idx`` / ``IdxMNIST``) with the two tensor
transforms that go with them (``Normalize`` / ``Compose``).

``synthetic_mnist`` produces uint8 28x28 images of a *learnable but noisy*
10-class task (overlapping class-conditional blob prototypes, per-sample
displacement, distractors, noise and label noise), so the reference's accuracy
gate (>= 0.5 after 10 train batches, ray_lightning/tests/utils.py:137-152 of the
reference) stays meaningful and converged runs keep a non-degenerate loss.
Images are uint8 like real MNIST; the ``ToTensor`` scaling (x / 255) happens
in the dataset's ``__getitem__`` on CPU or inside the fused kernel on GPU.
"""
from __future__ import annotations

import gzip
import math
import os
import struct
import tempfile
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

IMG = 28


def _blob_spec():
    """Class definitions: three gaussian blobs per class at fixed ring positions
    (angle of blob k of class c from (c, 3c + 1, 7c + 4) mod 10, radii 8 / 4 /
    10.5 px, sigmas 2.5 / 2.0 / 1.5 px, a small fixed angular offset) -- classes
    share blob positions pairwise, so they overlap instead of being separable by
    any single pixel."""
    g = torch.Generator().manual_seed(1234)
    c = torch.arange(10).float()
    k = torch.stack([c, (3 * c + 1) % 10, (7 * c + 4) % 10], 1)
    ang = 2 * math.pi * k / 10 + 0.3 * torch.rand(10, 3, generator=g)
    rad = torch.tensor([8.0, 4.0, 10.5]).expand(10, 3)
    sig = torch.tensor([2.5, 2.0, 1.5]).expand(10, 3)
    return 13.5 + rad * torch.sin(ang), 13.5 + rad * torch.cos(ang), sig


def _render(cy: torch.Tensor, cx: torch.Tensor, sig: torch.Tensor, amp: torch.Tensor) -> torch.Tensor:
    """Sum of gaussian blobs ([n, k] centres / widths / amplitudes) -> [n, 28, 28]."""
    yy = torch.arange(IMG).float().view(1, 1, IMG, 1)
    xx = torch.arange(IMG).float().view(1, 1, 1, IMG)
    d = (yy - cy[..., None, None]) ** 2 + (xx - cx[..., None, None]) ** 2
    return (amp[..., None, None] * torch.exp(-d / (2 * sig[..., None, None] ** 2))).sum(1)


# version 2 (round 3): a task that is learnable but NOT trivially separable -- per-
# sample blob displacement, a faint second-class distractor on 40 % of the samples,
# background noise, +-1 px jitter and 4 % label noise.  An fp32 784-32-64-10 Adam
# (lr 1e-3) model settles near 0.96 validation accuracy at a validation loss of
# ~0.28 after two epochs (version 1 reached loss 1e-7 / accuracy 1.0, which made every
# convergence check and the Tune sweep's val-loss selection degenerate),
# while 10 batches of 32 at lr 1e-2 still pass the reference's >= 0.5 accuracy gate
# (ray_lightning/tests/utils.py:137-152): 0.57-0.76 over four initialisations.
_CACHE_VERSION = 2
_memo = {}


def _cache_dir() -> str:
    return os.environ.get("RLA_DATA_CACHE") or os.path.join(tempfile.gettempdir(), "rla-synthetic-mnist")


def synthetic_mnist(n: int, seed: int = 0, noise: float = 0.2, jitter: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Return (images uint8 [n, 784], labels int64 [n]).

    Generated once per machine: the arrays are cached as ``.npy`` files (the
    stand-in for the reference's MNIST download into ``data_dir``), so every
    later Tune trial / training worker loads 47 MB in tens of milliseconds
    instead of regenerating it (~3 s, which dominated the start-up of short
    trials).  ``RLA_DATA_CACHE=0`` disables the disk cache."""
    key = (n, seed, float(noise), jitter)
    if key in _memo:
        x, y = _memo[key]
        return x.clone(), y.clone()
    use_disk = os.environ.get("RLA_DATA_CACHE", "") != "0"
    stem = os.path.join(_cache_dir(), f"v{_CACHE_VERSION}_n{n}_s{seed}_z{noise:g}_j{jitter}")
    if use_disk:
        try:
            x = torch.from_numpy(np.load(stem + "_x.npy"))
            y = torch.from_numpy(np.load(stem + "_y.npy"))
            if x.shape == (n, IMG * IMG) and y.shape == (n,):
                _memo[key] = (x, y)
                return x.clone(), y.clone()
        except (OSError, ValueError):
            pass
    x, y = _generate(n, seed, noise, jitter)
    _memo[key] = (x, y)
    if use_disk:
        try:  # atomic publish: concurrent trials may race to write the same arrays
            os.makedirs(_cache_dir(), exist_ok=True)
            for suffix, arr in (("_x.npy", x), ("_y.npy", y)):
                tmp = f"{stem}{suffix}.{os.getpid()}.tmp"
                with open(tmp, "wb") as f:
                    np.save(f, arr.numpy())
                os.replace(tmp, stem + suffix)
        except OSError:
            pass
    return x.clone(), y.clone()


def _generate(n: int, seed: int, noise: float, jitter: int, blob_sd: float = 0.8, distract: float = 0.4,
              distract_p: float = 0.4, label_noise: float = 0.04) -> Tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    cy, cx, sig = _blob_spec()  # class definitions are shared by every split
    labels = torch.randint(0, 10, (n,), generator=g)
    other = (labels + torch.randint(1, 10, (n,), generator=g)) % 10
    damp = distract * (0.4 + 0.6 * torch.rand(n, generator=g)) * (torch.rand(n, generator=g) < distract_p)
    off = torch.randn(n, 3, 2, generator=g) * blob_sd
    amp = (0.6 + 0.4 * torch.rand(n, 3, generator=g)) * torch.tensor([1.0, 1.0, 0.6])
    out = torch.empty(n, IMG, IMG)
    ch = 8192
    for s in range(0, n, ch):
        lab, oth = labels[s:s + ch], other[s:s + ch]
        img = _render(cy[lab] + off[s:s + ch, :, 0], cx[lab] + off[s:s + ch, :, 1], sig[lab], amp[s:s + ch])
        img += damp[s:s + ch, None, None] * _render(cy[oth], cx[oth], sig[oth], torch.ones(len(oth), 3))
        out[s:s + ch] = img
    out /= out.amax(dim=(1, 2), keepdim=True).clamp(min=1e-6)
    # per-sample translation jitter (rolled in blocks of equal shift for speed)
    shifts = torch.randint(-jitter, jitter + 1, (n, 2), generator=g)
    res = torch.empty_like(out)
    for dy in range(-jitter, jitter + 1):
        for dx in range(-jitter, jitter + 1):
            m = (shifts[:, 0] == dy) & (shifts[:, 1] == dx)
            if m.any():
                res[m] = torch.roll(out[m], shifts=(dy, dx), dims=(1, 2))
    res = res * (0.7 + 0.6 * torch.rand(n, 1, 1, generator=g)) + noise * torch.rand(n, IMG, IMG, generator=g)
    flip = torch.rand(n, generator=g) < label_noise
    labels = torch.where(flip, torch.randint(0, 10, (n,), generator=g), labels)
    return (res.clamp(0, 1) * 255).round().to(torch.uint8).reshape(n, IMG * IMG), labels


def _synthetic_mnist_from_spec(n: int, seed: int, train: bool, transform=None) -> "SyntheticMNIST":
    return SyntheticMNIST(n, seed, train, transform=transform)


class SyntheticMNIST(Dataset):
    """Map-style dataset yielding (float [1,28,28] in [0,1], label) like torchvision MNIST+ToTensor.

    Pickles as its generation spec while the arrays are untouched: a model or
    data module that carries it to a worker ships ~100 bytes instead of 47 MB
    (measured: 70 ms per Tune trial, profiles/r3_tune), and the worker loads the
    arrays from its process memo / the disk cache.  Modified arrays (replaced or
    changed in place) pickle by value.  ``transform`` (e.g. ``Normalize``) is applied to the
    float image in ``__getitem__`` and travels with the spec."""

    def __init__(self, n: int = 60000, seed: int = 0, train: bool = True, transform: Optional[Callable] = None):
        self._spec = (n, seed, train)
        self.transform = transform
        self.images, self.targets = synthetic_mnist(n, seed=seed if train else seed + 1)
        self._stamp = self._fingerprint()

    def _fingerprint(self):
        return tuple((id(t), t.data_ptr(), t._version) for t in (self.images, self.targets))

    def __reduce__(self):
        if getattr(self, "_stamp", None) is not None and self._fingerprint() == self._stamp:
            return _synthetic_mnist_from_spec, (*self._spec, self.transform)
        return super().__reduce__()

    def __len__(self) -> int:
        return self.targets.numel()

    def __getitem__(self, i):
        x = self.images[i].view(1, IMG, IMG).float() / 255.0
        if self.transform is not None:
            x = self.transform(x)
        return x, int(self.targets[i])


# ---------------------------------------------------------------------------
# Real MNIST: the IDX files as distributed (and as torchvision lays them out)
# ---------------------------------------------------------------------------
IDX_IMAGES, IDX_LABELS = 0x00000803, 0x00000801  # unsigned byte, 3 / 1 dimensions


def read_idx(path: str) -> torch.Tensor:
    """One MNIST IDX file, plain or ``.gz``: images (magic 0x00000803, ``n x 28 x 28``) as
    uint8 ``[n, 28, 28]``, labels (magic 0x00000801) as uint8 ``[n]``.  Any other magic or
    image size, a truncated file and trailing bytes raise ``ValueError``."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read()
    if len(raw) < 8:
        raise ValueError(f"{path}: truncated IDX header ({len(raw)} bytes)")
    magic, n = struct.unpack(">II", raw[:8])
    if magic == IDX_LABELS:
        head, shape = 8, (n,)
    elif magic == IDX_IMAGES:
        if len(raw) < 16:
            raise ValueError(f"{path}: truncated IDX header ({len(raw)} bytes)")
        rows, cols = struct.unpack(">II", raw[8:16])
        if (rows, cols) != (IMG, IMG):
            raise ValueError(f"{path}: images are {rows} x {cols}, expected {IMG} x {IMG}")
        head, shape = 16, (n, IMG, IMG)
    else:
        raise ValueError(f"{path}: bad IDX magic 0x{magic:08x} (expected 0x{IDX_IMAGES:08x} images or "
                         f"0x{IDX_LABELS:08x} labels)")
    want = head + math.prod(shape)
    if len(raw) != want:
        raise ValueError(f"{path}: {len(raw)} bytes, the header announces {want} "
                         f"({'truncated' if len(raw) < want else 'over-long'} file)")
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8, offset=head).reshape(shape).copy())


def idx_files(root: str, train: bool = True) -> Optional[Tuple[str, str]]:
    """(images, labels) paths of one MNIST split under ``root``: torchvision's
    ``<root>/MNIST/raw/`` first, then ``root`` itself; plain before ``.gz``.  None when
    either file is missing."""
    stem = "train" if train else "t10k"
    for d in (os.path.join(str(root), "MNIST", "raw"), str(root)):
        found = []
        for name in (f"{stem}-images-idx3-ubyte", f"{stem}-labels-idx1-ubyte"):
            hit = next((os.path.join(d, name + ext) for ext in ("", ".gz")
                        if os.path.isfile(os.path.join(d, name + ext))), None)
            if hit is None:
                break
            found.append(hit)
        if len(found) == 2:
            return found[0], found[1]
    return None


class IdxMNIST(Dataset):
    """Real MNIST from its IDX files, in torchvision's layout: ``.data`` uint8 ``[N, 28, 28]``,
    ``.targets`` int64 ``[N]``, ``.transform`` / ``.target_transform``.  ``__getitem__``
    yields ``(float [1, 28, 28] = u8 / 255, int)`` -- ToTensor is built in -- and then applies
    ``transform`` (tensor callables such as ``Normalize``)."""

    def __init__(self, root: str, train: bool = True, transform: Optional[Callable] = None,
                 target_transform: Optional[Callable] = None):
        files = idx_files(root, train)
        if files is None:
            stem = "train" if train else "t10k"
            raise FileNotFoundError(f"no {stem}-images-idx3-ubyte[.gz] / {stem}-labels-idx1-ubyte[.gz] under "
                                    f"{os.path.join(str(root), 'MNIST', 'raw')} or {root}")
        self.root, self.train = str(root), bool(train)
        self.transform, self.target_transform = transform, target_transform
        self.data = read_idx(files[0])
        labels = read_idx(files[1])
        if self.data.dim() != 3 or labels.dim() != 1:
            raise ValueError(f"{files[0]} / {files[1]}: expected an image file and a label file")
        if self.data.size(0) != labels.numel():
            raise ValueError(f"{files[0]} holds {self.data.size(0)} images, {files[1]} {labels.numel()} labels")
        self.targets = labels.to(torch.int64)

    def __len__(self) -> int:
        return self.targets.numel()

    def __getitem__(self, i):
        x = self.data[i].view(1, IMG, IMG).float() / 255.0
        y = int(self.targets[i])
        if self.transform is not None:
            x = self.transform(x)
        if self.target_transform is not None:
            y = self.target_transform(y)
        return x, y


class Normalize:
    """``(x - mean) / std`` per channel of a float tensor ``[C, H, W]`` (torchvision's
    ``transforms.Normalize`` for tensors; torchvision is not a dependency)."""

    def __init__(self, mean: Sequence[float], std: Sequence[float]):
        self.mean = tuple(float(v) for v in (mean if isinstance(mean, (list, tuple)) else (mean,)))
        self.std = tuple(float(v) for v in (std if isinstance(std, (list, tuple)) else (std,)))
        if any(not (s > 0.0 and math.isfinite(s)) for s in self.std):
            raise ValueError(f"Normalize: std must be finite and > 0, got {self.std}")

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        mean = torch.tensor(self.mean, dtype=x.dtype).view(-1, 1, 1)
        std = torch.tensor(self.std, dtype=x.dtype).view(-1, 1, 1)
        return (x - mean) / std

    def __repr__(self) -> str:
        return f"Normalize(mean={self.mean}, std={self.std})"


class Compose:
    """Apply ``transforms`` in order (torchvision's ``transforms.Compose``)."""

    def __init__(self, transforms: Sequence[Callable]):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x

    def __repr__(self) -> str:
        return f"Compose({self.transforms!r})"


class RandomDataset(Dataset):
    """Gaussian vectors (reference tests/utils.py:12-21)."""

    def __init__(self, size: int, length: int, generator: Optional[torch.Generator] = None):
        self.len = length
        self.data = torch.randn(length, size, generator=generator)

    def __getitem__(self, index: int):
        return self.data[index]

    def __len__(self) -> int:
        return self.len
