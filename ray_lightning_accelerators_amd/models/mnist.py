"""MNIST classifier workloads.

``LightningMNISTClassifier`` is the upstream ``ray.tune.examples.mnist_ptl_mini``
model the reference imports (examples/ray_ddp_example.py:13,
tests/test_ddp.py:11): MLP 784 -> layer_1 -> layer_2 -> 10 with ReLU and
log_softmax, NLL loss, Adam(lr), metrics ``ptl/train_loss``,
``ptl/train_accuracy``, ``ptl/val_loss``, ``ptl/val_accuracy``.

On an MI355X the training step of this module runs on the fused HIP engine
(``configure_fused_step`` -> parallel/mlp_engine.py, csrc/mlp_step3.hip): the
trainer hands it the epoch's sampler indices once, the images stay resident in
HBM as uint8, and each step is TWO launches -- a head kernel (forward, loss,
backward of the small layers, next-batch gather) and a 49+ workgroup tail
(dW1, Adam, the next step's layer-1 partial).  At world size > 1 the tail also
exchanges the gradient tiles with the peers over xGMI inside its Adam epilogue
(``RLAConfig.fused_dp``), else head / tail / allreduce / tail.
``Trainer(gradient_clip_val=c)`` stays on the HIP path: head / tail(grad) /
[allreduce] / norm partials / tail(adam), the clip coefficient derived on the
device (``FusedMLPEngine(clip_norm=c)``).
``Trainer(accumulate_grad_batches=K)`` stays on it too (``FusedMLPEngine(accumulate=K)``):
a batch inside its window is head / tail(acc) -- gradients added up on the device, no
Adam -- and the batch that closes it head / tail(grad) / [allreduce] / [norm partials] /
tail(adam) with every micro-batch weighted 1/K; the Trainer dispatches per batch and this
step counts the optimizer steps (``counts_steps``).
The optimizer may be a fused single-group ``torch.optim.Adam``, ``AdamW`` or ``SGD``
(``FusedMLPEngine(optimizer=...)``).  AdamW takes every route Adam takes, the one-launch
step and the in-kernel exchange included.  SGD (momentum, dampening, Nesterov, weight decay)
is applied by the tail kernel: head / tail at world size 1, else -- and under clipping or
accumulation -- head / tail(grad | acc) / [allreduce] / [norm partials] / tail(sgd); never
one launch, never the in-kernel exchange.  ``optimizer.state_dict()`` stays torch's.
The short last batch of a ``drop_last=False`` loader (PyTorch's default) stays on the HIP path
as well: it is the epoch's last step, over its own rows (``begin_epoch(last_rows=r)``: mean
loss and gradient over ``r`` rows, a stats row that counts ``r``), run as head / tail where the
other steps are one launch; ``eval_epoch`` weighs a partial validation batch like a full one,
as the eager loop does.  Only the in-kernel exchange still drops it (one warning).

Datasets the resident path serves (``_u8_source``; ``Subset`` / ``random_split`` chains of
them included): ``.images`` uint8 ``[N, 784]`` with tensor ``.targets`` (``SyntheticMNIST``),
and the torchvision layout -- ``.data`` uint8 ``[N, 28, 28]`` or ``[N, 784]`` with ``.targets``
(``models.data.IdxMNIST`` over real MNIST's IDX files, or torchvision's own ``MNIST``).  Their
``transform`` may be nothing, ``ToTensor`` and one single-channel ``Normalize(mean, std)``
(bare or in a ``Compose``; matched by class name, so torchvision's objects count): the
normalisation becomes one FMA in the kernels' u8 -> bf16 conversion
(``ops.fused_mlp.input_affine``), for training and for ``eval_epoch``.  A dataset other than
ours must convert with ``ToTensor`` first; ``target_transform`` must be None.  Batches the
resident path cannot serve (any other transform, other datasets) use a one-launch fp32-input
kernel; CPU / unsupported shapes use the ordinary autograd path.
"""
from __future__ import annotations

import os
import time
from typing import Any, Dict, Optional

import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, DistributedSampler, SequentialSampler, Subset, random_split

from ..config import get_config
from ..lightning import LightningModule
from ..lightning.metrics import Accuracy
from ..lightning.sampling import deterministic_sampler, sampler_order
from ..ops import fused_mlp
from .data import IdxMNIST, SyntheticMNIST


class LightningMNISTClassifier(LightningModule):
    def __init__(self, config: Dict[str, Any], data_dir: Optional[str] = None):
        super().__init__()
        self.data_dir = data_dir or os.getcwd()
        self.lr = config["lr"]
        layer_1, layer_2 = config["layer_1"], config["layer_2"]
        self.batch_size = config["batch_size"]
        self.layer_1 = torch.nn.Linear(28 * 28, layer_1)
        self.layer_2 = torch.nn.Linear(layer_1, layer_2)
        self.layer_3 = torch.nn.Linear(layer_2, 10)
        self.accuracy = Accuracy()
        self.config = dict(config)

    def forward(self, x):
        b = x.size(0)
        x = x.reshape(b, -1)
        x = torch.relu(self.layer_1(x))
        x = torch.relu(self.layer_2(x))
        return torch.log_softmax(self.layer_3(x), dim=1)

    def configure_optimizers(self):
        return torch.optim.Adam(self.parameters(), lr=self.lr)

    def training_step(self, train_batch, batch_idx):
        x, y = train_batch
        logits = self.forward(x)
        loss = F.nll_loss(logits, y)
        acc = self.accuracy(logits, y)
        self.log("ptl/train_loss", loss)
        self.log("ptl/train_accuracy", acc)
        return loss

    def validation_step(self, val_batch, batch_idx):
        x, y = val_batch
        logits = self.forward(x)
        loss = F.nll_loss(logits, y)
        acc = self.accuracy(logits, y)
        return {"val_loss": loss, "val_accuracy": acc}

    def validation_epoch_end(self, outputs):
        if not outputs:
            return
        avg_loss = torch.stack([x["val_loss"] for x in outputs]).mean()
        avg_acc = torch.stack([x["val_accuracy"] for x in outputs]).mean()
        self.log("ptl/val_loss", avg_loss)
        self.log("ptl/val_accuracy", avg_acc)

    # default synthetic data (the upstream module downloads MNIST; no network here)
    def prepare_data(self):
        if not hasattr(self, "_train_set"):
            full = SyntheticMNIST(60000, seed=0)
            self._train_set, self._val_set = random_split(
                full, [55000, 5000], generator=torch.Generator().manual_seed(0))

    def train_dataloader(self):
        self.prepare_data()
        return DataLoader(self._train_set, batch_size=self.batch_size, drop_last=True)

    def val_dataloader(self):
        self.prepare_data()
        return DataLoader(self._val_set, batch_size=self.batch_size, drop_last=True)

    # ------------------------------------------------------------ fast path
    # the fused step clips by global norm itself (Trainer(gradient_clip_val=...))
    fused_step_clips_gradients = True
    # ... and accumulates gradients over Trainer(accumulate_grad_batches=K) batches itself
    fused_step_accumulates = True

    def configure_fused_step(self, trainer):
        if type(self).training_step is not LightningMNISTClassifier.training_step or \
                type(self).forward is not LightningMNISTClassifier.forward:
            raise RuntimeError("training_step/forward overridden: fused step not applicable")
        return FusedMNISTStep(self, trainer)

    def __getstate__(self):
        d = super().__getstate__()
        return d


def _transform_chain(t) -> list:
    """A transform as a flat list: None -> [], a ``Compose`` (anything with ``.transforms``)
    -> its items, flattened."""
    if t is None:
        return []
    if hasattr(t, "transforms"):
        return [u for item in t.transforms for u in _transform_chain(item)]
    return [t]


def _resident_normalize(transform, to_tensor_built_in: bool):
    """``(True, normalize)`` when the kernels' u8 -> bf16 conversion reproduces ``transform``
    -- ``normalize`` is None (ToTensor alone) or ``(mean, std)`` of one single-channel
    ``Normalize`` -- else ``(False, None)``.  Items are matched by class name.  A dataset
    that hands out raw images (``to_tensor_built_in`` False) must convert with ``ToTensor``
    first."""
    chain = _transform_chain(transform)
    names = [type(t).__name__ for t in chain]
    if not to_tensor_built_in and (not names or names[0] != "ToTensor"):
        return False, None
    rest = [t for t, n in zip(chain, names) if n != "ToTensor"]
    if not rest:
        return True, None
    if len(rest) != 1 or type(rest[0]).__name__ != "Normalize" or not hasattr(rest[0], "mean") \
            or not hasattr(rest[0], "std"):
        return False, None
    try:
        return True, fused_mlp.normalize_pair((rest[0].mean, rest[0].std))
    except (TypeError, ValueError):  # several channels, std <= 0, non-finite
        return False, None


def _u8_source(dataset):
    """Find (images_u8 [N,784], targets, index_map, normalize) behind a dataset (Subset chains
    allowed), or None when the resident path cannot reproduce it.  Accepted: ``.images`` uint8
    ``[N, 784]`` with tensor ``.targets``; ``.data`` uint8 ``[N, 28, 28]`` / ``[N, 784]`` with
    ``.targets`` (tensor or list).  ``normalize``: None, or ``(mean, std)`` of the dataset's
    single-channel ``Normalize`` (``_resident_normalize`` has the transform rules)."""
    idx_map = None
    ds = dataset
    while isinstance(ds, Subset):
        ind = torch.as_tensor(ds.indices, dtype=torch.int64)
        idx_map = ind if idx_map is None else ind[idx_map]
        ds = ds.dataset
    images = getattr(ds, "images", None)
    targets = getattr(ds, "targets", None)
    ours = True  # ToTensor is part of our datasets' __getitem__
    if not isinstance(images, torch.Tensor):
        images = getattr(ds, "data", None)
        ours = isinstance(ds, (IdxMNIST, SyntheticMNIST))
        if isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and images.dim() == 3 \
                and tuple(images.shape[1:]) == (28, 28) and images.is_contiguous():
            images = images.view(images.size(0), 784)
        if isinstance(targets, (list, tuple)):
            try:
                targets = torch.as_tensor(targets, dtype=torch.int64)
            except (TypeError, ValueError):
                return None
    if not (isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and images.dim() == 2
            and images.size(1) == 784 and isinstance(targets, torch.Tensor)):
        return None
    if getattr(ds, "target_transform", None) is not None:
        return None
    ok, normalize = _resident_normalize(getattr(ds, "transform", None), ours)
    if not ok:
        return None
    return images, targets, idx_map, normalize


def _transforms_of(dataset):
    """(transform, target_transform) objects of the dataset behind a Subset chain."""
    ds = dataset
    while isinstance(ds, Subset):
        ds = ds.dataset
    return getattr(ds, "transform", None), getattr(ds, "target_transform", None)


def _same_storage(a: Optional[torch.Tensor], b: Optional[torch.Tensor]) -> bool:
    """The same host images (a ``.data`` dataset is viewed as [N, 784] anew at every look)."""
    return a is not None and b is not None and (
        a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype))


# the sampler-order helpers live in lightning/sampling.py (shared with the
# graph-captured autograd step); the old private names stay importable
_deterministic_sampler = deterministic_sampler
_sampler_order = sampler_order


# rows of the engine's per-step (loss, correct, count, step) ring: two MNIST epochs at
# batch 32, so chunk outputs can be views of it (train_chunk)
ENGINE_STATS_RING = 4096


class FusedMNISTStep:
    """Drives the fused HIP step from the Trainer's loop (replaces autograd + optimizer).

    A step-interval LR scheduler (``{"scheduler": OneCycleLR(...), "interval": "step"}``; not
    ``ReduceLROnPlateau``) keeps chunked dispatch: the engine is built in ring mode
    (``FusedMLPEngine(lr_ring=ENGINE_STATS_RING)``), ``lr_tensor`` is the ring, and the Trainer
    hands each chunk's rates to ``set_lr_schedule`` -- the captured graph reads step ``t``'s
    rate from entry ``(t - 1) & mask``."""

    # the Trainer may chunk under a step-interval scheduler: this step takes a chunk's rates
    schedules_lr = True

    def __init__(self, model: LightningMNISTClassifier, trainer):
        dev = model.device
        if dev.type != "cuda":
            raise RuntimeError("fused step needs a GPU")
        L1, L2 = model.layer_1.out_features, model.layer_2.out_features
        if not fused_mlp.mlp_supported(L1, L2):
            raise RuntimeError(f"no fused kernel for {L1}/{L2}")
        if len(trainer.optimizers) != 1:
            raise RuntimeError("fused step expects one optimizer")
        opt = trainer.optimizers[0]
        if type(opt) not in (torch.optim.Adam, torch.optim.AdamW, torch.optim.SGD) or len(opt.param_groups) != 1 or \
                not getattr(opt, "_rla_fused", False) or opt.param_groups[0].get("amsgrad") or \
                opt.param_groups[0].get("maximize"):
            raise RuntimeError("fused step expects a fused single-group torch.optim.Adam, AdamW or SGD "
                               "(no amsgrad, no maximize)")
        # which update the engine applies: "adam" / "adamw" / "sgd"
        self.opt_kind = {torch.optim.Adam: "adam", torch.optim.AdamW: "adamw", torch.optim.SGD: "sgd"}[type(opt)]
        self.sgd = self.opt_kind == "sgd"
        acc = trainer.accelerator_backend
        arena = acc.arena
        self.np = fused_mlp.mlp_param_count(L1, L2)
        if arena is None or arena.numel < self.np or arena.params[0] is not model.layer_1.weight:
            raise RuntimeError("parameters are not in the expected arena layout")
        self.model, self.trainer, self.opt, self.acc, self.arena = model, trainer, opt, acc, arena
        self.L1, self.L2 = L1, L2
        self.gs = opt._rla_groups[0]
        self.dev = dev
        self.world = trainer.world_size
        clip = float(getattr(trainer, "gradient_clip_val", 0.0) or 0.0)
        if clip < 0.0:
            raise RuntimeError("fused step cannot clip to a negative norm")
        self.clip_norm = clip if clip > 0.0 else None
        # accumulate_grad_batches: micro-batches per optimizer step; this object then counts
        # trainer.global_step itself (one per window, as Trainer._autograd_step does)
        self.accumulate = max(1, int(getattr(trainer, "accumulate_grad_batches", 1) or 1))
        self.counts_steps = self.accumulate > 1
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self.counters[0] = self.gs.step
        self.lr_val = float(opt.param_groups[0]["lr"])
        # a ring of rates indexed by the optimizer step when a step-interval scheduler drives
        # the rate (fixed here: the engine's graphs bake the mask); else the one scalar
        self.lr_ring = ENGINE_STATS_RING if any(
            s.get("interval", "epoch") == "step" and not s.get("reduce_on_plateau")
            for s in getattr(trainer, "lr_schedulers", None) or []) else 0
        self.lr_tensor = torch.full((max(self.lr_ring, 1),), self.lr_val, device=dev)
        self.stats = torch.zeros(64, 4, device=dev)
        self._u8 = None
        self._normalize = None  # the training dataset's Normalize (mean, std), folded into the kernels
        self._order = None
        self._epoch_key = None
        self.eng = None  # v3 pipelined engine (resident-data mode), bound to the arena
        self._allreduce = None
        self._capture_failed = False
        if self.world > 1:
            from ..parallel.comm import make_allreduce

            self._allreduce = make_allreduce()

    def _engine(self, B: int):
        """The v3 engine over the Trainer's arena views (module params stay the masters)."""
        if self.eng is not None and self.eng.B == B:
            return self.eng
        from ..parallel.mlp_engine import FusedMLPEngine

        g = self.opt.param_groups[0]
        bufs = dict(params=self.arena.data[: self.np], grads=self.arena.grad[: self.np])
        if self.sgd:
            bufs["momentum_buffer"] = self.gs.buf[: self.np]
            hyper = dict(optimizer="sgd", momentum=g.get("momentum", 0.0), dampening=g.get("dampening", 0.0),
                         nesterov=bool(g.get("nesterov", False)))
        else:
            bufs.update(exp_avg=self.gs.m[: self.np], exp_avg_sq=self.gs.v[: self.np])
            hyper = dict(optimizer=self.opt_kind, betas=tuple(g["betas"]), eps=g["eps"])
        dp_ctx = None
        rearm = None
        # clipping needs the whole averaged gradient before Adam: the allreduce route;
        # accumulation steps once per window, the in-kernel exchange at every batch; and the
        # exchange's epilogue is Adam / AdamW, so SGD takes the allreduce route too
        if self.world > 1 and get_config().fused_dp and self.clip_norm is None and self.accumulate == 1 \
                and not self.sgd:
            from ..parallel.comm import get_native_comm

            comm = get_native_comm()  # every rank reaches here together (first epoch)
            if comm is not None:
                dp_ctx = comm.dp_context(fused_mlp.mlp3_dp_capacity(self.L1, self.L2))
                rearm = comm.dp_rearm
        eng = FusedMLPEngine(self.L1, self.L2, B, lr=float(g["lr"]),
                             weight_decay=g["weight_decay"], device=self.dev, world_size=self.world,
                             rank=self.trainer.global_rank, allreduce=self._allreduce, buffers=bufs,
                             stats_ring=ENGINE_STATS_RING, dp_context=dp_ctx, dp_rearm=rearm,
                             clip_norm=self.clip_norm, accumulate=self.accumulate, lr_ring=self.lr_ring, **hyper)
        eng.set_step(self.gs.step)
        # LR schedulers update one device scalar (ring mode: this object's ring, which set_lr
        # below fills so that the engine's host picture of it is true)
        eng.lr_tensor = self.lr_tensor
        if self.lr_ring:
            eng.set_lr(self.lr_val)
        eng.attach_dataset(self._u8, self._labels, normalize=self._normalize)
        self.eng = eng
        return eng

    # ---------------------------------------------------------- data plane
    def _source(self, dataset):
        """``_u8_source`` resolved once per dataset object: rebuilding random_split's
        55K-int index list as a tensor every epoch cost ~2 ms of host time while
        the GPU sat idle at the epoch start."""
        cache = self.__dict__.setdefault("_src_cache", {})
        ent = cache.get(id(dataset))
        # the answer holds for the transforms it was derived from: a ``transform`` assigned to
        # the same dataset object later is looked at again (another Normalize, or none the
        # kernels can reproduce)
        tf = _transforms_of(dataset)
        if ent is None or ent[0] is not dataset or ent[2][0] is not tf[0] or ent[2][1] is not tf[1]:
            ent = cache[id(dataset)] = (dataset, _u8_source(dataset), tf)
        return ent[1]

    def make_epoch_batches(self, dl, n_batches: int):
        """Resident-data mode: upload this epoch's sampler order once; yield batch indices."""
        src = self._source(dl.dataset)
        if src is None or dl.batch_size is None:
            return None
        images, targets, idx_map, normalize = src
        if self._u8 is None:
            self._u8_host = images
            self._u8 = images.to(self.dev).contiguous()
            self._labels = targets.to(self.dev, torch.int64).contiguous()
            self._normalize = normalize
        elif normalize != self._normalize:
            # the loader's transform changed: the engine re-primes and re-captures under the new map
            self._normalize = normalize
            if self.eng is not None:
                self.eng.attach_dataset(self._u8, self._labels, normalize=normalize)
        pre = getattr(self, "_prefetched", None)
        self._prefetched = None
        ep = getattr(dl.sampler, "epoch", None)
        if pre is not None and pre[0] is dl.sampler and pre[1] == ep:
            order = pre[2]  # computed (and bounds-checked) while the previous epoch ran
        else:
            order = self._epoch_order(dl.sampler, idx_map)
        B = dl.batch_size
        full, rem = divmod(order.numel(), B)
        nb = min(n_batches, full if dl.drop_last else -(-order.numel() // B))
        # the short last batch of a drop_last=False loader is the epoch's last step: its
        # ``rem`` rows train on the HIP path (FusedMLPEngine.begin_epoch(last_rows=...)); a
        # limit_train_batches that stops before it leaves only full batches
        last_rows = rem if (nb > full and rem) else None
        if nb <= 0:
            return None
        eng = self._engine(B)
        if last_rows is not None and eng.dp_ctx is not None:
            # the in-kernel exchange has no short batch: the engine drops it (and says so once)
            eng.begin_epoch(order, nb, checked=True, last_rows=last_rows)
            nb = eng.n_batches
        else:
            eng.begin_epoch(order[: (nb - 1) * B + (last_rows or B)], nb, checked=True, last_rows=last_rows)
        self._B = B
        self._nb = nb
        return [("__rla_resident__", i) for i in range(nb)]

    def _epoch_order(self, sampler, idx_map):
        order = _sampler_order(sampler)
        if idx_map is not None:
            order = idx_map[order]
        assert int(order.max()) < self._u8.size(0) and int(order.min()) >= 0  # the kernels trust indices
        return order

    def prefetch_next_epoch(self, dl, epoch: int) -> None:
        """Compute epoch ``epoch``'s sample order now -- the Trainer calls this right
        after dispatching an epoch's last steps, while the host would otherwise just
        wait for the GPU -- so the next epoch's first launch is not delayed by it
        (~1 ms of host work for 55K indices).  Only for samplers whose order is a
        function of the epoch number (DistributedSampler, SequentialSampler)."""
        import copy

        sampler = dl.sampler
        if not (isinstance(sampler, DistributedSampler) or isinstance(sampler, SequentialSampler)):
            return
        src = self._source(dl.dataset)
        if src is None or self._u8 is None:
            return
        s2 = copy.copy(sampler)
        if isinstance(s2, DistributedSampler):
            s2.epoch = epoch
        self._prefetched = (sampler, epoch if isinstance(sampler, DistributedSampler) else
                            getattr(sampler, "epoch", None), self._epoch_order(s2, src[2]))

    def _sync_lr(self) -> None:
        lr = float(self.opt.param_groups[0]["lr"])
        if lr != self.lr_val:
            self.lr_val = lr
            if self.lr_ring and self.eng is not None:
                self.eng.set_lr(lr)  # the whole ring; any schedule is forgotten
            else:
                self.lr_tensor.fill_(lr)

    def on_lr_change(self) -> None:
        self._sync_lr()

    def set_lr_schedule(self, rates) -> None:
        """The rates of the next ``len(rates)`` optimizer steps, from the Trainer ahead of
        ``train_chunk``: it has already stepped the schedulers past them, so the group's rate
        is now the one of the step after the chunk -- which is what any step past the
        schedule runs with."""
        self.lr_val = float(self.opt.param_groups[0]["lr"])
        self._sync_engine()
        self.eng.set_lr_schedule(rates)

    def _lr_one(self) -> torch.Tensor:
        """The one-element rate tensor of a loader-fed batch (those kernels keep their
        single-scalar contract): ring mode fills the ring with the current rate first."""
        if not self.lr_ring:
            return self.lr_tensor
        if self.eng is None or self.eng._ring_uniform != self.lr_val:
            if self.eng is not None:
                self.eng.set_lr(self.lr_val)
            else:
                self.lr_tensor.fill_(self.lr_val)
        return self.lr_tensor[:1]

    def _sync_engine(self) -> None:
        """The group's hyperparameters, refreshed per dispatch (a user or a scheduler may
        have edited ``param_groups``)."""
        eng, g = self.eng, self.opt.param_groups[0]
        eng.lr, eng.wd = self.lr_val, g["weight_decay"]
        if self.sgd:
            eng.momentum, eng.dampening = float(g.get("momentum", 0.0)), float(g.get("dampening", 0.0))
            eng.nesterov = bool(g.get("nesterov", False))
            # torch's SGD state has no step: after a resume the group restarts at 1, and
            # loader-fed batches step outside the engine.  Its device counter (the kernels'
            # "first step" rule, the stats-ring slot) follows gs.step.
            if eng.optimizer_steps != self.gs.step:
                eng.set_step(self.gs.step)
        else:
            eng.betas, eng.eps = tuple(g["betas"]), g["eps"]

    def _apply_optimizer(self, p, gr, scale: float) -> None:
        """The optimizer over the arena after a loader-fed batch left its gradient."""
        from ..ops.optim import fused_adam_, fused_sgd_

        g = self.opt.param_groups[0]
        if self.sgd:
            mom = float(g.get("momentum", 0.0))
            fused_sgd_(p, gr, self.gs.buf[: self.np] if mom != 0.0 else None, lr=self.lr_val, momentum=mom,
                       dampening=g.get("dampening", 0.0), weight_decay=g["weight_decay"],
                       nesterov=bool(g.get("nesterov", False)), grad_scale=scale, step=self.counters[0:1],
                       lr_tensor=self._lr_one())
        else:
            fused_adam_(p, gr, self.gs.m[: self.np], self.gs.v[: self.np], lr=self.lr_val, betas=tuple(g["betas"]),
                        eps=g["eps"], weight_decay=g["weight_decay"], grad_scale=scale,
                        adamw=self.opt_kind == "adamw", step=self.counters[0:1], lr_tensor=self._lr_one())

    def _train_micro_batch(self, batch, batch_idx: int):
        """``train_batch`` under ``accumulate_grad_batches=K``: one micro-batch.  Batch i of
        the epoch closes its window when (i + 1) % K == 0 or it is the epoch's last; only
        then do Adam, ``trainer.global_step``, the optimizer's step counts and the
        step-interval LR schedulers move.  Returns the batch's own stats row."""
        self._sync_lr()
        K = self.accumulate
        g = self.opt.param_groups[0]
        if isinstance(batch, tuple) and len(batch) == 2 and batch[0] == "__rla_resident__":
            eng = self.eng
            self._sync_engine()
            before = eng.optimizer_steps
            eng.step()  # one micro-batch (no graph is captured on this per-batch path)
            closing = eng.optimizer_steps != before
            row = eng.stats[(eng.global_step - 1) % eng.stats.size(0)]  # one ring row per micro-batch
        else:
            from ..ops.optim import clip_partials

            p, gr = self.arena.data[: self.np], self.arena.grad[: self.np]
            n = int(getattr(self.trainer, "num_training_batches", 0) or 0)
            micro = batch_idx % K
            closing = (batch_idx + 1) % K == 0 or (n > 0 and batch_idx + 1 >= n)
            self.counters[0] = self.gs.step
            x, y = batch
            x = x.to(self.dev, non_blocking=True).reshape(x.size(0), -1).float().contiguous()
            y = y.to(self.dev, non_blocking=True).long().contiguous()
            stats = torch.zeros(1, 4, device=self.dev)  # this batch's own row
            fused_mlp.mlp_train_step(p, gr, B=x.size(0), labels=y, x_f32=x, L1=self.L1, L2=self.L2,
                                     stats=stats, accumulate_grad=micro > 0, apply_adam=False,
                                     advance_step=closing, lr=self.lr_val, weight_decay=g["weight_decay"],
                                     lr_tensor=self._lr_one(), counters=self.counters)
            if closing:
                scale = 1.0 / (self.world * K)
                if self._allreduce is not None and self.acc.sync is not None:
                    self._allreduce(gr)
                if self.clip_norm is not None:
                    norm = clip_partials(gr, 32).sum().sqrt() * scale
                    gr.mul_(torch.clamp(self.clip_norm / (norm + 1e-6), max=1.0))
                self._apply_optimizer(p, gr, scale)
                if self.eng is not None:
                    self.eng.refresh_shadow()  # params moved outside the engine
            row = stats[0]
        if closing:
            self.gs.step += 1
            for q in g["params"]:
                st = self.opt.state.get(q)
                if st is not None and "step" in st:
                    st["step"].fill_(float(self.gs.step))
            self.trainer.global_step += 1
            self.trainer._update_lr_schedulers("step")
        loss = row[0]
        self.model.log("ptl/train_loss", loss)
        self.model.log("ptl/train_accuracy", row[1] / row[2].clamp(min=1))
        self.trainer.callback_metrics["loss"] = loss
        return {"loss": loss}

    def train_batch(self, batch, batch_idx: int):
        if self.accumulate > 1:
            return self._train_micro_batch(batch, batch_idx)
        self._sync_lr()
        g = self.opt.param_groups[0]
        p = self.arena.data[: self.np]
        gr = self.arena.grad[: self.np]
        # the loader-fed kernel applies Adam / AdamW itself; SGD follows it as its own launch
        fused = self.world == 1 and self.clip_norm is None and not self.sgd
        kw = dict(L1=self.L1, L2=self.L2, stats=self.stats, apply_adam=fused, advance_step=True, lr=self.lr_val,
                  weight_decay=g["weight_decay"], lr_tensor=self._lr_one(), counters=self.counters)
        if not self.sgd:
            kw.update(exp_avg=self.gs.m[: self.np], exp_avg_sq=self.gs.v[: self.np], betas=tuple(g["betas"]),
                      eps=g["eps"], adamw=self.opt_kind == "adamw")
        stats = self.stats
        if isinstance(batch, tuple) and len(batch) == 2 and batch[0] == "__rla_resident__":
            # v3 pipelined step (head + tail [+ allreduce + tail-adam]); Adam is the engine's
            eng = self.eng
            self._sync_engine()
            eng.step()
            stats = eng.stats
            fused = True  # optimizer already applied
        else:
            # the optimizer step may have moved outside this object (resume, engine steps)
            self.counters[0] = self.gs.step
            x, y = batch
            x = x.to(self.dev, non_blocking=True).reshape(x.size(0), -1).float().contiguous()
            y = y.to(self.dev, non_blocking=True).long().contiguous()
            fused_mlp.mlp_train_step(p, gr, B=x.size(0), labels=y, x_f32=x, **kw)
        if not fused:
            if self._allreduce is not None and self.acc.sync is not None:
                self._allreduce(self.arena.grad[: self.np])
            from ..ops.optim import clip_partials

            if self.clip_norm is not None:
                # loader-fed batches are rare and slow anyway: the coefficient with torch
                # ops on the device (no host sync), the gradient scaled in place
                norm = clip_partials(gr, 32).sum().sqrt() * (1.0 / self.world)
                coef = torch.clamp(self.clip_norm / (norm + 1e-6), max=1.0)
                gr.mul_(coef)

            self._apply_optimizer(p, gr, 1.0 / self.world)
        if self.eng is not None and stats is self.stats:
            self.eng.refresh_shadow()  # params moved outside the engine
        self.gs.step += 1
        for q in g["params"]:
            st = self.opt.state.get(q)
            if st is not None and "step" in st:
                st["step"].fill_(float(self.gs.step))
        slot = (self.gs.step - 1) % stats.size(0)
        loss = stats[slot, 0]
        # metrics (device tensors; no host sync here)
        self.model.log("ptl/train_loss", loss)
        self.model.log("ptl/train_accuracy", stats[slot, 1] / stats[slot, 2].clamp(min=1))
        self.trainer.callback_metrics["loss"] = loss
        return {"loss": loss}

    @property
    def max_chunk(self) -> int:
        """Most steps one :meth:`train_chunk` can report per-step losses for: half the
        engine's stats ring (a chunk's rows stay valid through the next chunk)."""
        return ENGINE_STATS_RING // 2

    # the Trainer may run a chunk across several log points: log_points() gives each
    # one's metrics (views of the stats ring) -- no dispatch cut every 50 steps
    chunk_spans_log_points = True

    def log_points(self, rows: torch.Tensor, first: int, every: int):
        """``(global step, metrics)`` for every multiple of ``every`` among the steps
        ``first + 1 .. first + len(rows)`` whose (loss, correct, count) rows are
        ``rows`` -- ring views, plus ONE division kernel for all their accuracies."""
        steps = [first + 1 + i for i in range(rows.size(0)) if (first + 1 + i) % every == 0]
        if not steps:
            return []
        acc = rows[:, 1] / rows[:, 2]
        out = []
        for st in steps:
            i = st - first - 1
            loss, a = rows[i, 0], acc[i]
            loss._rla_fresh = a._rla_fresh = True
            out.append((st, {"ptl/train_loss": loss, "ptl/train_accuracy": a}))
        return out

    def _graph_steps(self) -> int:
        """Steps per captured graph: the Trainer cuts dispatches at multiples of
        ``log_every_n_steps``, so the largest divisor of it up to the stats ring
        (64; 50 for the default 50) makes a typical chunk ONE replay (a graph
        launch costs the host tens of us; the engine's 1/2/4/... remainder
        graphs cover the chunks cut short by validation or the epoch end)."""
        if getattr(self.trainer, "_chunks_span_logs", False):
            # dispatch chunks run across log points: bigger graphs, fewer replays --
            # the largest power of two within the dispatch chunk and the epoch (<= 256)
            tr = self.trainer
            spd = tr.steps_per_dispatch if tr.steps_per_dispatch is not None else get_config().steps_per_dispatch
            cap = min(256, int(spd), int(getattr(tr, "num_training_batches", 256) or 256))
            g = 1
            while g * 2 <= cap:
                g *= 2
            return max(g, 1)
        every = max(1, int(getattr(self.trainer, "log_every_n_steps", 50) or 50))
        for g in range(min(64, every), 3, -1):
            if every % g == 0:
                return g
        return 8

    def train_chunk(self, n_steps: int, graph_steps: Optional[int] = None):
        """``n_steps`` consecutive resident-mode steps in one dispatch (hipGraph
        replays of ``graph_steps`` steps each, captured once per epoch); the
        Trainer uses it when nothing observes individual batches.  Returns the
        per-step ``{"loss"}`` outputs (views of one device copy, no host sync)."""
        if graph_steps is None:
            graph_steps = self._graph_steps()
        eng = self.eng
        self._sync_lr()
        g = self.opt.param_groups[0]
        self._sync_engine()
        done = 0
        if graph_steps > 1 and eng._graph is None and not self._capture_failed and get_config().use_hip_graph \
                and n_steps >= graph_steps and eng.steps_to_epoch_end() >= graph_steps:
            # one real (warm-up) step, then the recording; identical on every rank
            self._capture_failed = not eng.capture(graph_steps)
            done = 1
        t_run = time.perf_counter()
        eng.run(n_steps - done)
        self._last_run_us = (time.perf_counter() - t_run) * 1e6  # diagnostic (RLA_CHUNK_TIMING)
        first = self.gs.step
        self.gs.step += n_steps
        for q in g["params"]:
            st = self.opt.state.get(q)
            if st is not None and "step" in st:
                st["step"].fill_(float(self.gs.step))
        ring = eng.stats.size(0)
        k = min(n_steps, ring)
        # Rows of the chunk's last k steps, in step order: step first + 1 + i sits in
        # ring slot (first + i) % ring, which the host knows.  When the ring holds two
        # epochs (MNIST: 1,718 steps in 4,096 rows) the rows are handed out as VIEWS of
        # it: an epoch's outputs stay intact until the end of the next epoch, past its
        # training_epoch_end and the blocking log flush -- no copy kernel per chunk
        # (each small kernel between two graph replays left the GPU idle for a few us,
        # ~1 ms per epoch in all).  Otherwise: one or two device-to-device copies into a
        # fresh tensor.  Never an index kernel: a chunk-sized gather picked a different
        # ROCm index kernel for small chunks, whose code object loaded mid-epoch and
        # stalled it by ~60 ms (profiles/r2_c05); no host sync either.
        s0 = (first + n_steps - k) % ring
        n1 = min(k, ring - s0)
        if n1 == k and 2 * max(int(getattr(self.trainer, "num_training_batches", ring)), 1) <= ring:
            rows = eng.stats[s0:s0 + k]
        else:
            rows = torch.empty(k, 4, device=self.dev)
            rows[:n1].copy_(eng.stats[s0:s0 + n1])
            if n1 < k:
                rows[n1:].copy_(eng.stats[: k - n1])
        last = rows[-1]
        loss = last[0]
        acc = last[1] / last[2]  # every step counts > 0 rows (B, or a short last batch's)
        # neither tensor is written again before the deferred log flush: no snapshot copy
        loss._rla_fresh = acc._rla_fresh = True
        self.model.log("ptl/train_loss", loss)
        self.model.log("ptl/train_accuracy", acc)
        self.trainer.callback_metrics["loss"] = loss
        self._last_rows, self._last_first = rows, first + n_steps - k
        return [{"loss": v} for v in rows[:, 0].unbind(0)]

    # ---------------------------------------------------------- validation
    def eval_compatible(self, model) -> bool:
        """The stock validation_step / _end / _epoch_end: per-batch mean NLL and
        accuracy, averaged over the (equal-size) batches."""
        t = type(model)
        return (t.validation_step is LightningMNISTClassifier.validation_step
                and t.validation_epoch_end is LightningMNISTClassifier.validation_epoch_end
                and t.validation_step_end is LightningModule.validation_step_end
                and t.forward is LightningMNISTClassifier.forward)

    def _resident(self, images: torch.Tensor, targets: torch.Tensor):
        if self._u8 is not None and _same_storage(images, getattr(self, "_u8_host", None)):
            return self._u8, self._labels  # validation split of the training dataset
        cache = self.__dict__.setdefault("_eval_sets", {})
        key = id(images)
        if key not in cache:
            cache[key] = (images, images.to(self.dev).contiguous(), targets.to(self.dev, torch.int64).contiguous())
        return cache[key][1], cache[key][2]

    def eval_epoch(self, dl, n_batches: int):
        """One validation pass over the resident dataset in ONE launch (a workgroup
        per 32 samples, per-chunk partial sums reduced deterministically).
        Returns ``{"val_loss", "val_accuracy"}`` device scalars -- the mean over the
        ``n_batches`` batches of their per-batch means, which is what the eager
        validation_step + validation_epoch_end produce -- or None when the loader
        cannot be served from the resident data (the Trainer then runs the
        per-batch loop).  The short last batch of a ``drop_last=False`` loader (``r`` rows)
        weighs like a full one there, ``(S_full / B + S_last / r) / n_batches``: a second
        launch over its ``r`` samples gives ``S_last``."""
        src = self._source(dl.dataset)
        if src is None or dl.batch_size is None or n_batches <= 0:
            return None
        images, targets, idx_map, normalize = src
        x_scale, x_shift = fused_mlp.input_affine(normalize)  # the validation dataset's own transform
        B = int(dl.batch_size)
        key = (id(dl), id(images), int(n_batches))
        cached = self.__dict__.setdefault("_eval_orders", {}).get(key)
        # the entry holds `dl` and `images` themselves: an id reused after garbage
        # collection must not return another loader's order
        if cached is not None and (cached[2] is not dl or cached[3] is not images):
            cached = None
        if cached is None:
            order = _sampler_order(dl.sampler)
            if idx_map is not None:
                order = idx_map[order]
            full, rem = divmod(order.numel(), B)
            total = full if dl.drop_last else full + (1 if rem else 0)
            nb = min(int(n_batches), total)
            if nb <= 0:
                return None
            last = rem if nb > full else 0  # rows of a partial last batch inside the limit
            nb -= 1 if last else 0  # nb: the full batches
            order = order[: nb * B + last]
            assert int(order.max()) < images.size(0) and int(order.min()) >= 0  # the kernel trusts indices
            cached = (order.to(self.dev), nb, dl, images, last)
            # reuse only an order that cannot change between epochs (a deterministic
            # sampler): a shuffled sampler is re-drawn every call, as eager iteration
            # does (same subset under limit_val_batches, same global-RNG draws)
            if _deterministic_sampler(dl.sampler):
                self._eval_orders[key] = cached
        order_dev, nb, last = cached[0], cached[1], cached[4]
        u8, labels = self._resident(images, targets)
        n = nb * B
        kw = dict(L1=self.L1, L2=self.L2, labels=labels, x_u8=u8, x_scale=x_scale, x_shift=x_shift)
        tot = None
        if n:
            part = torch.empty((n + 31) // 32, 2, device=self.dev)
            fused_mlp.mlp_eval(self.arena.data[: self.np], B=n, out=part, index=order_dev[:n], **kw)
            tot = part.sum(0) / n
            if not last:
                return {"val_loss": tot[0], "val_accuracy": tot[1]}
        # the partial batch's own per-batch mean, then the mean over the nb + 1 batches
        part = torch.empty((last + 31) // 32, 2, device=self.dev)
        fused_mlp.mlp_eval(self.arena.data[: self.np], B=last, out=part, index=order_dev[n:], **kw)
        short = part.sum(0) / last
        tot = short if tot is None else (tot * nb + short) / (nb + 1)
        return {"val_loss": tot[0], "val_accuracy": tot[1]}

    def check(self, blocking: bool = True) -> None:
        """Raise if the engine's in-launch hand-off ever timed out, and report saturated /
        non-finite layer-1 partial sums as ``RLAConfig.mlp_saturation`` says (epoch end:
        ``blocking=False`` checks the previous epoch's asynchronously copied words)."""
        if self.eng is not None:
            self.eng.check(blocking)

    def health(self, blocking: bool = True) -> Dict[str, Any]:
        """``FusedMLPEngine.health()`` of the engine behind this step."""
        if self.eng is not None:
            return self.eng.health(blocking)
        return {"saturated": 0, "nonfinite": 0, "last_step": 0, "timed_out": False}

    def sync_optimizer_state(self) -> None:
        """Owner protocol: consolidate the Adam state before it is read (collective)."""
        if self.eng is not None:
            self.eng.sync_optimizer_state()

    # --------------------------------------------------------------- state
    def sync_params_to_module(self) -> None:
        pass  # module parameters ARE arena views

    def load_params_from_module(self) -> None:
        self.arena.rebind_all()
        self.counters[0] = self.gs.step
        if self.eng is not None:
            self.eng.set_step(self.gs.step)
            self.eng.refresh_shadow()


# The reference's examples subclass the upstream module as ``MNISTClassifier``
# with an MNIST-downloading prepare_data (examples/ray_ddp_example.py:18-58);
# ours already prepares the 55,000/5,000 split on the driver (synthetic data).
MNISTClassifier = LightningMNISTClassifier
