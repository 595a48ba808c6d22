"""Lightning-compatible ``Trainer``.

Re-implements the PyTorch Lightning 1.1 training-loop contract that the
reference inherits: ``fit`` returns 1, the sanity
validation run (``running_sanity_check``), train/val/test loops with
``limit_*_batches``, ``DistributedSampler`` injection when the accelerator
requires it (reference ray_ddp.py:280-295), hook ordering (validation before
``on_epoch_end``), ``ModelCheckpoint``/``EarlyStopping``, LR schedulers,
gradient accumulation/clipping, ``self.log`` metrics in ``callback_metrics``,
and the Lightning checkpoint format.

Distribution is delegated to the accelerator object: the driver calls
``accelerator.setup(model) -> train() -> teardown()``; every worker then runs
``Trainer._run(model)`` (via the accelerator's ``ddp_train``-style entry).
"""
from __future__ import annotations

import gc
import math
import os
import sys
import time
from collections import defaultdict
from typing import Any, Dict, List, Optional, Sequence, Union

import torch
from torch.utils.data import DataLoader, DistributedSampler, RandomSampler, SequentialSampler

from .callbacks import Callback, EarlyStopping, ModelCheckpoint
from .core import LightningDataModule, LightningModule, _normalize_optimizers
from .loggers import CSVLogger, LightningLoggerBase
from .utilities import (CheckpointWriter, atomic_save, load_checkpoint, log, move_to_device,  # noqa: F401
                        process_checkpoint_writer, rank_zero_warn)
from ..config import get_config
from ..utils.faults import maybe_inject as maybe_inject_fault
from ..utils.profiling import resolve_profiler
from ..utils.timeline import mark

PL_COMPAT_VERSION = "1.1.7"


class _CheckpointConnector:
    def __init__(self, trainer: "Trainer"):
        self.trainer = trainer

    def dump_checkpoint(self, weights_only: bool = False, staged: bool = False) -> dict:
        """The Lightning checkpoint dict (PL 1.1 layout; callback keys are class names).
        ``staged``: device state goes into device-side snapshots (``_Staged``; no
        host sync) that :func:`_resolve_staged` turns into host tensors later."""
        t = self.trainer
        model = t.get_model()
        ckpt: Dict[str, Any] = {
            "epoch": t.current_epoch + 1,
            "global_step": t.global_step + 1,
            "pytorch-lightning_version": PL_COMPAT_VERSION,
        }
        if not weights_only:
            cb_states = {}
            for cb in t.callbacks:
                st = cb.on_save_checkpoint(t, model, ckpt)
                if st is not None:
                    cb_states[cb.state_key] = st
            ckpt["callbacks"] = cb_states
            ckpt["optimizer_states"] = [t._optimizer_state_dict(o, staged) for o in t.optimizers]
            ckpt["lr_schedulers"] = [s["scheduler"].state_dict() for s in t.lr_schedulers]
        ckpt["state_dict"] = t._model_state_dict(model, staged)
        hp = dict(model.hparams) if getattr(model, "hparams", None) else {}
        if hp:
            ckpt[LightningModule.CHECKPOINT_HYPER_PARAMS_NAME] = "hparams"
            ckpt[LightningModule.CHECKPOINT_HYPER_PARAMS_KEY] = hp
        model.on_save_checkpoint(ckpt)
        return ckpt

    def restore(self, checkpoint_path: str, on_gpu: bool = False) -> None:
        t = self.trainer
        ckpt = load_checkpoint(checkpoint_path, map_location="cpu")
        model = t.get_model()
        model.on_load_checkpoint(ckpt)
        model.load_state_dict(ckpt["state_dict"])
        for cb in t.callbacks:
            st = ckpt.get("callbacks", {}).get(cb.state_key)
            if st is not None:
                cb.on_load_checkpoint(st)
        for opt, st in zip(t.optimizers, ckpt.get("optimizer_states", [])):
            opt.load_state_dict(st)
        for s, st in zip(t.lr_schedulers, ckpt.get("lr_schedulers", [])):
            s["scheduler"].load_state_dict(st)
        if t._fused is not None:
            # after the optimizer state: the fused step's device step counter (Adam
            # bias correction) is re-read from the restored optimizer step
            t._fused.load_params_from_module()
        t.current_epoch = ckpt.get("epoch", 0)
        t.global_step = ckpt.get("global_step", 0)


class Trainer:
    def __init__(
        self,
        default_root_dir: Optional[str] = None,
        gpus: Optional[Union[int, List[int]]] = None,
        max_epochs: Optional[int] = None,
        min_epochs: Optional[int] = None,
        max_steps: Optional[int] = None,
        limit_train_batches: Union[int, float] = 1.0,
        limit_val_batches: Union[int, float] = 1.0,
        limit_test_batches: Union[int, float] = 1.0,
        val_check_interval: Union[int, float] = 1.0,
        check_val_every_n_epoch: int = 1,
        num_sanity_val_steps: int = 2,
        progress_bar_refresh_rate: int = 1,
        checkpoint_callback: bool = True,
        callbacks: Optional[List[Callback]] = None,
        accelerator: Any = None,
        precision: Union[int, str] = 32,
        gradient_clip_val: float = 0.0,
        accumulate_grad_batches: int = 1,
        logger: Union[bool, LightningLoggerBase] = True,
        log_every_n_steps: int = 50,
        resume_from_checkpoint: Optional[str] = None,
        deterministic: bool = False,
        benchmark: bool = False,
        weights_summary: Optional[str] = "top",
        fast_dev_run: Union[bool, int] = False,
        num_nodes: int = 1,
        sync_batchnorm: bool = False,
        replace_sampler_ddp: bool = True,
        reload_dataloaders_every_epoch: bool = False,
        fused_step: Optional[bool] = None,
        steps_per_dispatch: Optional[int] = None,
        profiler=None,
        **kwargs,
    ):
        for k in kwargs:
            rank_zero_warn(f"Trainer argument {k!r} is accepted for compatibility and ignored")
        self.default_root_dir = default_root_dir or os.getcwd()
        if isinstance(gpus, (list, tuple)):
            gpus = len(gpus)
        elif isinstance(gpus, str):
            gpus = len([g for g in gpus.split(",") if g.strip()])
        self.gpus = int(gpus or 0)
        self.fast_dev_run = int(fast_dev_run) if fast_dev_run else 0
        if self.fast_dev_run:
            max_epochs = 1
            limit_train_batches = limit_val_batches = limit_test_batches = self.fast_dev_run
            num_sanity_val_steps = 0
        self.max_epochs = 1000 if max_epochs is None else int(max_epochs)
        self.min_epochs = 1 if min_epochs is None else int(min_epochs)
        self.max_steps = max_steps
        self.limit_train_batches = limit_train_batches
        self.limit_val_batches = limit_val_batches
        self.limit_test_batches = limit_test_batches
        self.val_check_interval = val_check_interval
        self.check_val_every_n_epoch = check_val_every_n_epoch
        self.num_sanity_val_steps = num_sanity_val_steps
        self.progress_bar_refresh_rate = progress_bar_refresh_rate
        self.precision = precision
        self.gradient_clip_val = gradient_clip_val
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self.log_every_n_steps = log_every_n_steps
        self.resume_from_checkpoint = resume_from_checkpoint
        self.deterministic = deterministic
        self.benchmark = bool(benchmark)  # torch.backends.cudnn.benchmark on the workers (MIOpen find)
        self.num_nodes = num_nodes
        self.sync_batchnorm = sync_batchnorm
        self.replace_sampler_ddp = replace_sampler_ddp
        self.reload_dataloaders_every_epoch = reload_dataloaders_every_epoch
        self.weights_summary = weights_summary
        self.fused_step = fused_step
        # set at the end of a fit that ran the fused MNIST step: FusedMLPEngine.health()
        self.fused_step_health: Optional[Dict[str, Any]] = None
        self.steps_per_dispatch = steps_per_dispatch  # None: RLAConfig.steps_per_dispatch
        self._chunks_span_logs = False
        self.profiler = resolve_profiler(profiler)
        self.profiler_summary = ""
        if deterministic:
            torch.use_deterministic_algorithms(True, warn_only=True)
        # callbacks
        self.callbacks: List[Callback] = list(callbacks or [])
        self._checkpoint_enabled = bool(checkpoint_callback)
        if isinstance(checkpoint_callback, ModelCheckpoint):
            self.callbacks.append(checkpoint_callback)
        elif checkpoint_callback and not any(isinstance(c, ModelCheckpoint) for c in self.callbacks):
            self.callbacks.append(ModelCheckpoint())
        # logger
        if logger is True:
            self.logger: Optional[LightningLoggerBase] = CSVLogger(self.default_root_dir)
        elif logger is False or logger is None:
            self.logger = None
        else:
            self.logger = logger
        self.accelerator = accelerator
        self.accelerator_backend = None
        self.distributed_backend = None
        # state
        self.global_rank = 0
        self.local_rank = 0
        self.node_rank = 0
        self.world_size = 1
        self.root_gpu: Optional[int] = None
        self.use_ddp = False
        self.use_horovod = False
        self.use_dp = False
        self.use_single_gpu = False
        self.model: Optional[LightningModule] = None
        self.datamodule: Optional[LightningDataModule] = None
        self.train_dataloader: Optional[DataLoader] = None
        self.val_dataloaders: Optional[List[DataLoader]] = None
        self.test_dataloaders: Optional[List[DataLoader]] = None
        self.num_training_batches = 0
        self.num_val_batches: List[int] = []
        self.num_test_batches: List[int] = []
        self.callback_metrics: Dict[str, Any] = {}
        self.logged_metrics: Dict[str, Any] = {}
        self.progress_bar_metrics: Dict[str, Any] = {}
        self.running_sanity_check = False
        self.testing = False
        self.training = False
        self.current_epoch = 0
        self.global_step = 0
        self.should_stop = False
        self.optimizers: List[torch.optim.Optimizer] = []
        self.lr_schedulers: List[dict] = []
        self.optimizer_frequencies: List[int] = []
        self.checkpoint_connector = _CheckpointConnector(self)
        self.interrupted = False
        self._has_val_loop = False
        self._fused = None
        self._graph_step_reason: Optional[str] = None
        self._log_sink: Optional[list] = None  # GraphedTrainStep records self.log calls here
        self._pending_log = None
        self._staged_logs: List[dict] = []  # deferred log rows whose host copy is in flight
        self._log_dir: Optional[str] = None
        self._train_dl_src = self._val_dl_src = self._test_dl_src = None
        self._results: Dict[str, Dict[str, list]] = {}
        self._current_fx: Optional[str] = None
        self.test_results = None

    # ------------------------------------------------------------ properties
    @property
    def on_gpu(self) -> bool:
        acc = self.accelerator
        if acc is not None and hasattr(acc, "use_gpu"):
            return bool(acc.use_gpu) or self.gpus > 0 and bool(getattr(acc, "use_gpu", True))
        return self.gpus > 0

    @property
    def is_global_zero(self) -> bool:
        return self.global_rank == 0

    @property
    def checkpoint_callback(self) -> Optional[ModelCheckpoint]:
        for c in self.callbacks:
            if isinstance(c, ModelCheckpoint):
                return c
        return None

    @property
    def checkpoint_callbacks(self) -> List[ModelCheckpoint]:
        return [c for c in self.callbacks if isinstance(c, ModelCheckpoint)]

    @property
    def early_stopping_callback(self) -> Optional[EarlyStopping]:
        for c in self.callbacks:
            if isinstance(c, EarlyStopping):
                return c
        return None

    @property
    def log_dir(self) -> Optional[str]:
        if self._log_dir is not None:
            return self._log_dir
        if self.logger is not None and getattr(self.logger, "log_dir", None):
            return self.logger.log_dir
        return self.default_root_dir

    @property
    def lightning_module(self) -> Optional[LightningModule]:
        return self.get_model()

    def get_model(self) -> Optional[LightningModule]:
        m = self.model
        while m is not None and hasattr(m, "module") and not isinstance(m, LightningModule):
            m = m.module
        return m

    # ---------------------------------------------------------------- public
    def fit(self, model: LightningModule, train_dataloader: Optional[DataLoader] = None,
            val_dataloaders: Optional[Union[DataLoader, List[DataLoader]]] = None,
            datamodule: Optional[LightningDataModule] = None):
        # PL 1.1: a datamodule passed positionally (reference examples/ray_ddp_tune.py:42)
        if isinstance(train_dataloader, LightningDataModule):
            datamodule, train_dataloader = train_dataloader, None
        self._attach(model, train_dataloader, val_dataloaders, None, datamodule)
        self.testing = False
        self._prepare_data_on_driver(model)
        results = self._launch(model)
        return results if results not in (None, 0) else 1

    def test(self, model: Optional[LightningModule] = None, test_dataloaders=None, ckpt_path: Optional[str] = "best",
             verbose: bool = True, datamodule: Optional[LightningDataModule] = None):
        if isinstance(test_dataloaders, LightningDataModule):
            datamodule, test_dataloaders = test_dataloaders, None
        if model is None:
            model = self.get_model()
            if ckpt_path == "best" and self.checkpoint_callback and self.checkpoint_callback.best_model_path:
                ckpt = load_checkpoint(self.checkpoint_callback.best_model_path)
                model.load_state_dict(ckpt["state_dict"])
            elif ckpt_path not in (None, "best"):
                ckpt = load_checkpoint(ckpt_path)
                model.load_state_dict(ckpt["state_dict"])
        self._attach(model, None, None, test_dataloaders, datamodule)
        self.testing = True
        self._prepare_data_on_driver(model)
        try:
            results = self._launch(model)
        finally:
            self.testing = False
        if verbose and results and self.is_global_zero:
            for i, r in enumerate(results):
                print(f"TEST RESULTS (dataloader {i}): {r}")
        return results

    def validate(self, model: Optional[LightningModule] = None, val_dataloaders=None,
                 datamodule: Optional[LightningDataModule] = None):
        model = model or self.get_model()
        self._attach(model, None, val_dataloaders, None, datamodule)
        model.trainer = self
        self._setup_stage(model, "validate")
        self._prepare_dataloaders(model)
        return self.run_evaluation(test_mode=False)

    def save_checkpoint(self, filepath: str, weights_only: bool = False, blocking: bool = True) -> None:
        """``blocking=False`` (ModelCheckpoint): the checkpoint dict is built now and
        written by the background writer (``RLAConfig.async_checkpoint``); a
        blocking save first drains earlier background writes (file order kept)."""
        self.wait_deferred()  # earlier background saves first (one writer, file order kept)
        mark("ckpt_dump_begin")
        ckpt = self.checkpoint_connector.dump_checkpoint(weights_only)
        mark("ckpt_dumped")
        if not self.is_global_zero:
            return
        if not blocking and get_config().async_checkpoint:
            # the writer PROCESS (pickling + file I/O off this process and its GIL);
            # until it has started, saves stay synchronous (short fits never wait
            # for its start-up)
            w = process_checkpoint_writer()
            if w.ready() or getattr(self, "_ckpt_writer", None) is w:
                self._ckpt_writer = w
                w.save(ckpt, filepath)
                mark("ckpt_handed_off")
                return
        self.wait_checkpoints()
        atomic_save(ckpt, filepath)

    def write_checkpoint(self, ckpt: dict, filepath: str) -> None:
        """Write an already-built checkpoint dict (the deferred saves' path): through
        the writer process when it is up, else in place.  Only rank 0 writes."""
        if ckpt is None or not self.is_global_zero:
            return
        w = getattr(self, "_ckpt_writer", None)
        if w is None and get_config().async_checkpoint:
            # the writer process started for this worker (ddp_train pre-warms it):
            # pickling and file I/O leave this process's GIL; later removals
            # (file_op) and wait_checkpoints order behind these writes
            from . import utilities as _u

            pw = _u._process_writer  # never started here (a spawn from this thread)
            if pw is not None and pw.alive() and pw.ready():
                self._ckpt_writer = w = pw
        if w is not None and w.alive():
            w.save(ckpt, filepath)
        else:
            atomic_save(ckpt, filepath)

    def file_op(self, fn, *args) -> None:
        """Run a checkpoint-file operation (e.g. a top-k removal) after the pending
        background writes, in order."""
        w = getattr(self, "_ckpt_writer", None)
        if w is not None:
            w.submit(fn, *args)
        else:
            fn(*args)

    def wait_checkpoints(self) -> None:
        """Block until every background checkpoint write has landed (re-raises a failed one)."""
        self.wait_deferred()
        w = getattr(self, "_ckpt_writer", None)
        if w is not None:
            w.wait()

    # ------------------------------------------------------------- driving
    def _attach(self, model, train_dl, val_dls, test_dls, datamodule) -> None:
        model.trainer = self
        self.model = model
        if train_dl is not None:
            self._train_dl_src = train_dl
        if val_dls is not None:
            self._val_dl_src = val_dls
        if test_dls is not None:
            self._test_dl_src = test_dls
        if datamodule is not None:
            self.datamodule = datamodule
            datamodule.trainer = self

    def _prepare_data_on_driver(self, model: LightningModule) -> None:
        # PL data_connector.prepare_data: on the DRIVER (reference examples rely on it,
        # ray_ddp_example.py:23-28: the dataset is pickled to the workers with the model)
        dm = self.datamodule
        if dm is not None and not getattr(dm, "has_prepared_data", False):
            dm.prepare_data()
            dm.has_prepared_data = True
        model.prepare_data()
        if self._log_dir is None and self.logger is not None:
            self._log_dir = self.logger.log_dir

    def _launch(self, model: LightningModule):
        from .accelerators import resolve_accelerator

        acc = resolve_accelerator(self)
        acc.trainer = self
        mark("fit_setup_begin")
        acc.setup(model)
        mark("fit_setup_end")
        try:
            results = acc.train()
        finally:
            mark("fit_teardown_begin")
            acc.teardown()
            mark("fit_teardown_end")
        return results

    # -------------------------------------------------- worker-side entry
    def _setup_stage(self, model: LightningModule, stage: str) -> None:
        dm = self.datamodule
        if dm is not None:
            flag = "has_setup_test" if stage == "test" else "has_setup_fit"
            if not getattr(dm, flag, False):
                dm.setup(stage)
                setattr(dm, flag, True)
        model.setup(stage)
        for cb in self.callbacks:
            cb.setup(self, model, stage)

    def call_setup_hook(self, model: LightningModule) -> None:
        self._setup_stage(model, "test" if self.testing else "fit")

    def _run(self, model: LightningModule):
        """Everything after process-group bring-up and device placement (runs on every worker)."""
        model.trainer = self
        self.model = model
        if self.benchmark and torch.cuda.is_available():
            torch.backends.cudnn.benchmark = True  # PL 1.1: Trainer(benchmark=True)
        self.call_setup_hook(model)
        mark("setup_hook_done", rank=self.global_rank)
        self._prepare_dataloaders(model)
        mark("dataloaders_ready", rank=self.global_rank)
        if self.testing:
            self.optimizers, self.lr_schedulers = [], []
            results = self.run_test()
            model.teardown("test")
            return results
        opts, scheds = _normalize_optimizers(model.configure_optimizers())
        mark("configure_optimizers_done", rank=self.global_rank)
        self.optimizers, self.lr_schedulers = self.accelerator_backend.setup_optimizers(model, opts, scheds)
        mark("optimizers_ready", rank=self.global_rank)
        self.accelerator_backend.configure_ddp(model)
        mark("ddp_configured", rank=self.global_rank)
        self._fused = self._maybe_fused(model)
        self.fused_step_health = None
        mark("fused_step_ready", rank=self.global_rank)
        if self.resume_from_checkpoint and os.path.exists(self.resume_from_checkpoint):
            self.checkpoint_connector.restore(self.resume_from_checkpoint, on_gpu=self.on_gpu)
        try:
            self.run_train()
        finally:
            self.wait_checkpoints()  # every checkpoint file is on disk when fit returns
            q = getattr(self, "_deferred", None)
            if q is not None:  # its thread ends with the fit (a later save starts a new one)
                q.close()
        f = self._fused
        if f is not None and hasattr(f, "check"):
            f.check(blocking=True)  # the epoch-end checks trail by one epoch: the last one here
            if hasattr(f, "health"):
                # the fused MNIST step's saturation / non-finite counts of the whole fit
                self.fused_step_health = f.health()
                mark("fused_step_health", rank=self.global_rank, **self.fused_step_health)
        model.teardown("fit")
        return None

    def _maybe_fused(self, model: LightningModule):
        """Model-provided fused training step (e.g. MNISTClassifier's single HIP launch),
        else the graph-captured autograd step when the module opts in
        (``lightning/graph_step.py``)."""
        want = self.fused_step
        if want is False:
            return None
        if not hasattr(model, "configure_fused_step"):
            from .graph_step import maybe_graph_step

            return maybe_graph_step(self, model)
        # accumulate_grad_batches: only a fused step that accumulates itself (it reads
        # trainer.accumulate_grad_batches and counts the optimizer steps); a model
        # declines by leaving ``fused_step_accumulates`` unset
        if self.accumulate_grad_batches != 1 and not getattr(model, "fused_step_accumulates", False):
            return None
        # gradient_clip_val: only a fused step that clips itself (it reads
        # trainer.gradient_clip_val); a model declines by leaving
        # ``fused_step_clips_gradients`` unset, or by raising in configure_fused_step
        if self.gradient_clip_val and not getattr(model, "fused_step_clips_gradients", False):
            return None
        try:
            return model.configure_fused_step(self)
        except Exception as e:  # noqa: BLE001
            if want:
                raise
            log.info(f"fused step unavailable ({e!r}); using the autograd path")
            return None

    # ----------------------------------------------------------- dataloaders
    def _resolve_loader(self, name: str, model: LightningModule):
        src = {"train": self._train_dl_src, "val": self._val_dl_src, "test": self._test_dl_src}[name]
        if src is None and self.datamodule is not None:
            src = getattr(self.datamodule, f"{name}_dataloader")()
        if src is None:
            src = getattr(model, f"{name}_dataloader")()
        return src

    def _maybe_replace_sampler(self, dl: DataLoader, shuffle: bool) -> DataLoader:
        acc = self.accelerator_backend
        if dl is None or acc is None or not acc.require_distributed_sampler or not self.replace_sampler_ddp:
            return dl
        if isinstance(dl.sampler, DistributedSampler):
            return dl
        kw = dict(acc.distributed_sampler_kwargs)
        sampler = DistributedSampler(dl.dataset, shuffle=shuffle, **kw)
        return DataLoader(
            dl.dataset, batch_size=dl.batch_size, sampler=sampler, num_workers=dl.num_workers,
            collate_fn=dl.collate_fn, pin_memory=dl.pin_memory, drop_last=dl.drop_last,
            timeout=dl.timeout, worker_init_fn=dl.worker_init_fn,
            persistent_workers=getattr(dl, "persistent_workers", False) and dl.num_workers > 0,
        )

    @staticmethod
    def _num_batches(dl, limit) -> int:
        try:
            n = len(dl)
        except TypeError:
            n = math.inf
        if isinstance(limit, float):
            if limit >= 1.0:
                return n if n != math.inf else int(1e18)
            return int(n * limit) if n != math.inf else int(1e18)
        return min(int(limit), n) if n != math.inf else int(limit)

    def _prepare_dataloaders(self, model: LightningModule) -> None:
        if not self.testing:
            dl = self._resolve_loader("train", model)
            self.train_dataloader = self._maybe_replace_sampler(dl, shuffle=True) if dl is not None else None
            self.num_training_batches = self._num_batches(self.train_dataloader, self.limit_train_batches) \
                if self.train_dataloader is not None else 0
            vdl = self._resolve_loader("val", model)
            self.val_dataloaders = self._as_list(vdl, shuffle=False)
            self.num_val_batches = [self._num_batches(d, self.limit_val_batches) for d in self.val_dataloaders]
            has_val_step = type(model).validation_step is not LightningModule.validation_step
            self._has_val_loop = bool(self.val_dataloaders) and has_val_step and \
                sum(self.num_val_batches) > 0
        else:
            tdl = self._resolve_loader("test", model)
            self.test_dataloaders = self._as_list(tdl, shuffle=False)
            self.num_test_batches = [self._num_batches(d, self.limit_test_batches) for d in self.test_dataloaders]

    def _as_list(self, dls, shuffle: bool) -> List[DataLoader]:
        if dls is None:
            return []
        if not isinstance(dls, (list, tuple)):
            dls = [dls]
        return [self._maybe_replace_sampler(d, shuffle=shuffle) for d in dls]

    # ---------------------------------------------------------------- hooks
    def call_hook(self, name: str, *args, **kwargs):
        model = self.get_model()
        for cb in self.callbacks:
            fn = getattr(cb, name, None)
            if fn is not None:
                fn(self, model, *args, **kwargs)
        mfn = getattr(model, name, None)
        if mfn is not None and callable(mfn):
            return mfn(*args, **kwargs) if name != "on_train_epoch_end" else mfn(*args, **kwargs)
        return None

    # -------------------------------------------------------------- metrics
    def _log_metric(self, module, name, value, prog_bar=False, logger=True, on_step=None, on_epoch=None,
                    sync_dist=False, sync_dist_op="mean") -> None:
        fx = self._current_fx or "training_step"
        if self._log_sink is not None:
            # graph-captured step: recorded, replayed per step from the device ring
            self._log_sink.append((name, value, dict(prog_bar=prog_bar, logger=logger, on_step=on_step,
                                                     on_epoch=on_epoch, sync_dist=sync_dist,
                                                     sync_dist_op=sync_dist_op), fx))
            return
        training = fx.startswith("training")
        if on_step is None:
            on_step = training
        if on_epoch is None:
            on_epoch = not training
        if not isinstance(value, torch.Tensor):
            value = torch.tensor(float(value))
        fresh = getattr(value, "_rla_fresh", False)
        value = value.detach()
        if fresh:  # framework-made value that nothing writes before the log flush
            value._rla_fresh = True
        if sync_dist and self.accelerator_backend is not None:
            value = self.accelerator_backend.sync_tensor(value.float(), reduce_op=sync_dist_op)
        store = self._results.setdefault(fx, defaultdict(list))
        if on_epoch:
            store[name].append(value)
        if on_step:
            key = name if not on_epoch else f"{name}_step"
            self.callback_metrics[key] = value
            if logger:
                self.logged_metrics[key] = value
            if prog_bar:
                self.progress_bar_metrics[key] = value
        self._results.setdefault("_meta", {})[name] = (prog_bar, logger, on_step, on_epoch)

    def _reduce_epoch_metrics(self, fx: str) -> Dict[str, torch.Tensor]:
        store = self._results.pop(fx, None) or {}
        meta = self._results.get("_meta", {})
        out = {}
        for name, vals in store.items():
            # reduced where the values live: one device tensor, no host sync per value
            dev = vals[0].device
            v = torch.stack([x.float().mean().to(dev) for x in vals]).mean()
            prog_bar, logger, on_step, on_epoch = meta.get(name, (False, True, False, True))
            key = f"{name}_epoch" if on_step else name
            out[key] = v
            self.callback_metrics[key] = v
            if logger:
                self.logged_metrics[key] = v
            if prog_bar:
                self.progress_bar_metrics[key] = v
        return out

    def _absorb_legacy(self, out: Any) -> None:
        """PL <1.0 style dict returns ({'val_loss':..., 'log': {...}, 'progress_bar': {...}})."""
        if not isinstance(out, dict):
            return
        for k, v in out.items():
            if k in ("log", "progress_bar") and isinstance(v, dict):
                for kk, vv in v.items():
                    t = vv.detach() if isinstance(vv, torch.Tensor) else torch.tensor(float(vv))
                    self.callback_metrics[kk] = t
                    (self.logged_metrics if k == "log" else self.progress_bar_metrics)[kk] = t
            elif isinstance(v, torch.Tensor) and v.numel() == 1:
                self.callback_metrics[k] = v.detach()

    def _flush_logger(self, defer: bool = False) -> None:
        """Hand ``logged_metrics`` to the logger.  ``defer`` (multi-step dispatch):
        the device values are only referenced (no copy, no wait) and written, in
        step order, at the next blocking flush (validation / epoch end, which sync
        anyway) with ONE batched device->host transfer for all of them.  A
        per-log-point D2H copy made the host wait for the GPU queue at every
        50-step dispatch chunk (the host then could not run ahead, and its ~0.5 ms
        of per-chunk work showed up as GPU idle time)."""
        self._write_pending_log(block=not defer)
        if self.logger is None or not self.logged_metrics or not self.is_global_zero:
            return
        metrics = dict(self.logged_metrics)
        if not defer:
            self._drain_staged_logs(wait=True)  # earlier steps' rows first
        if defer and any(isinstance(v, torch.Tensor) and v.is_cuda for v in metrics.values()):
            # a device-side copy (no host sync): a logged tensor the module later
            # changes in place must still be written with its value at log time
            snap = {k: (v.detach().clone() if isinstance(v, torch.Tensor) and not getattr(v, "_rla_fresh", False)
                        else v) for k, v in metrics.items()}
            if self._pending_log is None:
                self._pending_log = []
            self._pending_log.append((snap, self.global_step))
            return
        self.logger.log_metrics(metrics, step=self.global_step)

    def _stage_pending_log(self) -> None:
        """Start the host transfer of the deferred snapshots WITHOUT waiting: one
        concatenation + one async copy into pinned memory per dtype, an event behind
        them; the rows are written by :meth:`_drain_staged_logs` once it completed --
        the validation end no longer holds the next epoch's first dispatch for the
        logger's file writes (~0.5 ms of GPU idle per epoch, profiles/r3_trainer)."""
        pending = self._pending_log or []
        if not pending:
            return
        self._pending_log = None
        dev_vals = [(i, k, v) for i, (snap, _) in enumerate(pending) for k, v in snap.items()
                    if isinstance(v, torch.Tensor) and v.is_cuda]
        st = {"pending": pending, "groups": [], "event": None}
        if dev_vals:
            groups: Dict[torch.dtype, list] = {}
            for e in dev_vals:
                groups.setdefault(e[2].dtype, []).append(e)
            for dtype, ents in groups.items():
                flat = torch.cat([v.reshape(-1) for _, _, v in ents])
                host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
                host.copy_(flat, non_blocking=True)
                st["groups"].append((ents, host))
            st["event"] = torch.cuda.Event()
            st["event"].record()
        self._staged_logs.append(st)

    def _drain_staged_logs(self, wait: bool) -> None:
        """Write staged rows in step order, as far as their copies completed (``wait``: all)."""
        while self._staged_logs:
            st = self._staged_logs[0]
            ev = st["event"]
            if ev is not None and not ev.query():
                if not wait:
                    return
                ev.synchronize()
            pending = st["pending"]
            for ents, host in st["groups"]:
                vals = host.double().tolist()
                off = 0
                for i, k, v in ents:
                    n = v.numel()
                    pending[i][0][k] = vals[off] if n == 1 else host[off: off + n].reshape(v.shape).clone()
                    off += n
            for snap, step in pending:
                self.logger.log_metrics(snap, step=step)
            self._staged_logs.pop(0)

    def _write_pending_log(self, block: bool = True) -> None:
        """Write the deferred snapshots in step order (``block``, or once more than
        1024 are held), their device values fetched by one batched transfer."""
        if block:
            self._drain_staged_logs(wait=True)
        pending = self._pending_log or []
        if not pending or (not block and len(pending) <= 1024):
            return
        dev_vals = [(i, k, v) for i, (snap, _) in enumerate(pending) for k, v in snap.items()
                    if isinstance(v, torch.Tensor) and v.is_cuda]
        if dev_vals:
            # ONE concatenation kernel and ONE device->host copy per dtype (a per-value
            # cast launched ~70 kernels per epoch: ~1 ms of host time while the GPU idled)
            groups: Dict[torch.dtype, list] = {}
            for e in dev_vals:
                groups.setdefault(e[2].dtype, []).append(e)
            for dtype, ents in groups.items():
                flat = torch.cat([v.reshape(-1) for _, _, v in ents]).cpu()
                vals = flat.double().tolist()
                off = 0
                for i, k, v in ents:
                    n = v.numel()
                    # scalars as Python floats (what the logger records), tensors re-shaped
                    pending[i][0][k] = vals[off] if n == 1 else flat[off: off + n].reshape(v.shape)
                    off += n
        for snap, step in pending:
            self.logger.log_metrics(snap, step=step)
        self._pending_log = None

    # ---------------------------------------------------------- evaluation
    def run_sanity_check(self, model: LightningModule) -> None:
        if not self._has_val_loop or self.num_sanity_val_steps == 0:
            return
        self.running_sanity_check = True
        self.call_hook("on_sanity_check_start")
        n = self.num_sanity_val_steps if self.num_sanity_val_steps > 0 else None
        self.run_evaluation(test_mode=False, max_batches=n)
        self.call_hook("on_sanity_check_end")
        # PL resets metrics logged during the sanity check
        self.callback_metrics = {}
        self.logged_metrics = {}
        self.progress_bar_metrics = {}
        self.running_sanity_check = False

    def run_evaluation(self, test_mode: bool = False, max_batches: Optional[int] = None):
        model = self.get_model()
        stage = "test" if test_mode else "validation"
        dls = self.test_dataloaders if test_mode else self.val_dataloaders
        nbs = self.num_test_batches if test_mode else self.num_val_batches
        if not dls:
            return []
        was_training = model.training
        model.eval()
        mark("eval_start", stage=stage)
        self.call_hook(f"on_{stage}_start")
        self.call_hook(f"on_{stage}_epoch_start")
        fused_eval = (self._fused is not None and not test_mode and hasattr(self._fused, "eval_epoch")
                      and len(dls) == 1 and self._fused.eval_compatible(model)
                      and not self._eval_batch_hooks_overridden(model))
        all_outputs = []
        with torch.no_grad():
            for dl_idx, dl in enumerate(dls):
                limit = nbs[dl_idx] if max_batches is None else min(max_batches, nbs[dl_idx])
                outputs = []
                res = self._fused.eval_epoch(dl, limit) if fused_eval else None
                if res is not None:
                    # the pass over the resident data: either one output standing for
                    # `limit` equal-size batches (the fused MNIST pass, same epoch-end
                    # mean) or the per-batch outputs (device-gathered batches)
                    all_outputs.append(res if isinstance(res, list) else [res])
                    continue
                for batch_idx, batch in enumerate(dl):
                    if batch_idx >= limit:
                        break
                    batch = self.accelerator_backend.batch_to_device(batch)
                    self.call_hook(f"on_{stage}_batch_start", batch, batch_idx, dl_idx)
                    self._current_fx = f"{stage}_step"
                    args = [batch, batch_idx] + ([dl_idx] if len(dls) > 1 else [])
                    with self.accelerator_backend.autocast():
                        out = getattr(model, f"{stage}_step")(*args)
                    self._current_fx = f"{stage}_step_end"
                    out = getattr(model, f"{stage}_step_end")(out)
                    self._current_fx = None
                    self.call_hook(f"on_{stage}_batch_end", out, batch, batch_idx, dl_idx)
                    if out is not None:
                        outputs.append(out)
                all_outputs.append(outputs)
        mark("eval_launched", stage=stage)
        self._current_fx = f"{stage}_epoch_end"
        epoch_out = getattr(model, f"{stage}_epoch_end")(all_outputs[0] if len(dls) == 1 else all_outputs)
        self._absorb_legacy(epoch_out)
        self._current_fx = None
        metrics = {}
        metrics.update(self._reduce_epoch_metrics(f"{stage}_step"))
        metrics.update(self._reduce_epoch_metrics(f"{stage}_step_end"))
        metrics.update(self._reduce_epoch_metrics(f"{stage}_epoch_end"))
        self.call_hook(f"on_{stage}_epoch_end")
        mark("eval_epoch_end_hooks", stage=stage)
        if stage == "validation" and not self.running_sanity_check:
            self._consolidate_optimizer_state()
        self.call_hook(f"on_{stage}_end")
        mark("eval_end_hooks", stage=stage)
        if stage == "validation" and getattr(self, "world_size", 1) > 1 and not self.deferred_checkpoints_ok():
            # ModelCheckpoint (on_validation_end) may have rank 0 writing a file: the
            # other ranks wait for it here, not inside the next step's gradient
            # collective, where a long write would look like a stalled peer.  (Deferred
            # checkpoints write in the background: no rank waits, no barrier.)
            acc = self.accelerator_backend
            if acc is not None and hasattr(acc, "barrier"):
                acc.barrier("validation_end")
        if was_training:
            model.train()
        if not self.running_sanity_check:
            if self.on_gpu and self.training and self.logger is not None and self.is_global_zero:
                # rows go out asynchronously; written while the next chunks run
                self._flush_logger(defer=True)
                self._stage_pending_log()
            else:
                self._flush_logger()
        # inside fit nobody reads the returned floats: no host sync for them (the
        # epoch end then never waits for the device; validate()/test() do convert)
        out = [metrics] if (self.training and not self.running_sanity_check) else [_floats(metrics)]
        mark("eval_done", stage=stage)
        return out

    def run_test(self):
        model = self.get_model()
        results = self.run_evaluation(test_mode=True)
        self.test_results = results
        return results

    # -------------------------------------------------------------- training
    def _should_validate(self, batch_idx: int, is_last: bool) -> bool:
        if not self._has_val_loop or (self.current_epoch + 1) % self.check_val_every_n_epoch != 0:
            return False
        vci = self.val_check_interval
        if isinstance(vci, float):
            if vci >= 1.0:
                return is_last
            every = max(1, int(self.num_training_batches * vci))
        else:
            every = int(vci)
        return (batch_idx + 1) % every == 0 or is_last

    def run_train(self) -> None:
        model = self.get_model()
        self.training = True
        self.call_hook("on_fit_start")
        for cb in self.callbacks:
            if hasattr(cb, "on_pretrain_routine_start"):
                cb.on_pretrain_routine_start(self, model)
        if self.logger is not None:
            self.logger.rank = self.global_rank
            if self.is_global_zero and model.hparams:
                self.logger.log_hyperparams(model.hparams)
        self.run_sanity_check(model)
        mark("sanity_check_done", rank=self.global_rank)
        self.call_hook("on_train_start")
        # Everything alive now (torch, the model, the data) is long-lived: move it
        # out of the cyclic GC's generations, so a full collection during the
        # epochs scans only the loop's own garbage instead of pausing the
        # dispatching host for ~100 ms (measured on the fused MNIST epochs).
        # No collection first: it cost 80-240 ms per Tune trial (profiles/r3_tune);
        # garbage frozen here is collected after the fit (gc.unfreeze below).
        gc.freeze()
        # RLA_PROFILE_EPOCHS=<path>: host profile (cProfile) of the steady epochs (the
        # first is skipped: imports / graph capture), written per rank on fit end
        prof_path = os.environ.get("RLA_PROFILE_EPOCHS")
        prof = None
        if prof_path:
            import cProfile

            prof = cProfile.Profile()
        try:
            while self.current_epoch < self.max_epochs:
                if prof is not None and self.current_epoch == 1:
                    prof.enable()
                self._run_epoch(model)
                if self.max_steps is not None and self.global_step >= self.max_steps:
                    break
                if self.should_stop and self.current_epoch + 1 >= self.min_epochs:
                    break
                self.current_epoch += 1
                self.should_stop = False if self.current_epoch < self.min_epochs else self.should_stop
        except KeyboardInterrupt:
            self.interrupted = True
            self.call_hook("on_keyboard_interrupt")
        finally:
            gc.unfreeze()
            if prof is not None:
                prof.disable()
                self._dump_profile(prof, prof_path)
        # every rank, before a checkpoint callback may dump on rank 0 only
        self._consolidate_optimizer_state()
        self.call_hook("on_train_end")
        self.call_hook("on_fit_end")
        if self.logger is not None:
            self._write_pending_log()
            self.logger.finalize("success")
        self.training = False
        self.profiler_summary = self.profiler.summary()
        if self.profiler_summary and self.is_global_zero:
            print(self.profiler_summary, flush=True)

    def _dump_profile(self, prof, path: str) -> None:
        import io
        import pstats

        buf = io.StringIO()
        st = pstats.Stats(prof, stream=buf)
        st.sort_stats("tottime").print_stats(40)
        st.sort_stats("cumulative").print_stats(80)
        with open(f"{path}.rank{self.global_rank}.txt", "w") as f:
            f.write(buf.getvalue())

    def _run_epoch(self, model: LightningModule) -> None:
        dl = self.train_dataloader
        sampler = getattr(dl, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(self.current_epoch)
        mark("epoch_start", rank=self.global_rank, epoch=self.current_epoch)
        self.call_hook("on_epoch_start")
        self.call_hook("on_train_epoch_start")
        epoch_outputs: List[Any] = []
        n = self.num_training_batches
        validated = False
        batches = None
        chunk = self._dispatch_chunk(model)
        if self._fused is not None and hasattr(self._fused, "make_epoch_batches") and \
                (chunk > 1 or not self._batch_hooks_overridden(model)) and dl is not None and n > 0:
            batches = self._fused.make_epoch_batches(dl, n)  # data stays resident on the device
            mark("epoch_order_ready", epoch=self.current_epoch)
            if batches is not None:
                n = min(n, len(batches))
        if dl is not None and n > 0 and chunk > 1 and batches is not None:
            validated = self._run_chunked(model, n, chunk, epoch_outputs)
        elif dl is not None and n > 0:
            for batch_idx, batch in enumerate(batches if batches is not None else dl):
                if batch_idx >= n:
                    break
                is_last = batch_idx + 1 >= n
                out = self._train_batch(model, batch, batch_idx, is_last)
                if out is not None:
                    epoch_outputs.append(out)
                if self.max_steps is not None and self.global_step >= self.max_steps:
                    is_last = True
                if self._should_validate(batch_idx, is_last):
                    self.run_evaluation(test_mode=False)
                    validated = True
                if is_last and self.max_steps is not None and self.global_step >= self.max_steps:
                    break
                if self.should_stop:
                    break
        mark("epoch_train_done", epoch=self.current_epoch)
        self._current_fx = "training_epoch_end"
        res = model.training_epoch_end(epoch_outputs)
        self._absorb_legacy(res)
        self._current_fx = None
        self._reduce_epoch_metrics("training_step")
        self._reduce_epoch_metrics("training_step_end")
        self._reduce_epoch_metrics("training_epoch_end")
        # PL 1.1: on_epoch_end, then on_train_epoch_end
        self.call_hook("on_epoch_end")
        for cb in self.callbacks:
            cb.on_train_epoch_end(self, model, epoch_outputs)
        model.on_train_epoch_end(epoch_outputs)
        self._update_lr_schedulers("epoch")
        if not self._has_val_loop:
            # PL 1.1 TrainLoop.run_training_epoch: with no validation loop
            # (should_train_only) the checkpoint callbacks run at every training-epoch
            # end (check_checkpoint_callback -> ModelCheckpoint.on_validation_end)
            self._consolidate_optimizer_state()
            for cb in self.checkpoint_callbacks:
                cb.on_validation_end(self, model)
        if not validated:
            if self.on_gpu and self.logger is not None and self.is_global_zero and torch.cuda.is_available():
                # rows go out asynchronously (one batched copy, written once it landed):
                # no host sync at the end of an epoch without validation either
                self._flush_logger(defer=True)
                self._stage_pending_log()
            else:
                self._flush_logger()
        self._check_collectives()
        mark("epoch_end", epoch=self.current_epoch)

    def _check_collectives(self) -> None:
        """Fail fast on a collective that went wrong this epoch: the xGMI kernels'
        bounded polls set an error word instead of hanging on a dead / stalled peer
        (and skip that block's reduction), RCCL reports async errors -- surface
        either as an exception on every rank."""
        from ..parallel.comm import get_native_comm

        comm = get_native_comm(create=False)
        if comm is not None:
            comm.check()
        # the fused one-launch step's in-launch hand-off (a bounded wait that expired
        # means a block overwrote state another block was still reading)
        f = getattr(self, "_fused", None)
        if f is not None and hasattr(f, "check"):
            f.check(blocking=False)  # the previous epoch's flag: no device sync here

    def _dispatch_chunk(self, model: LightningModule) -> int:
        """Steps per host dispatch of the fused resident step (1 = one per batch).

        Several steps go out at once (hipGraph replays, no per-batch Python) only
        when nothing observes single batches: no batch hooks (callbacks that
        implement ``on_train_chunk_end`` are chunk-aware and fine), no fault
        injection at a given step, and no step-interval LR scheduler the fused step
        cannot follow on the device: one that declares ``schedules_lr`` is handed each
        chunk's rates (``_chunk_lr_schedule``) -- ``ReduceLROnPlateau`` (it reads a metric
        per step), a scheduler that also cycles the momentum (``OneCycleLR`` / ``CyclicLR``
        with ``cycle_momentum``: it rewrites ``betas`` / ``momentum`` per step, which a
        captured graph bakes) and several optimizers or parameter groups still go out per
        batch."""
        f = self._fused
        if f is None or not hasattr(f, "train_chunk"):
            return 1
        if self.accumulate_grad_batches != 1:
            return 1  # _run_chunked equates batches with global steps: windows go out per batch
        k = self.steps_per_dispatch if self.steps_per_dispatch is not None else get_config().steps_per_dispatch
        k = min(int(k), int(getattr(f, "max_chunk", 1)))
        if k <= 1 or self._batch_hooks_overridden(model, chunk_aware_ok=True):
            return 1
        if any(getattr(model, nm, None) is not None for nm in ("on_batch_start", "on_batch_end")):
            return 1
        step_scheds = self._step_schedulers()
        if step_scheds and (not getattr(f, "schedules_lr", False) or not hasattr(f, "set_lr_schedule")
                            or any(s.get("reduce_on_plateau") or getattr(s["scheduler"], "cycle_momentum", False)
                                   for s in step_scheds)
                            or len(self.optimizers) != 1 or len(self.optimizers[0].param_groups) != 1):
            return 1
        if os.environ.get("RLA_FAULT_STEP") is not None:
            return 1
        return k

    def _step_schedulers(self) -> List[dict]:
        return [s for s in self.lr_schedulers if s.get("interval", "epoch") == "step"]

    def _chunk_lr_schedule(self, k: int) -> Optional[List[float]]:
        """The rates of the next ``k`` steps, derived by doing on the host exactly what ``k``
        per-batch iterations do: step i runs at the group's current rate, then every
        step-interval scheduler whose ``frequency`` divides ``global_step + i`` steps.  The
        schedulers, ``param_groups[0]["lr"]`` and the checkpointed scheduler state are
        afterwards what the per-batch loop leaves behind the chunk's last step.  None: no
        step-interval scheduler."""
        scheds = self._step_schedulers()
        if not scheds:
            return None
        group = self.optimizers[0].param_groups[0]
        rates = []
        for i in range(1, k + 1):
            rates.append(float(group["lr"]))
            for s in scheds:
                if (self.global_step + i) % s.get("frequency", 1) == 0:
                    s["scheduler"].step()
        return rates

    def _run_chunked(self, model: LightningModule, n: int, chunk: int, epoch_outputs: List[Any]) -> bool:
        """The epoch's ``n`` resident batches in dispatches of <= ``chunk`` steps.
        A dispatch ends where the per-batch loop would do host work: a logger
        flush (``log_every_n_steps``), a validation point, ``max_steps`` or the
        epoch end -- so metrics, checkpoints and Tune reports land on the same
        steps as with per-batch dispatch.  Returns whether validation ran."""
        every = max(1, self.log_every_n_steps)
        bsz = int(getattr(self._fused, "_B", 0))
        validated = False
        # the fused step reports every log point of a chunk itself (ring views): the
        # chunk need not end at each one (35 cuts -> 1-2 per MNIST epoch)
        spans = bool(getattr(self._fused, "chunk_spans_log_points", False)) and self.logger is not None
        self._chunks_span_logs = spans
        # RLA_CHUNK_TIMING=1 (diagnostic): host time per chunk vs the GPU time
        # between chunk-end events, reported at the epoch end (which syncs anyway)
        timing = [] if os.environ.get("RLA_CHUNK_TIMING") == "1" and torch.cuda.is_available() else None
        b = 0
        while b < n:
            if timing is not None:
                h0 = time.perf_counter()
            e = b
            while True:
                e += 1
                gs = self.global_step + (e - b)
                if (e >= n or e - b >= chunk or (gs % every == 0 and not spans)
                        or self._should_validate(e - 1, False)
                        or (self.max_steps is not None and gs >= self.max_steps)):
                    break
            k = e - b
            # the chunk's per-step rates (chunks end at validation, max_steps and the epoch
            # end, so no scheduler is stepped past a stop); chunk-aware callbacks read them
            self._chunk_rates = self._chunk_lr_schedule(k)
            if self._chunk_rates is not None:
                self._fused.set_lr_schedule(self._chunk_rates)
            self.profiler.start("run_training_batch")
            outs = self._fused.train_chunk(k)
            self.profiler.stop("run_training_batch")
            if b == 0:
                mark("first_chunk_dispatched", epoch=self.current_epoch)
            if self._staged_logs:
                self._drain_staged_logs(wait=False)  # the previous validation's rows, if copied
            self.global_step += k
            epoch_outputs.extend(outs)
            self._lr_log_points = None
            for cb in self.callbacks:
                fn = getattr(cb, "on_train_chunk_end", None)
                if fn is not None:
                    fn(self, model, outs, k, k * bsz)
            if spans:
                rows = getattr(self._fused, "_last_rows", None)
                if rows is not None and rows.size(0) == k:
                    final, current = self.global_step, dict(self.logged_metrics)
                    lr_points = self._lr_log_points or {}
                    for st, met in self._fused.log_points(rows, final - k, every):
                        self.global_step = st  # the row is written under its own step
                        self.logged_metrics.update(met)
                        self.logged_metrics.update(lr_points.get(st, {}))  # LearningRateMonitor("step")
                        self._flush_logger(defer=True)
                    self.global_step = final
                    self.logged_metrics.clear()
                    self.logged_metrics.update(current)  # the chunk's last step, as before
                elif self.global_step % every == 0:
                    self._flush_logger(defer=True)
            elif self.global_step % every == 0:
                self._flush_logger(defer=True)
            if timing is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                timing.append((k, time.perf_counter() - h0, ev, getattr(self._fused, "_last_run_us", 0.0)))
            is_last = e >= n or (self.max_steps is not None and self.global_step >= self.max_steps)
            if is_last and hasattr(self._fused, "prefetch_next_epoch") and self.train_dataloader is not None \
                    and self.current_epoch + 1 < self.max_epochs:
                # host work of the next epoch's start, done while the GPU runs this one's tail
                self._fused.prefetch_next_epoch(self.train_dataloader, self.current_epoch + 1)
            if self._should_validate(e - 1, is_last):
                if timing is not None:
                    self._report_chunk_timing(timing)
                    timing = None
                self.run_evaluation(test_mode=False)
                validated = True
            if is_last or self.should_stop:
                break
            b = e
        if timing:
            self._report_chunk_timing(timing)
        return validated

    @staticmethod
    def _report_chunk_timing(timing) -> None:
        torch.cuda.synchronize()
        host = sorted(t[1] * 1e6 for t in timing)
        run = sorted(t[3] for t in timing)
        gpu = sorted(a[2].elapsed_time(b[2]) * 1e3 / b[0] for a, b in zip(timing, timing[1:]))
        if gpu:
            print(f"[chunk-timing] chunks={len(timing)} host_us_per_chunk_median={host[len(host) // 2]:.1f} "
                  f"engine_run_us_median={run[len(run) // 2]:.1f} "
                  f"host_us_max={host[-1]:.1f} gpu_us_per_step_median={gpu[len(gpu) // 2]:.3f} "
                  f"gpu_us_per_step_max={gpu[-1]:.3f} steps={sum(t[0] for t in timing)}", file=sys.stderr,
                  flush=True)

    def _eval_batch_hooks_overridden(self, model: LightningModule) -> bool:
        names = ("on_validation_batch_start", "on_validation_batch_end")
        for cb in self.callbacks:
            for nm in names:
                if getattr(type(cb), nm, None) is not getattr(Callback, nm, None):
                    return True
        return any(getattr(type(model), nm, None) is not getattr(LightningModule, nm, None) or nm in model.__dict__
                   for nm in names)

    def _batch_hooks_overridden(self, model: LightningModule, chunk_aware_ok: bool = False) -> bool:
        names = ("on_train_batch_start", "on_train_batch_end", "on_batch_start", "on_batch_end")
        for cb in self.callbacks:
            if chunk_aware_ok and callable(getattr(cb, "on_train_chunk_end", None)):
                continue
            for nm in names:
                if getattr(type(cb), nm, None) is not getattr(Callback, nm):
                    return True
        for nm in ("on_train_batch_start", "on_train_batch_end"):
            if getattr(type(model), nm) is not getattr(LightningModule, nm) or nm in model.__dict__:
                return True
        return False

    def _train_batch(self, model: LightningModule, batch, batch_idx: int, is_last: bool):
        self.call_hook("on_batch_start")
        r = model.on_train_batch_start(batch, batch_idx, 0)
        for cb in self.callbacks:
            cb.on_train_batch_start(self, model, batch, batch_idx, 0)
        if r == -1:
            return None
        maybe_inject_fault(self.global_rank, self.global_step)
        self.profiler.start("run_training_batch")
        if self._fused is not None:
            out = self._fused.train_batch(batch, batch_idx)
            if not getattr(self._fused, "counts_steps", False):
                self.global_step += 1
                self._update_lr_schedulers("step")  # (a step that counts itself steps them itself)
        else:
            out = self._autograd_step(batch, batch_idx, is_last)
        self.profiler.stop("run_training_batch")
        for cb in self.callbacks:
            cb.on_train_batch_end(self, model, out, batch, batch_idx, 0)
        model.on_train_batch_end(out, batch, batch_idx, 0)
        self.call_hook("on_batch_end")
        if self.global_step % max(1, self.log_every_n_steps) == 0:
            self._flush_logger()
        return out

    def _autograd_step(self, batch, batch_idx: int, is_last: bool = False):
        """The eager autograd step of one batch (every optimizer), step counting and
        step-interval LR schedulers included."""
        model = self.get_model()
        batch = self.accelerator_backend.batch_to_device(batch)
        out = None
        for opt_idx, opt in enumerate(self.optimizers or [None]):
            out = self._optimizer_step_for(model, batch, batch_idx, opt_idx, opt, is_last)
        accumulate_done = ((batch_idx + 1) % self.accumulate_grad_batches == 0) or is_last
        if accumulate_done:
            self.global_step += 1
            self._update_lr_schedulers("step")
        return out

    def _optimizer_step_for(self, model, batch, batch_idx, opt_idx, opt, is_last):
        acc = self.accelerator_backend
        n_opt = len(self.optimizers)
        accumulate_done = ((batch_idx + 1) % self.accumulate_grad_batches == 0) or is_last
        self._current_fx = "training_step"
        args = [batch, batch_idx] + ([opt_idx] if n_opt > 1 else [])
        acc.before_forward(sync=accumulate_done)
        with acc.autocast():
            out = model.training_step(*args)
        self._current_fx = "training_step_end"
        out = model.training_step_end(out)
        self._current_fx = None
        if out is None:
            return None
        loss = out if isinstance(out, torch.Tensor) else out["loss"]
        if isinstance(out, dict):
            self._absorb_legacy({k: v for k, v in out.items() if k in ("log", "progress_bar")})
        if opt is not None:
            scaled = loss / self.accumulate_grad_batches if self.accumulate_grad_batches > 1 else loss
            acc.backward(model, scaled, opt, opt_idx)
            model.on_after_backward()
            for cb in self.callbacks:
                cb.on_after_backward(self, model)
            if accumulate_done:
                acc.before_optimizer_step(opt)
                if self.gradient_clip_val:
                    acc.clip_gradients(opt, self.gradient_clip_val)
                model.optimizer_step(self.current_epoch, batch_idx, opt, opt_idx, None)
                model.on_before_zero_grad(opt)
                for cb in self.callbacks:
                    cb.on_before_zero_grad(self, model, opt)
                model.optimizer_zero_grad(self.current_epoch, batch_idx, opt, opt_idx)
        self.callback_metrics.setdefault("loss", loss.detach())
        self.callback_metrics["loss"] = loss.detach()
        if isinstance(out, dict):
            return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
        return {"loss": loss.detach()}

    def _update_lr_schedulers(self, interval: str) -> None:
        for s in self.lr_schedulers:
            if s.get("interval", "epoch") != interval:
                continue
            freq = s.get("frequency", 1)
            counter = self.current_epoch + 1 if interval == "epoch" else self.global_step
            if counter % freq != 0:
                continue
            sch = s["scheduler"]
            if s.get("reduce_on_plateau"):
                key = s.get("monitor") or "val_loss"
                if key in self.callback_metrics:
                    sch.step(float(self.callback_metrics[key]))
            else:
                sch.step()
            if self._fused is not None and hasattr(self._fused, "on_lr_change"):
                self._fused.on_lr_change()

    # ---------------------------------------------------------------- state
    def _model_state_dict(self, model: LightningModule, staged: bool = False):
        if self._fused is not None:
            self._fused.sync_params_to_module()
        sd = dict(model.state_dict())
        return _Staged(sd) if staged else _to_cpu(sd)

    def _optimizer_state_dict(self, opt, staged: bool = False):
        if self._fused is not None and hasattr(self._fused, "optimizer_state_dict"):
            return self._fused.optimizer_state_dict()
        if hasattr(opt, "sync_host_state"):
            opt.sync_host_state()  # graph replays advance only the host group counters
        if (self._fused is not None and hasattr(self._fused, "sync_optimizer_state")
                and getattr(self, "_opt_state_synced_step", None) != self.global_step):
            # fused data-parallel step with the owner protocol: every element's Adam
            # state lives on its owner rank until consolidated (collective; every
            # rank dumps the checkpoint).  At validation ends it already ran on every
            # rank (_consolidate_optimizer_state): ModelCheckpoint's per-rank save
            # decision cannot strand a rank inside this collective.
            self._fused.sync_optimizer_state()
        sd = opt.state_dict()
        return _Staged(sd) if staged else _to_cpu(sd)

    def _consolidate_optimizer_state(self) -> None:
        """Validation end at world > 1: the owner-protocol Adam state is consolidated
        on EVERY rank before the checkpoint callbacks run (a collective at a point
        every rank reaches), so a checkpoint dump on only some ranks needs none."""
        if (getattr(self, "world_size", 1) > 1 and self._fused is not None
                and hasattr(self._fused, "sync_optimizer_state") and self.training
                and getattr(self, "_opt_state_synced_step", None) != self.global_step
                and any(hasattr(cb, "best_model_path") or "Checkpoint" in type(cb).__name__
                        for cb in self.callbacks)):
            self._fused.sync_optimizer_state()
            self._opt_state_synced_step = self.global_step

    # ------------------------------------------------- deferred checkpoints
    def deferred_checkpoints_ok(self) -> bool:
        """Whether ModelCheckpoint may hand its epoch-end save to the background
        (``_DeferredCheckpoints``): every rank of a GPU fit on the fused step whose
        checkpoint writer is configured (``RLA_DEFER_CKPT=0`` turns it off).  Rank 0
        stages the state on the device and decides / writes in the background; the
        other ranks stage nothing and write nothing (PL 1.1: only rank 0 saves), they
        only keep the top-k bookkeeping.  The owner-protocol consolidation -- the one
        collective a dump can need -- already ran on every rank at validation end
        (``_consolidate_optimizer_state``), so nothing here is collective."""
        if os.environ.get("RLA_DEFER_CKPT", "1") == "0" or not get_config().async_checkpoint:
            return False
        if not (self.on_gpu and torch.cuda.is_available()):
            return False
        # (without the writer process the background thread pickles the file itself)
        return self._fused is not None

    def defer_checkpoint(self, job, weights_only: bool, values=()):
        """Snapshot the checkpoint state ON THE DEVICE now (stream-ordered copies, no
        host sync) and queue ``job(resolve, values)`` for the background thread, which
        runs it once the device has produced that state: ``resolve()`` returns the
        host checkpoint dict, ``values`` (device scalars, e.g. the monitored metric)
        arrive as floats.  The training loop keeps dispatching meanwhile."""
        mark("ckpt_stage_begin")
        q = getattr(self, "_deferred", None)
        if q is None or q.closed:
            q = self._deferred = _DeferredCheckpoints()
        q.drain_done()  # earlier decisions (best model path / score) are in place
        # ranks > 0 never write a file: no device snapshot, no host copy
        ckpt = self.checkpoint_connector.dump_checkpoint(weights_only, staged=True) if self.is_global_zero else None
        vals = [v.detach().reshape(()).double().clone() if isinstance(v, torch.Tensor) and v.is_cuda else v
                for v in values]
        q.submit(ckpt, vals, job)
        mark("ckpt_staged")

    def wait_deferred(self) -> None:
        q = getattr(self, "_deferred", None)
        if q is not None:
            q.wait()

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_fused"] = None
        d["_log_sink"] = None
        d["_pending_log"] = None
        d["_ckpt_writer"] = None
        d["_deferred"] = None
        d["accelerator_backend"] = None
        return d


def _floats(metrics: Dict[str, Any]) -> Dict[str, float]:
    """Metric dict -> Python floats with ONE device->host transfer for the device values."""
    dev = [(k, v) for k, v in metrics.items() if isinstance(v, torch.Tensor) and v.is_cuda and v.numel() == 1]
    out = {k: float(v) for k, v in metrics.items() if not (isinstance(v, torch.Tensor) and v.is_cuda
                                                           and v.numel() == 1)}
    if dev:
        vals = torch.stack([v.detach().reshape(()).double() for _, v in dev]).cpu().tolist()
        out.update({k: x for (k, _), x in zip(dev, vals)})
    return {k: out[k] for k in metrics}


def _to_cpu(obj):
    """Host copy of a (nested) state dict.  Device tensors move in ONE transfer per
    dtype (flattened into a device buffer, copied, split into host views) instead of
    one blocking copy each: a checkpoint of the MNIST model was ~24 synchronous
    small copies, ResNet-50's ~800."""
    leaves: List[torch.Tensor] = []

    def collect(o):
        if isinstance(o, torch.Tensor):
            if o.device.type != "cpu" and o.numel() > 0:
                leaves.append(o)
        elif isinstance(o, dict):
            for v in o.values():
                collect(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                collect(v)

    collect(obj)
    host: Dict[int, torch.Tensor] = {}
    groups: Dict[tuple, List[torch.Tensor]] = {}
    for t in leaves:
        if id(t) not in host:
            host[id(t)] = None  # placeholder: de-duplicates a tensor referenced twice
            groups.setdefault((t.device, t.dtype), []).append(t)
    for (_, dtype), ts in groups.items():
        flat = torch.cat([t.detach().reshape(-1) for t in ts]).cpu() if len(ts) > 1 else \
            ts[0].detach().reshape(-1).cpu()
        off = 0
        for t in ts:
            n = t.numel()
            # each leaf gets its OWN storage (a host memcpy): a view would pickle the
            # whole flat buffer once per leaf (cloudpickle writes a view's storage,
            # torch.save dedups it) -- the worker -> driver state-dict return would
            # grow by a factor of the leaf count
            v = flat[off: off + n].view(t.shape)
            host[id(t)] = v.clone() if len(ts) > 1 else v
            off += n

    def rebuild(o):
        if isinstance(o, torch.Tensor):
            return host[id(o)] if id(o) in host else o.detach().cpu()
        if isinstance(o, dict):
            return {k: rebuild(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return type(o)(rebuild(v) for v in o)
        return o

    return rebuild(obj)


class _Staged:
    """A (nested) state dict whose device tensors were copied into device-side flat
    buffers (one per device / dtype, stream-ordered: no host sync) and whose host
    tensors were cloned, at staging time; :meth:`host` makes the host copy."""

    def __init__(self, obj):
        leaves: List[torch.Tensor] = []
        self._cpu: Dict[int, torch.Tensor] = {}

        def collect(o):
            if isinstance(o, torch.Tensor):
                if o.device.type != "cpu" and o.numel() > 0:
                    leaves.append(o)
                elif id(o) not in self._cpu:
                    self._cpu[id(o)] = o.detach().clone()  # e.g. Adam's step: changes in place
            elif isinstance(o, dict):
                for v in o.values():
                    collect(v)
            elif isinstance(o, (list, tuple)):
                for v in o:
                    collect(v)

        collect(obj)
        self._obj = obj
        seen: Dict[int, bool] = {}
        groups: Dict[tuple, List[torch.Tensor]] = {}
        for t in leaves:
            if id(t) not in seen:
                seen[id(t)] = True
                groups.setdefault((t.device, t.dtype), []).append(t)
        self._groups = [(ts, torch.cat([t.detach().reshape(-1) for t in ts]) if len(ts) > 1 else
                         ts[0].detach().reshape(-1).clone()) for ts in groups.values()]

    def host(self):
        host: Dict[int, torch.Tensor] = dict(self._cpu)
        for ts, flat in self._groups:
            hflat = flat.cpu()
            off = 0
            for t in ts:
                n = t.numel()
                host[id(t)] = hflat[off: off + n].view(t.shape).clone()  # own storage (see _to_cpu)
                off += n

        def rebuild(o):
            if isinstance(o, torch.Tensor):
                return host[id(o)] if id(o) in host else o.detach().cpu()
            if isinstance(o, dict):
                return {k: rebuild(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return type(o)(rebuild(v) for v in o)
            return o

        out = rebuild(self._obj)
        self._groups, self._obj = [], None
        return out


def _resolve_staged(o):
    if isinstance(o, _Staged):
        return o.host()
    if isinstance(o, dict):
        return {k: _resolve_staged(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_resolve_staged(v) for v in o]
    return o


class _DeferredCheckpoints:
    """One background thread that finishes staged checkpoint saves in order.

    The main thread stages the state on the device and records an event; the
    thread makes its device-to-host copies on its OWN stream after waiting for
    that event only -- so neither the copies nor the wait queue behind the next
    epoch's work the main thread keeps dispatching (on the default stream a D2H
    copy would wait for all of it), and the main thread never blocks at the epoch
    end.  ``job`` decides (ModelCheckpoint's top-k on the now-known metric), writes
    through the checkpoint writer process and removes superseded files, in
    submission order.  Errors re-raise on the next :meth:`wait` / ``drain_done``."""

    def __init__(self):
        import queue
        import threading

        self._q: "queue.Queue" = queue.Queue()
        self._err: Optional[BaseException] = None
        self._pending = 0
        self._cv = threading.Condition()
        self._stream = torch.cuda.Stream()
        self.closed = False
        self._t = threading.Thread(target=self._loop, name="rla-deferred-ckpt", daemon=True)
        self._t.start()

    def submit(self, ckpt, values, job) -> None:
        ev = torch.cuda.Event()
        ev.record()
        with self._cv:
            self._pending += 1
        self._q.put((ckpt, values, job, ev))

    def _loop(self) -> None:
        while True:
            item = self._q.get()
            if item is None:
                return
            ckpt, values, job, ev = item
            try:
                with torch.cuda.stream(self._stream):
                    self._stream.wait_event(ev)
                    vals = [float(v.cpu()) if isinstance(v, torch.Tensor) else v for v in values]
                    job(lambda: _resolve_staged(ckpt) if ckpt is not None else None, vals)
            except BaseException as e:  # surfaced on the main thread
                self._err = e
            finally:
                del ckpt, values, item
                with self._cv:
                    self._pending -= 1
                    self._cv.notify_all()

    def _raise(self) -> None:
        if self._err is not None:
            e, self._err = self._err, None
            raise RuntimeError(f"deferred checkpoint save failed: {e!r}") from e

    def drain_done(self) -> None:
        """Wait for the queued saves (their device state was produced long ago when
        the next one is staged: this returns at once in steady state)."""
        self.wait()

    def wait(self) -> None:
        with self._cv:
            while self._pending:
                self._cv.wait()
        self._raise()

    def close(self) -> None:
        """Finish the queued saves and end the thread (idempotent)."""
        if not self.closed:
            self.closed = True
            self._q.put(None)
            self._t.join()
        self._raise()
