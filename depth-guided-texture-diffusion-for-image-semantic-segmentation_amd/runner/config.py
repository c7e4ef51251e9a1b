"""Minimal config-driven runner for the keys the reference's YAML files use (config/sod.yml:1-104, config/cod.yml:1-143):
``train_cfg`` (by_epoch, max_epochs, val_interval), ``train_dataloader.batch_size``, ``model.type`` (+ kwargs the reference
ignores, cod.py:38-46), ``optim_wrapper`` (AdamW, ``paramwise_cfg.custom_keys`` lr_mult, bypass_duplicate, ``clip_grad`` by norm or by value),
``param_scheduler`` (CosineAnnealingLR by epoch), ``default_hooks.logger.interval`` / ``checkpoint.interval``,
``custom_hooks: our_init`` and ``EMAHook`` (validate and checkpoint with the moving average of the weights), ``*_dataloader.sampler`` (DefaultSampler), ``val_evaluator``, ``optim_wrapper.type: AmpOptimWrapper``
(= fp16 autocast + dynamic loss scaling when the runner is built with ``compute_dtype=torch.float16``).  The external nest/mmengine runner is out of scope; this is what drives the HIP-backed model from
the same file.  ``model:`` keys beyond ``type`` reach the model class as keyword arguments (``build_model``), so
``model: {type: cod, diffuser: {grid: 22, k: 5, max_step: 6}}`` selects a texture-diffuser configuration (keys ``grid``, ``k``, ``max_step``,
``latent_dim``; an unknown key is a TypeError) with no further runner code.  ``train_dataloader.dataset`` / ``val_dataloader.dataset`` bind through the same registry (runner/datasets.py: the reference's seven
folder datasets) in ``Runner.fit`` / ``Runner.validate_config``; ``train`` / ``validate`` still take any iterable of the dataset dict contract (runner/data.py)."""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, Iterable, Optional

import torch
import yaml

from .checkpoint import load_checkpoint_file, load_pretrained, save_checkpoint
from .data import DefaultSampler, DeviceLoader, batches
from .metrics import build_evaluators, check_score_size
from .predict import MapWriter, parse_save_maps
from .optim import EmaTorch, FlatAdamW, LossScaler, build_optimizer, clip_grad_torch, parse_clip_grad, parse_ema

MODEL_REGISTRY: Dict[str, Callable] = {}


def register_model(name: str):
    def deco(fn):
        MODEL_REGISTRY[name] = fn
        return fn
    return deco


def load_config(path_or_text: str) -> dict:
    text = open(path_or_text).read() if os.path.exists(path_or_text) else path_or_text
    return yaml.safe_load(text)


def build_model(cfg: dict, compute_dtype=torch.bfloat16):
    from ..nn import cod
    MODEL_REGISTRY.setdefault("cod", cod)
    mcfg = dict(cfg["model"])
    cls = MODEL_REGISTRY[mcfg.pop("type")]
    return cls(**mcfg, compute_dtype=compute_dtype)


def build_optim(cfg: dict, model: torch.nn.Module, capturable: bool = False):
    ow = cfg["optim_wrapper"]
    ocfg = dict(ow["optimizer"])
    assert ocfg.pop("type") == "AdamW", "the reference configs use AdamW (config/sod.yml:58-61)"
    keys = {k: float(v.get("lr_mult", 1.0)) for k, v in (ow.get("paramwise_cfg", {}).get("custom_keys") or {}).items()}
    return build_optimizer(model, lr=float(ocfg["lr"]), weight_decay=float(ocfg.get("weight_decay", 0.0)), custom_keys=keys,
                           fused=None, capturable=capturable)


class CosineByEpoch:
    """CosineAnnealingLR(by_epoch=True, T_max=max_epochs, eta_min=0) (config/sod.yml:78-81): lr_e = lr_0 * (1 + cos(pi e / T)) / 2."""

    def __init__(self, optimizer, t_max: int):
        self.opt, self.t_max, self.epoch = optimizer, int(t_max), 0
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])

    def _apply(self):
        f = 0.5 * (1.0 + math.cos(math.pi * min(self.epoch, self.t_max) / self.t_max))
        for g in self.opt.param_groups:
            g["lr"] = g["initial_lr"] * f

    def step(self):
        self.epoch += 1
        self._apply()

    def state_dict(self):
        return {"epoch": self.epoch, "t_max": self.t_max}

    def load_state_dict(self, sd):
        self.epoch, self.t_max = int(sd["epoch"]), int(sd["t_max"])
        self._apply()


def custom_keys_of(cfg: dict) -> Dict[str, float]:
    ow = cfg["optim_wrapper"]
    return {k: float(v.get("lr_mult", 1.0)) for k, v in (ow.get("paramwise_cfg", {}).get("custom_keys") or {}).items()}


class Runner:
    """Train / validate the HIP-backed model from the reference's YAML.  On the HIP device the optimizer is ``FlatAdamW`` over the
    gradient reducer's flat buckets (what bench.py measures); ``compute_dtype=torch.float16`` adds the dynamic ``LossScaler`` of
    the configs' ``AmpOptimWrapper``.  On CPU (gloo tests of the host logic) it is torch.optim.AdamW over the same groups."""

    def __init__(self, cfg: dict, device="cuda", compute_dtype=torch.bfloat16, work_dir="work_dir", log: Callable = print,
                 rank: int = 0, world: int = 1, seed: int = 0, sod_metrics: Optional[str] = None, score_size: Optional[str] = None):
        from ..dist import GradReducer, broadcast_parameters
        self.cfg, self.device, self.work_dir, self.log = cfg, device, work_dir, log
        self.rank, self.world, self.seed = rank, world, seed
        # val_cfg.save_maps: the defaults of predict_config (out_dir, normalize); a misspelt key or value fails here, before the model is built
        self.save_maps = parse_save_maps((cfg.get("val_cfg") or {}).get("save_maps"))
        # S/E/F-measure on the device (runner/sod_metrics.py) are opt-in: keyword, else val_cfg.sod_metrics, else "skip".  score_size:
        # keyword, else val_cfg.score_size, else "network"; "original" scores the bytes of ops.predict_maps against the GT at each
        # image's own size.  A bad value or combination fails here, before the model is built
        self.sod_metrics = sod_metrics or (cfg.get("val_cfg") or {}).get("sod_metrics") or "skip"
        self.score_size = check_score_size(score_size or (cfg.get("val_cfg") or {}).get("score_size"), self.sod_metrics, cfg.get("val_evaluator"))
        self.model = build_model(cfg, compute_dtype).to(device)
        if any(h.get("type") == "our_init" for h in cfg.get("custom_hooks") or []):
            have = [p for p in ("pretrain/pvt_v2_b2.pth", "pretrain/convnext_base_22k_224.pth") if os.path.exists(p)]
            if len(have) == 2:
                self.log(load_pretrained(self.model))
            else:
                self.log("our_init: pretrain/*.pth not found, keeping the random initialisation")
        broadcast_parameters(self.model)
        self.reducer = GradReducer(self.model, working_dtype=compute_dtype)
        ow = cfg["optim_wrapper"]
        ocfg = dict(ow["optimizer"])
        assert ocfg.get("type") == "AdamW", "the reference configs use AdamW (config/sod.yml:58-61)"
        on_gpu = torch.device(device).type == "cuda"
        self.scaler = None
        # optim_wrapper.clip_grad (config/cod.yml:108-110): inside FlatAdamW on the HIP device, torch's utilities before torch.optim.AdamW on CPU
        self.clip_grad = parse_clip_grad(ow.get("clip_grad"))
        self._grad_norm = None
        # custom_hooks: EMAHook (mmengine): train with the raw weights, validate and checkpoint with their moving average.  Inside
        # FlatAdamW on the HIP device, EmaTorch beside torch.optim.AdamW on CPU; self.ema is whichever carries it, or None without the hook
        ema_hooks = [h for h in cfg.get("custom_hooks") or [] if h.get("type") == "EMAHook"]
        if len(ema_hooks) > 1:
            raise ValueError("custom_hooks holds more than one EMAHook")
        self.ema_cfg = parse_ema(ema_hooks[0]) if ema_hooks else None
        self.ema = None
        if on_gpu:
            if compute_dtype == torch.float16:
                assert ow.get("type") == "AmpOptimWrapper", "fp16 compute needs the AmpOptimWrapper recipe (loss scaling)"
                self.scaler = LossScaler(device)
            self.optimizer = FlatAdamW(self.reducer, lr=float(ocfg["lr"]), weight_decay=float(ocfg.get("weight_decay", 0.0)),
                                       custom_keys=custom_keys_of(cfg), scaler=self.scaler, clip_grad=self.clip_grad, ema=ema_hooks[0] if ema_hooks else None, module=self.model)
            self.ema = self.optimizer if self.ema_cfg is not None else None
        else:
            self.optimizer = build_optim(cfg, self.model)
            self.ema = EmaTorch(self.model, ema_hooks[0]) if ema_hooks else None
        tc = cfg["train_cfg"]
        self.max_epochs = int(tc["max_epochs"])
        self.val_interval = int(tc.get("val_interval", 0) or 0)
        ps = cfg.get("param_scheduler") or {}
        self.scheduler = CosineByEpoch(self.optimizer, int(ps.get("T_max", self.max_epochs))) if ps.get("type") == "CosineAnnealingLR" else None
        hooks = cfg.get("default_hooks") or {}
        self.log_interval = int((hooks.get("logger") or {}).get("interval", 50))
        self.ckpt_interval = int((hooks.get("checkpoint") or {}).get("interval", 1))
        self.evaluators = build_evaluators(cfg.get("val_evaluator"), log, sod_metrics=self.sod_metrics, score_size=self.score_size)
        self.epoch = 0
        self._device_loaders: Dict[tuple, DeviceLoader] = {}     # one per (dataset, split): staging buffers and decode threads persist over the epochs
        self._ema_gate()

    # ------------------------------------------------------------------ EMA of the weights
    def _ema_gate(self) -> None:
        """``begin_epoch``: until then the average stays a copy of the weights (the flag travels to the device with the next step)."""
        if self.ema is not None and self.ema_cfg["begin_epoch"]:
            self.ema.set_ema_enabled(self.epoch >= self.ema_cfg["begin_epoch"])

    def swap_ema(self) -> None:
        """Exchange the model's weights with their average, in place (and back with a second call)."""
        self.ema.swap_ema()
        if not isinstance(self.optimizer, FlatAdamW):
            self.reducer.refresh_working()

    def _ema_by_key(self) -> Dict[str, torch.Tensor]:
        """The averages under every state_dict key they stand for (a shared parameter is averaged once, under its first name)."""
        avg, first, alias = self.ema.ema_tensors(), {}, {}
        for n, p in self.model.named_parameters(remove_duplicate=False):
            alias[n] = first.setdefault(id(p), n)
        return {k: avg[alias.get(k, k)] for k in self.model.state_dict() if alias.get(k, k) in avg}

    # ------------------------------------------------------------------ data
    def build_dataset(self, split: str = "train"):
        """``cfg['<split>_dataloader']['dataset']`` through the ``@export`` registry (runner/datasets.py holds the reference's seven
        classes; ``SyntheticRGBD`` registers the same way).  An unknown ``type`` raises and lists the registered names."""
        from .registry import build
        block = (self.cfg.get(f"{split}_dataloader") or {}).get("dataset")
        if not block or "type" not in block:
            raise KeyError(f"the config has no {split}_dataloader.dataset block with a type")
        ds = build(block)
        if hasattr(ds, "decode"):
            ds.seed = self.seed              # the flip coin is a function of (seed, epoch, index), the same on every rank
        return ds

    def model_img_size(self) -> Optional[int]:
        """``model.img_size`` of the YAML, else the model's ``img_size`` attribute; None when neither says."""
        v = (self.cfg.get("model") or {}).get("img_size", getattr(self.model, "img_size", None))
        return None if v is None else int(v)

    def check_dataset_size(self, dataset, split: str) -> None:
        have, want = getattr(dataset, "image_size", getattr(dataset, "size", None)), self.model_img_size()
        if have is not None and want is not None and int(have) != want:
            raise ValueError(f"{split}_dataloader.dataset yields {have}x{have} images but model.img_size is {want}")

    def loader(self, dataset, split: str = "train", epoch: int = 0, with_sizes: bool = False, with_gt8: bool = False):
        """Batches of ``dataset`` the way the YAML's ``<split>_dataloader`` asks: batch_size, DefaultSampler(shuffle) partitioned
        ``rank::world`` over a per-epoch seeded permutation.  A dataset with ``decode`` (runner/datasets.py) on the HIP device goes
        through ``DeviceLoader`` (one upload and three launches per batch, ``num_workers`` decode threads, stacked fp32 tensors);
        everything else through ``batches`` (lists of per-sample tensors from the dataset's own ``__getitem__``).  ``with_sizes``: the
        ``DeviceLoader`` batches also carry each sample's original ``(H, W)`` under ``'size'`` (``predict`` writes maps at that size);
        ``with_gt8``: also the packed GT planes at their own size under ``'gt8'`` (``score_size: original`` scores against them)."""
        dl = self.cfg.get(f"{split}_dataloader") or {}
        sc = dl.get("sampler") or {}
        sampler = DefaultSampler(len(dataset), shuffle=bool(sc.get("shuffle", split == "train")), seed=self.seed, rank=self.rank, world=self.world)
        sampler.set_epoch(epoch)
        if callable(getattr(dataset, "set_epoch", None)):
            dataset.set_epoch(epoch)
        batch_size, workers = int(dl.get("batch_size", 1)), int(dl.get("num_workers", 8))
        if hasattr(dataset, "decode") and torch.device(self.device).type == "cuda":
            # one loader per (dataset, split) over the epochs: its staging buffers and decode threads persist; ``close()`` ends them
            key, made_with = (id(dataset), split), (batch_size, workers)
            dev = self._device_loaders.get(key)
            if dev is not None and (dev.dataset is not dataset or dev.made_with != made_with):     # the YAML block changed since
                dev.close()
                dev = None
            if dev is None:
                dev = self._device_loaders[key] = DeviceLoader(dataset, sampler, batch_size, self.device, torch.float32, workers)
                dev.made_with = made_with
            dev.sampler, dev.with_gt8 = sampler, bool(with_gt8)
            dev.with_sizes = bool(with_sizes) or dev.with_gt8
            return dev
        return batches(dataset, sampler, batch_size, self.device)

    def close(self) -> None:
        """Stop the decode threads of every ``DeviceLoader`` that ``loader`` made and drop them (``fit`` and ``validate_config`` do
        this when they return; a caller that drives ``train`` / ``validate`` with ``loader`` itself calls it when done)."""
        for dev in self._device_loaders.values():
            dev.close()
        self._device_loaders.clear()

    def fit(self):
        """``script/train.sh``: build the train dataset (and the val dataset when ``val_interval`` is set) from the YAML and run
        ``train`` over them.  A dataset whose size differs from the model's ``img_size`` raises before the first step."""
        train_ds = self.build_dataset("train")
        self.check_dataset_size(train_ds, "train")
        val_ds = None
        if self.val_interval and (self.cfg.get("val_dataloader") or {}).get("dataset"):
            val_ds = self.build_dataset("val")
            self.check_dataset_size(val_ds, "val")
        try:
            return self.train(lambda epoch: self.loader(train_ds, "train", epoch),
                              val_loader_fn=None if val_ds is None else (lambda: self.loader(val_ds, "val")))
        finally:
            self.close()

    def validate_config(self, split: str = "val") -> Dict[str, float]:
        """``script/test.sh`` (``-m val``): build ``<split>_dataloader.dataset`` from the YAML and ``validate`` over it.  With
        ``score_size: original`` the loader also delivers the GT planes at their own size, and when ``val_cfg.save_maps.out_dir`` is
        set the same pass writes the scored bytes as PNGs there (one ``ops.predict_maps`` per batch serves both)."""
        ds = self.build_dataset(split)
        self.check_dataset_size(ds, split)
        original = self.score_size == "original"
        writer = None
        if original and self.save_maps and self.save_maps["out_dir"] is not None:
            writer = MapWriter(self.save_maps["out_dir"], minmax=self.save_maps["minmax"])
        try:
            return self.validate(self.loader(ds, split, with_gt8=original), writer=writer)
        finally:
            try:
                if writer is not None:
                    writer.close()
            finally:
                self.close()

    # ------------------------------------------------------------------ train
    def train_step(self, batch: dict) -> torch.Tensor:
        self.reducer.zero_grad()
        loss = self.model(batch.get("raw"), batch["input"], batch["label"], batch["depth"], mode="loss")["loss"]
        (self.scaler.scale(loss) if self.scaler is not None else loss).backward()
        self.reducer.finish()
        if self.clip_grad is not None and not isinstance(self.optimizer, FlatAdamW):
            self._grad_norm = clip_grad_torch((p for g in self.optimizer.param_groups for p in g["params"]), self.clip_grad)
        if self.ema is self.optimizer:
            self.optimizer.sync_ema()
        self.optimizer.step()
        if not isinstance(self.optimizer, FlatAdamW):
            self.reducer.refresh_working()
            if self.ema is not None:
                self.ema.update()
        return loss

    def grad_norm(self):
        """Clip by norm: the total gradient norm of the last step (a host read on the HIP device); ``None`` otherwise."""
        if isinstance(self.optimizer, FlatAdamW):
            return self.optimizer.grad_norm()
        return None if self._grad_norm is None else float(self._grad_norm)

    def train(self, loader_fn: Callable[[int], Iterable[dict]], epochs: Optional[int] = None, val_loader_fn: Optional[Callable[[], Iterable[dict]]] = None):
        """Epochs ``self.epoch .. (epochs or max_epochs)``: the loop the reference gets from mmengine's EpochBasedTrainLoop
        (logger / checkpoint hooks by their intervals, scheduler per epoch, validation every ``val_interval`` epochs)."""
        losses = []
        for epoch in range(self.epoch, epochs or self.max_epochs):
            self.model.train()
            self._ema_gate()
            for it, batch in enumerate(loader_fn(epoch)):
                loss = self.train_step(batch)
                losses.append(loss.detach())
                if (it + 1) % self.log_interval == 0:
                    line = f"epoch {epoch + 1} iter {it + 1} loss {loss.item():.4f} lr {self.optimizer.param_groups[0]['lr']:.3e}"
                    if self.clip_grad is not None and self.clip_grad["type"] == "norm":      # mmengine logs it too; read only here
                        line += f" grad_norm {self.grad_norm():.4f}"
                    self.log(line)
            if self.scheduler is not None:
                self.scheduler.step()
            self.epoch = epoch + 1
            if self.epoch % self.ckpt_interval == 0 and self.rank == 0:
                self.save(os.path.join(self.work_dir, f"epoch_{self.epoch}.pth"))
            if val_loader_fn is not None and self.val_interval and self.epoch % self.val_interval == 0:
                self.log(f"epoch {self.epoch} val {self.validate(val_loader_fn())}")
        return [float(l) for l in losses]

    # ------------------------------------------------------------------ val (script/test.sh: `-m val`)
    @torch.no_grad()
    def validate(self, loader: Iterable[dict], writer: Optional[MapWriter] = None) -> Dict[str, float]:
        """val_step = ``cod.forward(mode='predict')`` (cod.py:152-153, :219) per batch -> every evaluator's ``process`` ->
        ``compute_metrics`` (mmengine ValLoop + Evaluator).  With ``score_size: original`` the step is ``cod.forward(mode='tensor')``
        -> ``ops.predict_maps`` at ``batch['size']`` -> every evaluator's ``process(batch, ops.RaggedMaps)`` with ``batch['gt8']``: the
        bytes a PNG would hold, against the GT at its own size; ``writer`` (a ``MapWriter``) then receives those same bytes."""
        was_training = self.model.training
        self.model.eval()
        for ev in self.evaluators:
            ev.results.clear()
            ev.__dict__.pop("_all", None)
            if callable(getattr(ev, "reset", None)):
                ev.reset()
        if self.ema is not None:          # EMAHook.before_val_epoch / after_val_epoch: validate with the averaged weights
            self.swap_ema()
        try:
            for batch in loader:
                if self.score_size == "original":
                    out = self._original_size_maps(batch, writer)
                else:
                    out = self.model(batch.get("raw"), batch["input"], batch["label"], batch["depth"], mode="predict")
                for ev in self.evaluators:
                    ev.process(batch, out)
        finally:
            if self.ema is not None:
                self.swap_ema()
        self.model.train(was_training)
        metrics = {}
        for ev in self.evaluators:
            metrics.update(ev.compute_metrics())
        return metrics

    def _original_size_maps(self, batch: dict, writer: Optional[MapWriter]):
        from .. import ops
        if not isinstance(batch, dict) or batch.get("gt8") is None or batch.get("size") is None:
            raise ValueError("score_size: original needs batches with 'gt8' and 'size': build the loader with DeviceLoader(with_gt8=True) "
                             "(Runner.loader(..., with_gt8=True))")
        logits = self.model(batch.get("raw"), batch["input"], batch["label"], batch["depth"], mode="tensor")
        sizes = [tuple(int(v) for v in hw) for hw in batch["size"]]
        packed, offsets = ops.predict_maps(logits, sizes, minmax=bool(self.save_maps and self.save_maps["minmax"]))
        if writer is not None:
            writer.submit(batch, logits, packed=(packed, offsets))
        return ops.RaggedMaps(packed, batch["gt8"], sizes, offsets)

    # ------------------------------------------------------------------ prediction maps (script/test.sh's PNG side effect)
    @torch.no_grad()
    def predict(self, loader: Iterable[dict], out_dir: str, minmax: bool = False) -> list:
        """One grey-level PNG per sample of ``loader`` under ``out_dir``, named by the stem of ``raw``, at the sample's own size
        (``batch['size']``, else the model's): ``cod.forward(mode='tensor')`` per batch -> ``runner.predict.MapWriter`` (one launch and
        one device-to-host copy per batch, the encode overlapping the next forward).  Eval mode, and the averaged weights when EMAHook
        is configured, exactly as ``validate``.  Returns the written paths, in order."""
        was_training = self.model.training
        self.model.eval()
        if self.ema is not None:
            self.swap_ema()
        writer = MapWriter(out_dir, minmax=minmax)
        try:
            for batch in loader:
                writer.submit(batch, self.model(batch.get("raw"), batch["input"], batch["label"], batch["depth"], mode="tensor"))
        finally:
            try:
                paths = writer.close()
            finally:
                if self.ema is not None:
                    self.swap_ema()
                self.model.train(was_training)
        return paths

    def predict_config(self, split: str = "val", out_dir: Optional[str] = None, minmax: Optional[bool] = None) -> list:
        """Build ``<split>_dataloader.dataset`` from the YAML and ``predict`` over it.  ``out_dir`` and ``minmax`` default to
        ``val_cfg: {save_maps: {out_dir: ..., normalize: none | minmax}}``."""
        defaults = self.save_maps or {"out_dir": None, "minmax": False}
        out_dir = defaults["out_dir"] if out_dir is None else out_dir
        if out_dir is None:
            raise ValueError("predict_config needs out_dir, as an argument or as val_cfg.save_maps.out_dir")
        ds = self.build_dataset(split)
        self.check_dataset_size(ds, split)
        try:
            return self.predict(self.loader(ds, split, with_sizes=True), out_dir, defaults["minmax"] if minmax is None else bool(minmax))
        finally:
            self.close()

    # ------------------------------------------------------------------ checkpoint / resume
    def save(self, path: str) -> None:
        if self.ema is None:
            save_checkpoint(self.model, path, self.optimizer, [self.scheduler] if self.scheduler else None, {"epoch": self.epoch})
            return
        # EMAHook.before_save_checkpoint: ``state_dict`` carries the AVERAGED weights (what our_init.before_val and every plain loader
        # read), ``ema_state_dict`` the raw ones under ``module.*`` plus ``steps``
        save_checkpoint(self.model, path, self.optimizer, [self.scheduler] if self.scheduler else None,
                        {"epoch": self.epoch, "iter": self.ema.ema_iters}, ema=(self._ema_by_key(), self.ema.ema_steps))

    def resume(self, path: str) -> None:
        """Continue a run: weights (the reducer's load hooks refresh the working copies), optimizer state (moments, step, loss
        scale), scheduler and epoch.  With EMAHook the two entries of the file are exchanged back: ``ema_state_dict`` (raw) goes into
        the model, ``state_dict`` into the average; a file without ``ema_state_dict`` starts the average from its ``state_dict``
        (``strict_load``: raises)."""
        ckpt = load_checkpoint_file(path, weights_only=False)
        if self.ema is None:
            self.model.load_state_dict(ckpt["state_dict"], strict=True)
        else:
            sd, esd = ckpt["state_dict"], ckpt.get("ema_state_dict")
            iters = int((ckpt.get("meta") or {}).get("iter", 0))
            if esd is None:
                if self.ema_cfg["strict_load"]:
                    raise KeyError(f"{path} has no ema_state_dict (EMAHook strict_load)")
                self.model.load_state_dict(sd, strict=True)
                self.ema.load_ema(None, 0, iters)
            else:
                self.model.load_state_dict({k: esd["module." + k] for k in sd}, strict=True)
                self.ema.load_ema(sd, int(esd["steps"]), iters)
        if "optimizer" in ckpt:
            self.optimizer.load_state_dict(ckpt["optimizer"])
        if self.scheduler is not None and ckpt.get("param_schedulers"):
            self.scheduler.load_state_dict(ckpt["param_schedulers"][0])
        self.epoch = int((ckpt.get("meta") or {}).get("epoch", 0))
        self._ema_gate()
