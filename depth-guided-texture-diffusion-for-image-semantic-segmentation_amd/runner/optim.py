"""AdamW with the reference's per-prefix learning-rate multipliers (config/sod.yml:56-76, config/cod.yml):
mmengine's ``paramwise_cfg.custom_keys`` semantics = the LONGEST matching substring key wins;
``bypass_duplicate`` = a parameter reachable under several names (the shared PReLU) is added once."""
from __future__ import annotations

import math
import os
from typing import Dict, Iterable, Optional

import torch

SOD_CUSTOM_KEYS: Dict[str, float] = {
    "hitnet.backbone": 0.2,
    "hitnet.backbone.prompt_encoder.encoder2.downsample_layers": 0.02,
    "hitnet.backbone.prompt_encoder.encoder2.stages.0": 0.02,
    "hitnet.backbone.prompt_encoder.encoder2.stages.1": 0.02,
    "hitnet.backbone.prompt_encoder.encoder2.stages.2": 0.02,
    "hitnet.backbone.prompt_encoder.encoder2.stages.3": 0.02,
}


def lr_mult_for(name: str, custom_keys: Dict[str, float]) -> float:
    best, mult = -1, 1.0
    for key, m in custom_keys.items():
        if key in name and len(key) > best:
            best, mult = len(key), m
    return mult


def build_optimizer(model: torch.nn.Module, lr: float = 5e-4, weight_decay: float = 0.1,
                    custom_keys: Optional[Dict[str, float]] = None, fused: Optional[bool] = None,
                    capturable: bool = False):
    custom_keys = SOD_CUSTOM_KEYS if custom_keys is None else custom_keys
    groups: Dict[float, list] = {}
    seen = set()
    for name, p in model.named_parameters(remove_duplicate=False):
        if id(p) in seen:   # bypass_duplicate; masters whose compute runs on a working copy have requires_grad=False
            continue
        seen.add(id(p))
        groups.setdefault(lr_mult_for(name, custom_keys), []).append(p)
    param_groups = [{"params": ps, "lr": lr * m, "initial_lr": lr * m} for m, ps in sorted(groups.items(), reverse=True)]
    if fused is None:
        fused = any(p.is_cuda for g in param_groups for p in g["params"])
    return torch.optim.AdamW(param_groups, lr=lr, weight_decay=weight_decay, fused=fused, capturable=capturable and fused)


def parse_clip_grad(clip_grad: Optional[dict]) -> Optional[dict]:
    """``optim_wrapper.clip_grad`` in mmengine's spellings (OptimWrapper, config/cod.yml:108-110) -> a normal form, or ValueError:
    ``{"max_norm": x, "norm_type": 2 | "inf"}`` (optionally ``"type": "norm"``) -> ``{"type": "norm", "max_norm": x, "norm_type": 2.0 | inf}``;
    ``{"type": "value", "clip_value": x}`` -> ``{"type": "value", "clip_value": x}``; ``None`` (key absent) -> ``None``."""
    if clip_grad is None:
        return None
    if not isinstance(clip_grad, dict) or not clip_grad:
        raise ValueError(f"clip_grad must be a non-empty dict, got {clip_grad!r}")
    kind = clip_grad.get("type", "norm")
    if kind not in ("norm", "value"):
        raise ValueError(f"clip_grad.type must be 'norm' or 'value', got {kind!r}")
    if "max_norm" in clip_grad and "clip_value" in clip_grad:
        raise ValueError("clip_grad: max_norm (clip by norm) and clip_value (clip by value) exclude each other")
    allowed = {"type", "max_norm", "norm_type"} if kind == "norm" else {"type", "clip_value"}
    extra = set(clip_grad) - allowed
    if extra:
        raise ValueError(f"clip_grad of type {kind!r} does not take {sorted(extra)}")
    key = "max_norm" if kind == "norm" else "clip_value"
    if key not in clip_grad:
        raise ValueError(f"clip_grad of type {kind!r} needs {key}")

    def bound(v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v > 0) or math.isinf(v):
            raise ValueError(f"clip_grad.{key} must be a positive finite number, got {v!r}")
        return float(v)
    if kind == "value":
        return {"type": "value", "clip_value": bound(clip_grad["clip_value"])}
    nt = clip_grad.get("norm_type", 2)
    if isinstance(nt, str):
        nt = math.inf if nt == "inf" else None
    if isinstance(nt, bool) or not isinstance(nt, (int, float)) or float(nt) not in (2.0, math.inf):
        raise ValueError(f"clip_grad.norm_type must be 2 or 'inf', got {clip_grad.get('norm_type')!r}")
    return {"type": "norm", "max_norm": bound(clip_grad["max_norm"]), "norm_type": float(nt)}


def clip_grad_torch(params: Iterable[torch.Tensor], clip_grad: Optional[dict]) -> Optional[torch.Tensor]:
    """The CPU path (torch.optim.AdamW): ``clip_grad`` applied with torch's own utilities to the parameters that have a gradient.
    Returns the total norm (clip by norm) or ``None``."""
    cg = parse_clip_grad(clip_grad)
    if cg is None:
        return None
    params = [p for p in params if p.grad is not None]
    if cg["type"] == "norm":
        return torch.nn.utils.clip_grad_norm_(params, cg["max_norm"], norm_type=cg["norm_type"])
    torch.nn.utils.clip_grad_value_(params, cg["clip_value"])
    return None


EMA_TYPES = ("ExponentialMovingAverage", "MomentumAnnealingEMA", "StochasticWeightAverage")      # kind 0, 1, 2 of dgtd_ema_schedule


def parse_ema(ema: Optional[dict]) -> Optional[dict]:
    """mmengine's ``EMAHook`` entry of ``custom_hooks`` (or the same keys without ``type``) -> a normal form with every key present, or
    ValueError; ``None`` -> ``None``.  Keys: ``ema_type`` (one of ``EMA_TYPES``), ``momentum`` in (0, 1), ``gamma`` > 0 (only with
    MomentumAnnealingEMA), ``interval`` >= 1, ``update_buffers``, ``begin_iter`` >= 0, ``begin_epoch`` >= 0 (not both non-zero),
    ``strict_load``; ``type`` (must be EMAHook) and ``priority`` are the hook's own and carry nothing."""
    if ema is None:
        return None
    if not isinstance(ema, dict):
        raise ValueError(f"ema must be a dict, got {ema!r}")
    if ema.get("type", "EMAHook") != "EMAHook":
        raise ValueError(f"ema.type must be 'EMAHook', got {ema.get('type')!r}")
    extra = set(ema) - {"type", "priority", "ema_type", "momentum", "gamma", "interval", "update_buffers", "begin_iter", "begin_epoch", "strict_load"}
    if extra:
        raise ValueError(f"EMAHook does not take {sorted(extra)}")
    ema_type = ema.get("ema_type", EMA_TYPES[0])
    if ema_type not in EMA_TYPES:
        raise ValueError(f"ema.ema_type must be one of {EMA_TYPES}, got {ema_type!r}")

    def number(key, default, ok, what, integer=False):
        v = ema.get(key, default)
        if isinstance(v, bool) or not isinstance(v, int if integer else (int, float)) or not ok(v):
            raise ValueError(f"ema.{key} must be {what}, got {v!r}")
        return int(v) if integer else float(v)

    def flag(key):
        v = ema.get(key, False)
        if not isinstance(v, bool):
            raise ValueError(f"ema.{key} must be true or false, got {v!r}")
        return v
    if "gamma" in ema and ema_type != "MomentumAnnealingEMA":
        raise ValueError(f"ema.gamma belongs to MomentumAnnealingEMA, not to {ema_type}")
    out = {"ema_type": ema_type, "kind": EMA_TYPES.index(ema_type),
           "momentum": number("momentum", 0.0002, lambda v: 0.0 < v < 1.0, "in (0, 1)"),
           "gamma": number("gamma", 100, lambda v: v > 0 and not math.isinf(v), "a positive finite number"),
           "interval": number("interval", 1, lambda v: v >= 1, "an integer >= 1", integer=True),
           "update_buffers": flag("update_buffers"),
           "begin_iter": number("begin_iter", 0, lambda v: v >= 0, "an integer >= 0", integer=True),
           "begin_epoch": number("begin_epoch", 0, lambda v: v >= 0, "an integer >= 0", integer=True),
           "strict_load": flag("strict_load")}
    if out["begin_iter"] and out["begin_epoch"]:
        raise ValueError("ema: begin_iter and begin_epoch exclude each other")
    return out


def ema_coefficient(cfg: dict, steps: int) -> float:
    """``c(kind, steps)`` of the schedule: the weight of the current parameters in the update that follows ``steps`` counted ones."""
    if cfg["kind"] == 0:
        return cfg["momentum"]
    if cfg["kind"] == 1:
        return max(cfg["momentum"], cfg["gamma"] / (cfg["gamma"] + steps))
    return 1.0 / (steps // cfg["interval"] + 1)


class EmaTorch:
    """The CPU path of ``EMAHook`` (beside torch.optim.AdamW): the schedule of ``dgtd_ema_schedule`` on the host and the update
    ``e += c (p - e)`` in torch ops, over the parameters of ``model`` (shared ones once) and - ``update_buffers`` - its float buffers.
    Same surface as ``FlatAdamW(ema=...)``: ``update()`` once per iteration, ``ema_steps``, ``swap_ema()``, ``ema_tensors()``, ``load_ema()``."""

    def __init__(self, model: Optional[torch.nn.Module], ema: dict):
        self.ema = parse_ema(ema)
        if self.ema is None:
            raise ValueError("EmaTorch needs an EMAHook configuration")
        self.coef, self.steps, self.iters, self.enabled = 1.0, 0, 0, True
        self.live: Dict[str, torch.Tensor] = {}
        if model is not None:
            seen = set()
            for n, p in model.named_parameters():
                if id(p) not in seen:
                    seen.add(id(p))
                    self.live[n] = p
            if self.ema["update_buffers"]:
                self.live.update({n: b for n, b in model.named_buffers() if b.is_floating_point()})
        self.avg = {n: t.detach().clone() for n, t in self.live.items()}

    def schedule(self) -> float:
        """One iteration of the table in include/dgtd.h; returns (and keeps) the coefficient."""
        c = 1.0
        if self.enabled and self.iters >= self.ema["begin_iter"]:
            k = self.steps
            c = 1.0 if k == 0 else (ema_coefficient(self.ema, k) if k % self.ema["interval"] == 0 else 0.0)
            self.steps += 1
        self.iters += 1
        self.coef = c
        return c

    @torch.no_grad()
    def update(self) -> None:
        c = self.schedule()
        if c == 0.0:
            return
        for n, p in self.live.items():
            e = self.avg[n]
            if c == 1.0:
                e.copy_(p)
            else:
                e.add_(p.detach() - e, alpha=c)

    @property
    def ema_steps(self) -> int:
        return self.steps

    @property
    def ema_iters(self) -> int:
        return self.iters

    def set_ema_enabled(self, on: bool) -> None:
        self.enabled = bool(on)

    @torch.no_grad()
    def swap_ema(self) -> None:
        for n, p in self.live.items():
            t = p.detach().clone()
            p.copy_(self.avg[n])
            self.avg[n].copy_(t)

    def ema_tensors(self) -> Dict[str, torch.Tensor]:
        return dict(self.avg)

    @torch.no_grad()
    def load_ema(self, named: Optional[dict], steps: int = 0, iters: int = 0) -> None:
        """``named`` = averaged tensors by state_dict key (others are ignored), or ``None``: the average restarts as a copy of the weights."""
        for n, e in self.avg.items():
            e.copy_(self.live[n] if named is None else named[n])
        self.steps, self.iters = int(steps), int(iters)


class LossScaler:
    """Dynamic loss scaling with torch.amp.GradScaler's rule (the reference's AmpOptimWrapper, config/sod.yml:57): the loss is
    multiplied by ``scale``; a step whose gradients hold an inf / NaN is skipped and halves the scale, ``growth_interval`` clean
    steps in a row double it.  All state lives on the device (``state`` = [scale, growth_tracker, 1/scale, found_inf, optimizer
    steps actually taken]) and is updated by ``dgtd_loss_scale_update``: no host synchronisation per step."""

    def __init__(self, device, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, int(growth_interval)
        self.state = torch.tensor([init_scale, 0.0, 1.0 / init_scale, 0.0, 0.0], dtype=torch.float32, device=device)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.state[0]

    def get_scale(self) -> float:
        return float(self.state[0].item())

    def state_dict(self) -> dict:
        st = self.state.tolist()
        return {"scale": st[0], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(st[1]), "steps_taken": int(st[4])}

    def load_state_dict(self, sd: dict) -> None:
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self.state.copy_(torch.tensor([sd["scale"], float(sd["_growth_tracker"]), 1.0 / sd["scale"], 0.0, float(sd.get("steps_taken", 0))]))


_ADAM_G16 = os.environ.get("DGTD_ADAM_G16", "1") != "0"      # 0: always widen the 16-bit all-reduce payload into the fp32 bucket first


class FlatAdamW:
    """AdamW over the flat buckets of a ``dist.GradReducer``: one ``dgtd_adamw_flat`` launch per run of equal learning rate per
    bucket (≈ 20 launches for 114 M parameters) that also rewrites the 16-bit working copies, instead of torch's multi-tensor AdamW
    plus one cast per bucket.  Same update rule and defaults as ``torch.optim.AdamW``; ``param_groups`` carries one entry per
    distinct lr multiplier so the reference's epoch-wise cosine schedule (config/sod.yml:78-83) drives it unchanged.
    ``scaler``: a ``LossScaler`` (fp16 mode): the gradients are checked for inf / NaN (one pass per bucket), un-scaled inside
    the AdamW launch, and an overflowed step is skipped on the device.
    ``state_dict()`` has torch.optim.AdamW's layout (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` in the parameters'
    logical shapes, ``param_groups`` with parameter indices, plus ``param_names``), whatever the bucket size was.
    ``clip_grad``: mmengine's ``optim_wrapper.clip_grad`` (see ``parse_clip_grad``), on the device and capturable.
    Clip by norm: one ``dgtd_grad_norm_partial`` launch per run AdamW will update, over the operand AdamW will read (the 16-bit payload
    where the direct path applies, the fp32 bucket elsewhere; slots without a gradient and the alignment padding are zero), one
    ``dgtd_grad_clip_finalize`` that leaves { total norm, coefficient } in device memory, then the AdamW launches, which multiply by the
    coefficient.  With a ``scaler`` the norm pass IS the inf / NaN check (the finalize raises ``found_inf``): ``dgtd_found_inf`` is not
    launched.  A global norm needs every bucket: under ``pipelined`` each bucket's norm launch still waits for that bucket's all-reduce
    only, but the finalize and with it every AdamW launch come after the last bucket, so AdamW of the first buckets no longer overlaps
    the later all-reduces.  All-reduced gradients are identical on every rank, so the norm needs no collective of its own.
    Clip by value: only an argument of the AdamW launches changes.
    ``ema``: mmengine's ``EMAHook`` (see ``parse_ema``): an exponential moving average of the masters in one flat fp32 buffer per bucket
    (``ema_bufs``, +4 B/parameter), updated inside the AdamW launches (``dgtd_adamw_flat_ema``) with the coefficient ``dgtd_ema_schedule``
    leaves in ``ema_state`` (device, { coef, steps, iters, enabled }) once per step: nothing of it is a host value, so the captured step
    replays it.  Stretches AdamW does not visit (world 1: slots without a gradient) get ``dgtd_ema_flat``, so every element of every
    average sees exactly one update per step; an overflowed fp16 step still updates the average (against the unchanged masters).
    ``update_buffers``: the float buffers of ``module`` (the model the reducer was built over; required then, and only its buffer
    tensors are kept: the model's leaves hold the reducer through autograd hooks the cycle collector cannot see, so a reference back
    to the model would keep both alive) are averaged too, one ``dgtd_ema_flat`` each; otherwise the averaged model shares the live
    buffers.  ``swap_ema()`` exchanges masters and averages in place (working copies rewritten)."""

    def __init__(self, reducer, lr: float = 5e-4, weight_decay: float = 0.1, betas=(0.9, 0.999), eps: float = 1e-8,
                 custom_keys: Optional[Dict[str, float]] = None, scaler: Optional[LossScaler] = None, graph_safe: bool = False,
                 clip_grad: Optional[dict] = None, ema: Optional[dict] = None, module: Optional[torch.nn.Module] = None):
        from .. import _lib as L
        self._L = L
        self.clip_grad = parse_clip_grad(clip_grad)      # ValueError before anything is built
        self.ema = parse_ema(ema)
        if self.ema is not None and self.ema["update_buffers"] and module is None:
            raise ValueError("ema.update_buffers needs module=: the model whose float buffers are averaged")
        self.reducer, self.scaler = reducer, scaler
        custom_keys = SOD_CUSTOM_KEYS if custom_keys is None else custom_keys
        self.betas, self.eps, self.weight_decay, self._steps = betas, eps, weight_decay, 0
        self.pipelined = False      # set by GraphedTrainStep(comm="fused"): every bucket's AdamW waits for that bucket's all-reduce only
        mults = sorted({lr_mult_for(n, custom_keys) for b in reducer.buckets for n in b["names"]}, reverse=True)
        self.param_groups = [{"lr": lr * m, "initial_lr": lr * m, "mult": m, "weight_decay": weight_decay} for m in mults]
        gidx = {m: i for i, m in enumerate(mults)}
        self.slots, self.runs, self.state = [], [], []
        for b in reducer.buckets:
            if not b["mflat"].is_cuda:
                raise RuntimeError("FlatAdamW runs on the HIP device; use build_optimizer() (torch.optim.AdamW) on CPU")
            # slot = (offset, padded length, group); the alignment padding after a tensor travels with it (zeros: a no-op update)
            slots = [(off, n, gidx[lr_mult_for(name, custom_keys)]) for name, off, n in zip(b["names"], b["offsets"], b["padded"])]
            self.slots.append(slots)
            self.runs.append(self._merge(slots, b["n_work"], ()))
            self.state.append({"exp_avg": torch.zeros_like(b["mflat"]), "exp_avg_sq": torch.zeros_like(b["mflat"])})
        wd = reducer.working_dtype
        self._w_dt = L.F16 if wd == torch.float16 else L.BF16
        # graph_safe: no per-step HOST value may enter a launch (a captured hipGraph would replay it frozen): the step count for the
        # bias corrections and the learning rates live in device memory.  Without a loss scaler the same device state is used with
        # scale = 1 and growth/backoff = 1, so only its step counter moves.
        self.graph_safe = graph_safe
        dev = reducer.buckets[0]["mflat"].device if reducer.buckets else "cpu"
        self._state = scaler.state if scaler is not None else (
            torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0], dtype=torch.float32, device=dev) if graph_safe else None)
        self._lr_dev = torch.tensor([g["lr"] for g in self.param_groups], dtype=torch.float32, device=dev) if graph_safe else None
        self._lr_host = [g["lr"] for g in self.param_groups]
        # clip by norm: { total norm, coefficient } and the fp64 partials (one per workgroup of every norm launch) live in device memory,
        # allocated once.  Runs are unions of whole slots and _norm_grid is subadditive, so the per-slot sum bounds every step's need.
        self._clip_norm = self.clip_grad is not None and self.clip_grad["type"] == "norm"
        self._clip_value = self.clip_grad["clip_value"] if (self.clip_grad is not None and not self._clip_norm) else 0.0
        self._clip_state = self._norm_ws = None
        if self._clip_norm:
            self._clip_state = torch.zeros(2, dtype=torch.float32, device=dev)
            self._norm_ws = torch.zeros(max(1, sum(self._norm_grid(n) for slots in self.slots for _, n, _ in slots)), dtype=torch.float64, device=dev)
            self._norm_kind = 1 if math.isinf(self.clip_grad["norm_type"]) else 0
        # EMA: the averages start as copies of the masters (the padding stays zero), the state as { coef 1, 0 steps, 0 iters, enabled }
        self.ema_bufs, self.ema_state, self._ema_named_buffers, self._ema_enabled, self._ema_want = [], None, [], True, True
        if self.ema is not None:
            for b in reducer.buckets:
                e = torch.zeros_like(b["mflat"])
                e.copy_(b["mflat"])
                self.ema_bufs.append(e)
            self.ema_state = torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=torch.float32, device=dev)
            if self.ema["update_buffers"]:
                self._ema_named_buffers = [(n, bf, bf.detach().clone()) for n, bf in module.named_buffers()
                                           if bf.dtype == torch.float32 and bf.is_cuda and bf.is_contiguous() and bf.numel()]

    # ------------------------------------------------------------------ EMA of the weights
    @property
    def ema_steps(self) -> int:
        """Updates the average has counted (mmengine's ``steps``); ONE host read."""
        return int(self.ema_state[1].item()) if self.ema_state is not None else 0

    @property
    def ema_iters(self) -> int:
        return int(self.ema_state[2].item()) if self.ema_state is not None else 0

    def set_ema_enabled(self, on: bool) -> None:
        """``begin_epoch``: while off the average stays a copy of the weights; reaches the device with the next ``sync_ema()``."""
        self._ema_want = bool(on)

    def sync_ema(self) -> None:
        """Push the ``enabled`` flag to ``ema_state``; a no-op while unchanged (and without EMA)."""
        want = self._ema_want
        if self.ema_state is not None and want != self._ema_enabled:
            self.ema_state[3:4].copy_(torch.tensor([1.0 if want else 0.0], dtype=torch.float32))
            self._ema_enabled = want

    @torch.no_grad()
    def swap_ema(self) -> None:
        """Exchange masters and averages in place (+ the float buffers with ``update_buffers``); the working copies follow the masters.
        Two calls restore every bit."""
        if self.ema is None:
            raise RuntimeError("swap_ema() needs FlatAdamW(ema=...)")
        L, st = self._L, self._L.stream_ptr()
        for b, e in zip(self.reducer.buckets, self.ema_bufs):
            p, w, nw, n = b["mflat"], b["wflat"], b["n_work"], b["mflat"].numel()
            if w is not None and nw:
                L.call("dgtd_ema_swap", p.data_ptr(), e.data_ptr(), w.data_ptr(), self._w_dt, nw, st)
            lo = nw if w is not None else 0
            if n > lo:
                L.call("dgtd_ema_swap", p.data_ptr() + 4 * lo, e.data_ptr() + 4 * lo, None, self._w_dt, n - lo, st)
        for _, bf, e in self._ema_named_buffers:
            L.call("dgtd_ema_swap", bf.data_ptr(), e.data_ptr(), None, self._w_dt, bf.numel(), st)

    def ema_tensors(self) -> Dict[str, torch.Tensor]:
        """The averages by state_dict key, in the parameters' logical shapes (views of the flat buffers; averaged buffers as they are)."""
        out = {}
        for b, e in zip(self.reducer.buckets, self.ema_bufs):
            for i, name in enumerate(b["names"]):
                out[name] = self._logical(b, i, e)
        out.update({n: e for n, _, e in self._ema_named_buffers})
        return out

    @torch.no_grad()
    def load_ema(self, named: Optional[dict], steps: int = 0, iters: int = 0) -> None:
        """``named`` = averaged tensors by state_dict key (others are ignored), or ``None``: the average restarts as a copy of the weights."""
        if self.ema is None:
            raise RuntimeError("load_ema() needs FlatAdamW(ema=...)")
        if named is None:
            for b, e in zip(self.reducer.buckets, self.ema_bufs):
                e.copy_(b["mflat"])
            for _, bf, e in self._ema_named_buffers:
                e.copy_(bf)
        else:
            for n, e in self.ema_tensors().items():
                e.copy_(named[n])
        self.ema_state[1:3].copy_(torch.tensor([float(steps), float(iters)], dtype=torch.float32))

    def _ema_rest(self, bucket, runs, st) -> None:
        """The EMA update over what this step's AdamW runs left out of ``bucket`` (slots without a gradient)."""
        L, coef, pos = self._L, self.ema_state.data_ptr(), 0
        p, e = bucket["mflat"], self.ema_bufs[bucket["index"]]
        for lo, hi in [(r[0], r[1]) for r in runs] + [(p.numel(), p.numel())]:
            if lo > pos:
                L.call("dgtd_ema_flat", p.data_ptr() + 4 * pos, e.data_ptr() + 4 * pos, lo - pos, coef, st)
            pos = max(pos, hi)

    @staticmethod
    def _norm_grid(n: int) -> int:
        """Workgroups of one norm launch: 4096 elements each, at most 1024 (4 workgroups per CU keep ~64 KB of loads in flight per CU)."""
        return max(1, min(1024, -(-n // 4096)))

    def grad_norm(self) -> Optional[float]:
        """Clip by norm: the un-scaled total gradient norm of the last step (ONE host read); ``None`` otherwise."""
        return float(self._clip_state[0].item()) if self._clip_norm else None

    @property
    def steps(self) -> int:
        """Optimizer steps actually taken (fp16 mode: read from the scaler's device state - steps it skipped do not count)."""
        return int(self._state[4].item()) if self._state is not None else self._steps

    def sync_lr(self) -> None:
        """graph_safe: push the param_groups' learning rates (what a scheduler writes) to device memory; a no-op while unchanged."""
        if self._lr_dev is not None:
            cur = [float(g["lr"]) for g in self.param_groups]
            if cur != self._lr_host:
                self._lr_dev.copy_(torch.tensor(cur, dtype=torch.float32))
                self._lr_host = cur

    @staticmethod
    def _merge(slots, n_work, missing):
        """Runs = maximal contiguous stretches with one lr on one side of the working-copy boundary, skipping ``missing`` slots."""
        runs, prev_end = [], None
        for i, (off, n, g) in enumerate(slots):
            if i in missing:
                prev_end = None
                continue
            if runs and prev_end == off and runs[-1][2] == g and off != n_work:
                runs[-1][1] = off + n
            else:
                runs.append([off, off + n, g])
            prev_end = off + n
        return runs

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.reducer.zero_grad()

    def _join(self, b, slots, runs):
        """Wait for bucket ``b``'s all-reduce (pipelined) and settle what this step reads and updates: (16-bit payload or None, runs)."""
        # pipelined: the bucket's all-reduce runs on the reducer's side stream and is joined bucket by bucket; without a loss scaler
        # (no found_inf pass over the fp32 bucket) the working-copy segment is updated straight from the 16-bit payload
        g16 = b.get("g16") if (self.pipelined and self.scaler is None and b.get("works") and _ADAM_G16) else None
        if self.pipelined:
            self.reducer.wait_bucket(b["index"], widen=g16 is None)
        # world 1: parameters without a gradient this step are skipped, like torch.optim.AdamW does.  N > 1: ``missing`` is
        # rank-local while the all-reduced slot holds the average over every rank (zero from the ranks that did not use the
        # parameter) - every rank applies the same update, so the replicas cannot drift apart
        if b["missing"] and self.reducer.world == 1:
            runs = self._merge(slots, b["n_work"], set(b["missing"]))
        return g16, runs

    @torch.no_grad()
    def step(self) -> None:
        L = self._L
        self._steps += 1
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self._steps, 1.0 - b2 ** self._steps
        st = L.stream_ptr()
        amp = self._state.data_ptr() if self._state is not None else None
        es = self.ema_state.data_ptr() if self.ema is not None else None
        if es is not None:                          # this step's coefficient, on the device, before anything reads it
            L.call("dgtd_ema_schedule", es, self.ema["kind"], self.ema["momentum"], self.ema["gamma"], self.ema["interval"],
                   self.ema["begin_iter"], st)
        if self.scaler is not None and not self._clip_norm:
            for b in self.reducer.buckets:          # GradScaler.unscale_'s found_inf over every (already all-reduced) gradient
                if self.pipelined:
                    self.reducer.wait_bucket(b["index"])
                L.call("dgtd_found_inf", b["flat"].data_ptr(), b["flat"].numel(), amp + 12, st)
        lrp = self._lr_dev.data_ptr() if self._lr_dev is not None else None
        plans = None
        if self._clip_norm:
            # every bucket's partial sums (joining that bucket's all-reduce only), then ONE finalize: nothing below starts before it
            plans, k, ws = [], 0, self._norm_ws
            for b, slots, runs in zip(self.reducer.buckets, self.slots, self.runs):
                g16, runs = self._join(b, slots, runs)
                plans.append((g16, runs))
                for lo, hi, _ in runs:
                    direct = g16 is not None and hi <= b["n_work"]
                    grid = self._norm_grid(hi - lo)
                    assert k + grid <= ws.numel()
                    L.call("dgtd_grad_norm_partial", (g16.data_ptr() + 2 * lo) if direct else (b["flat"].data_ptr() + 4 * lo),
                           self._w_dt if direct else L.F32, hi - lo, self._norm_kind, ws.data_ptr() + 8 * k, grid, st)
                    k += grid
            if k:
                L.call("dgtd_grad_clip_finalize", ws.data_ptr(), k, self._norm_kind, self.clip_grad["max_norm"],
                       amp if self.scaler is not None else None, self._clip_state.data_ptr(), st)
        coef = (self._clip_state.data_ptr() + 4) if self._clip_norm else None
        for i, (b, slots, runs, state) in enumerate(zip(self.reducer.buckets, self.slots, self.runs, self.state)):
            g16, runs = plans[i] if plans is not None else self._join(b, slots, runs)
            p, g, m, v, w, nw = b["mflat"], b["flat"], state["exp_avg"], state["exp_avg_sq"], b["wflat"], b["n_work"]
            for lo, hi, gi in runs:
                wp = (w.data_ptr() + 2 * lo) if (w is not None and hi <= nw) else None
                direct = g16 is not None and hi <= nw
                tail = (m.data_ptr() + 4 * lo, v.data_ptr() + 4 * lo, wp,
                        self._w_dt, hi - lo, float(self.param_groups[gi]["lr"]), b1, b2, self.eps,
                        float(self.param_groups[gi]["weight_decay"]), bc1, bc2, amp,
                        (lrp + 4 * gi) if lrp is not None else None)
                if es is not None:
                    L.call("dgtd_adamw_flat_ema", p.data_ptr() + 4 * lo, None if direct else (g.data_ptr() + 4 * lo),
                           (g16.data_ptr() + 2 * lo) if direct else None, *tail, coef, self._clip_value,
                           self.ema_bufs[i].data_ptr() + 4 * lo, es, st)
                elif self.clip_grad is None:
                    L.call("dgtd_adamw_flat_g16" if direct else "dgtd_adamw_flat_amp", p.data_ptr() + 4 * lo,
                           (g16.data_ptr() + 2 * lo) if direct else (g.data_ptr() + 4 * lo), *tail, st)
                else:
                    L.call("dgtd_adamw_flat_clip", p.data_ptr() + 4 * lo, None if direct else (g.data_ptr() + 4 * lo),
                           (g16.data_ptr() + 2 * lo) if direct else None, *tail, coef, self._clip_value, st)
            if es is not None:
                self._ema_rest(b, runs, st)
        if es is not None:
            for _, bf, e in self._ema_named_buffers:
                L.call("dgtd_ema_flat", bf.data_ptr(), e.data_ptr(), bf.numel(), es, st)
        if self.scaler is not None:
            L.call("dgtd_loss_scale_update", self.scaler.state.data_ptr(), float(self.scaler.growth_factor),
                   float(self.scaler.backoff_factor), int(self.scaler.growth_interval), st)
        elif self._state is not None:               # only the device-side step counter moves
            L.call("dgtd_loss_scale_update", amp, 1.0, 1.0, 1 << 30, st)

    # ------------------------------------------------------------------ torch.optim.AdamW-compatible state
    def _logical(self, b, i, flat):
        off, n, shape = b["offsets"][i], b["sizes"][i], b["shapes"][i]
        t = flat[off:off + n]
        if b["nhwc"][i]:
            return t.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
        return t.view(shape)

    def state_dict(self) -> dict:
        steps = self.steps
        names, state, members = [], {}, [[] for _ in self.param_groups]
        for b, slots, st in zip(self.reducer.buckets, self.slots, self.state):
            for i, name in enumerate(b["names"]):
                idx = len(names)
                names.append(name)
                members[slots[i][2]].append(idx)
                state[idx] = {"step": torch.tensor(float(steps)),
                              "exp_avg": self._logical(b, i, st["exp_avg"]).detach().cpu().contiguous(),
                              "exp_avg_sq": self._logical(b, i, st["exp_avg_sq"]).detach().cpu().contiguous()}
        groups = [{"lr": g["lr"], "initial_lr": g["initial_lr"], "betas": tuple(self.betas), "eps": self.eps,
                   "weight_decay": g["weight_decay"], "amsgrad": False, "maximize": False, "params": members[i]}
                  for i, g in enumerate(self.param_groups)]
        out = {"state": state, "param_groups": groups, "param_names": names}
        if self.scaler is not None:
            out["loss_scaler"] = self.scaler.state_dict()
        return out

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        names = sd.get("param_names")
        index = {n: i for i, n in enumerate(names)} if names is not None else None
        steps, k = None, 0
        for b, st in zip(self.reducer.buckets, self.state):
            for i, name in enumerate(b["names"]):
                idx = index[name] if index is not None else k
                k += 1
                src = sd["state"][idx]
                if tuple(src["exp_avg"].shape) != b["shapes"][i]:
                    raise ValueError(f"optimizer state of {name}: shape {tuple(src['exp_avg'].shape)} != parameter shape {b['shapes'][i]}")
                self._logical(b, i, st["exp_avg"]).copy_(src["exp_avg"])
                self._logical(b, i, st["exp_avg_sq"]).copy_(src["exp_avg_sq"])
                steps = int(float(src["step"])) if steps is None else steps
        self._steps = steps or 0
        if self._state is not None:
            self._state[4] = float(self._steps)
        by_mult = sorted(sd["param_groups"], key=lambda g: -g["initial_lr"])
        for g, src in zip(self.param_groups, by_mult):
            g["lr"], g["initial_lr"], g["weight_decay"] = src["lr"], src["initial_lr"], src["weight_decay"]
        if self.scaler is not None and "loss_scaler" in sd:
            self.scaler.load_state_dict(sd["loss_scaler"])
