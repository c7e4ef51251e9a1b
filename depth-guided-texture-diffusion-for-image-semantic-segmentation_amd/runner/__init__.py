"""Minimal pieces of the training loop the reference delegates to nest/mmengine."""
from .optim import EmaTorch, FlatAdamW, LossScaler, build_optimizer, clip_grad_torch, ema_coefficient, lr_mult_for, parse_clip_grad, parse_ema  # noqa: F401
from .data import DefaultSampler, DeviceLoader, SyntheticRGBD, batches, device_preprocess, device_sample
from . import datasets  # noqa: F401  (registers SOD_TRAIN, COD10K_CAMO_TRAIN, SOD_TEST, COD10K_TEST, COD_TEST, CHAMELEON, NC4K)
from . import metrics  # noqa: F401  # noqa: F401
from .checkpoint import load_checkpoint, load_checkpoint_file, load_pretrained, save_checkpoint  # noqa: F401
from .config import CosineByEpoch, Runner, build_model, build_optim, load_config  # noqa: F401
from .graph import GraphedTrainStep  # noqa: F401
from . import predict  # noqa: F401
from .predict import MapWriter, score_maps  # noqa: F401
from . import registry  # noqa: F401
from .registry import build as build_exported, export, install_nest_shim, register_model  # noqa: F401
