"""The seven dataset classes of the reference's ``twig/dataset`` (sod_train.py, cod10k_camo_train.py, sod_test.py, cod10k_test.py,
camo_test.py, chameleon.py, nc4k.py), registered under the reference's names with its constructor signature
``(data_dir, depth_dir, split, image_size=None)``, so that the ``train_dataloader.dataset`` / ``val_dataloader.dataset`` blocks of
config/sod.yml and config/cod.yml bind unchanged.

Two ways to a sample:
  * ``ds[index]`` - the HOST path and executable specification: the reference's dict ``{'raw', 'input', 'label', 'depth'}`` as CPU
    fp32 tensors, computed with PIL's own ``resize((S, S), BILINEAR)`` after the flip, then ToTensor / Normalize in float32
    (``(v / 255 - mean) / std``, in that order).
  * ``ds.decode(index, epoch)`` - three decoded uint8 arrays plus the flip coin, for ``runner.data.DeviceLoader``, which resizes
    and normalises a whole batch on the device (``dgtd_preprocess_batch``) and must equal the host path bit for bit.

Deviations from the reference, both deliberate:
  * ``raw`` is the image PATH in every class.  The reference's train classes and NC4K return a resized PIL image there, which the loss
    path never reads (cod.py takes ``raw`` only for the PNG dumps of predict mode); ``SyntheticRGBD`` already returns a path.
  * ``filter_files`` drops the whole (image, GT, depth) TRIPLE when the image and GT sizes differ.  The reference filters only the
    image and GT lists, after which its depth list is out of step with them from the first dropped pair on.

The flip coin.  The reference draws one ``np.random`` seed per sample and re-seeds before each of the three transforms
(sod_train.py:65-77), so image, GT and depth share ONE RandomHorizontalFlip(p=0.5) coin that differs from call to call.  Here the
coin is the pure function ``flip_coin(seed, epoch, index)``: the top bit of the splitmix64 finaliser applied to
``seed * 0x9E3779B97F4A7C15 + epoch * 0xBF58476D1CE4E5B9 + index * 0x94D049BB133111EB + 0x2545F4914F6CDD1D (mod 2^64)``.  It does
not depend on the rank, the worker or the order of calls: every rank that draws index i in epoch e sees the same sample, and the
host and device paths can be compared.  ``seed`` is the dataset's ``seed`` attribute (0; ``Runner`` sets it to its own seed),
``epoch`` its ``epoch`` attribute for ``ds[index]`` (``set_epoch``) or the argument of ``decode``.  Test classes never flip.

``image_size``: the reference accepts it and ignores it.  Here an int or ``[s, s]`` overrides the class default; it must be square
and a multiple of 32 (the backbone's total stride).  ``None`` keeps the default."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from PIL import Image

from .data import IMAGENET_MEAN, IMAGENET_STD
from .registry import export

_M64 = (1 << 64) - 1


def flip_coin(seed: int, epoch: int, index: int) -> bool:
    """One fair coin per (seed, epoch, index): see the module docstring."""
    x = (int(seed) * 0x9E3779B97F4A7C15 + int(epoch) * 0xBF58476D1CE4E5B9 + int(index) * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return bool(x >> 63)


def _square_size(image_size, default: int) -> int:
    if image_size is None:
        return default
    if isinstance(image_size, (list, tuple)):
        if len(image_size) != 2 or int(image_size[0]) != int(image_size[1]):
            raise ValueError(f"image_size must be square, got {image_size!r}")
        image_size = image_size[0]
    s = int(image_size)
    if s < 32 or s % 32:
        raise ValueError(f"image_size must be a positive multiple of 32, got {image_size!r}")
    return s


def host_transform(img_u8: np.ndarray, size: int, normalize: bool, flip: bool) -> torch.Tensor:
    """uint8 [H, W, 3] / [H, W] -> CPU fp32 [C, size, size]: hflip, PIL resize((size, size), BILINEAR), ToTensor (, Normalize)."""
    x = np.ascontiguousarray(img_u8[:, ::-1]) if flip else img_u8
    r = np.asarray(Image.fromarray(x).resize((size, size), Image.BILINEAR))
    if r.ndim == 2:
        r = r[:, :, None]
    t = r.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    if normalize:
        t = (t - np.asarray(IMAGENET_MEAN, np.float32)[:, None, None]) / np.asarray(IMAGENET_STD, np.float32)[:, None, None]
    return torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))


class _FolderRGBD:
    """Shared body of the seven classes; a subclass names its directories, default size and whether it trains."""
    IMAGE_DIR = "RGB"
    GT_DIR = "GT"
    PREFIX: Tuple[str, ...] = ()      # directory levels between data_dir and the three folders (NC4K: 'train')
    DEFAULT_SIZE = 384
    TRAIN = False                     # train classes accept any split and flip; test classes take test/val and never flip
    SKIP = 0                          # leading positions of the sorted lists that are not part of the set (COD10K_TEST)
    WHAT = "this dataset"

    def __init__(self, data_dir: str, depth_dir: str, split: str, image_size: Optional[Union[int, Sequence[int]]] = None):
        if not self.TRAIN:
            if split == "train":
                raise ValueError(f"{self.WHAT} is usually used for testing")
            if split not in ("test", "val"):
                raise NotImplementedError(f"Unsupported split {split}")
        self.image_size = _square_size(image_size, self.DEFAULT_SIZE)
        self.seed, self.epoch = 0, 0
        dirs = [os.path.join(data_dir, *self.PREFIX, d) for d in (self.IMAGE_DIR, self.GT_DIR, depth_dir)]
        lists = [sorted(os.path.join(d, f) for f in os.listdir(d))[self.SKIP:] for d in dirs]     # sorted independently, matched by position
        if len({len(l) for l in lists}) != 1:
            raise ValueError("image, GT and depth lists differ in length: " + ", ".join(f"{d}: {len(l)}" for d, l in zip(dirs, lists)))
        self.images, self.gts, self.depth = lists
        self.filter_files()

    def filter_files(self) -> None:
        """Keep the positions whose image and GT have the same size; a mismatch drops the whole triple (module docstring)."""
        keep = []
        for i, (ip, gp) in enumerate(zip(self.images, self.gts)):
            with Image.open(ip) as a, Image.open(gp) as b:
                if a.size == b.size:
                    keep.append(i)
        self.images, self.gts, self.depth = ([l[i] for i in keep] for l in (self.images, self.gts, self.depth))

    def __len__(self) -> int:
        return len(self.images)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    @staticmethod
    def rgb_loader(path: str) -> np.ndarray:
        with open(path, "rb") as f:
            return np.asarray(Image.open(f).convert("RGB"))

    @staticmethod
    def binary_loader(path: str) -> np.ndarray:
        with open(path, "rb") as f:
            return np.asarray(Image.open(f).convert("L"))

    def flip(self, index: int, epoch: int) -> bool:
        return self.TRAIN and flip_coin(self.seed, epoch, index)

    def decode(self, index: int, epoch: int = 0):
        """``(rgb [H,W,3], gt [H,W], depth [H',W'], flip)``: uint8 arrays as the reference's loaders decode them, and the one coin."""
        return self.rgb_loader(self.images[index]), self.binary_loader(self.gts[index]), self.binary_loader(self.depth[index]), self.flip(index, epoch)

    def __getitem__(self, index: int) -> dict:
        rgb, gt, dep, flip = self.decode(index, self.epoch)
        S = self.image_size
        return {"raw": self.images[index], "input": host_transform(rgb, S, True, flip), "label": host_transform(gt, S, False, flip),
                "depth": host_transform(dep, S, False, flip)}


@export
class SOD_TRAIN(_FolderRGBD):
    """twig/dataset/sod_train.py: RGB / GT / <depth_dir>, 384, one shared flip coin."""
    IMAGE_DIR, DEFAULT_SIZE, TRAIN = "RGB", 384, True


@export
class COD10K_CAMO_TRAIN(_FolderRGBD):
    """twig/dataset/cod10k_camo_train.py: Imgs / GT / <depth_dir>, 384, one shared flip coin."""
    IMAGE_DIR, DEFAULT_SIZE, TRAIN = "Imgs", 384, True


@export
class SOD_TEST(_FolderRGBD):
    """twig/dataset/sod_test.py: RGB / GT / <depth_dir>, 384."""
    IMAGE_DIR, DEFAULT_SIZE, WHAT = "RGB", 384, "The NLPR dataset"


@export
class COD10K_TEST(_FolderRGBD):
    """twig/dataset/cod10k_test.py: Image / GT / <depth_dir>, 384; the three sorted lists are sliced ``[3381:]`` before filtering
    (the folder holds the CAMO and CHAMELEON files in front of the COD10K test set)."""
    IMAGE_DIR, DEFAULT_SIZE, SKIP, WHAT = "Image", 384, 3381, "The testing set of COD10K"


@export
class COD_TEST(_FolderRGBD):
    """twig/dataset/camo_test.py: Image / GT / <depth_dir>, 704."""
    IMAGE_DIR, DEFAULT_SIZE, WHAT = "Image", 704, "The testing set of CAMO"


@export
class CHAMELEON(_FolderRGBD):
    """twig/dataset/chameleon.py: Image / GT / <depth_dir>, 704."""
    IMAGE_DIR, DEFAULT_SIZE, WHAT = "Image", 704, "CHAMELEON"


@export
class NC4K(_FolderRGBD):
    """twig/dataset/nc4k.py: train/Image, train/GT, train/<depth_dir>, 704."""
    IMAGE_DIR, DEFAULT_SIZE, PREFIX, WHAT = "Image", 704, ("train",), "The NC4K"


DATASETS: List[str] = ["SOD_TRAIN", "COD10K_CAMO_TRAIN", "SOD_TEST", "COD10K_TEST", "COD_TEST", "CHAMELEON", "NC4K"]
