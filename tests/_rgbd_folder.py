"""Test helper: writes small RGB / GT / depth image folders in the layouts runner/datasets.py reads, from seeded numpy arrays."""
import os

import numpy as np
from PIL import Image

# (H, W) of seven triples: down-scales, an up-scale, odd sizes, a 1-pixel-high image
SIZES7 = [(97, 131), (20, 30), (1, 7), (50, 33), (120, 90), (64, 64), (75, 200)]


def write_folder(root, image_dir="RGB", depth_dir="depth", prefix=(), sizes=SIZES7, seed=0, jpeg=None, gt_sizes=None, names=None):
    """``len(sizes)`` triples under ``root/<prefix>/{image_dir, GT, depth_dir}``.  Image ``jpeg`` (an index) is written as JPEG, all
    others as PNG.  ``gt_sizes`` {index: (H, W)} gives a GT another size than its image.  Returns the arrays written, per triple
    ``(rgb, gt, depth)``; for the JPEG image the array is what decoding the file gives back."""
    rng = np.random.default_rng(seed)
    base = os.path.join(str(root), *prefix)
    for d in (image_dir, "GT", depth_dir):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    out = []
    for i, (h, w) in enumerate(sizes):
        name = names[i] if names else f"{i:03d}"
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        gh, gw = (gt_sizes or {}).get(i, (h, w))
        gt = (rng.integers(0, 2, (gh, gw), dtype=np.uint8) * 255).astype(np.uint8)
        dep = rng.integers(0, 256, (h, w), dtype=np.uint8)
        ipath = os.path.join(base, image_dir, name + (".jpg" if i == jpeg else ".png"))
        Image.fromarray(rgb).save(ipath, quality=90) if i == jpeg else Image.fromarray(rgb).save(ipath)
        if i == jpeg:
            rgb = np.asarray(Image.open(ipath).convert("RGB"))
        Image.fromarray(gt).save(os.path.join(base, "GT", name + ".png"))
        Image.fromarray(dep).save(os.path.join(base, depth_dir, name + ".png"))
        out.append((rgb, gt, dep))
    return out
