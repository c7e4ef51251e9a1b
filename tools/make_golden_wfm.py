#!/usr/bin/env python
"""Writes tests/golden/wfm.npz: small uint8 (pred, gt) pairs with scipy's own ``distance_transform_edt(gt == 0,
return_indices=True)`` output and the weighted F-measure of the restated package formula (tests/_wfm_ref.py) evaluated with scipy's
transform and ``scipy.ndimage.convolve``.  Needs scipy; the tests that read the file do not.

    python tools/make_golden_wfm.py

Keys per case k: pred_k, gt_k (uint8 [H,W]), q_k (fp64 scalar) and, where gt has foreground, idx_k (int16 [2,H,W]) and dst_k (fp64)."""
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _wfm_ref as R  # noqa: E402


def smooth(rng, H, W, sigma=6.0):
    z = ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma)
    z = (z - z.min()) / (z.max() - z.min())
    return z


def u8(x):
    return (np.asarray(x, np.float32) * 255).astype(np.uint8)


def cases():
    rng = np.random.default_rng(20231)
    out = []

    def add(name, gt, pred=None):
        H, W = gt.shape
        pred = smooth(rng, H, W) if pred is None else pred
        out.append((name, u8(pred), u8(gt.astype(np.float32))))

    g = np.zeros((64, 64), bool)
    g[10:30, 8:40] = True
    g[40:56, 30:60] = True
    add("rectangles", g)
    yy, xx = np.mgrid[:40, :56]
    add("checkerboard3", ((yy // 3 + xx // 3) % 2) == 0)
    yy, xx = np.mgrid[:24, :24]
    add("checkerboard1", ((yy + xx) % 2) == 0)
    g = np.zeros((48, 48), bool)
    g[12, 12] = g[35, 35] = True
    add("two_pixels_diagonal", g)
    g = np.zeros((33, 47), bool)
    g[16, 10] = g[16, 36] = True
    add("two_pixels_row", g)
    add("blob_border", smooth(rng, 96, 96, 10.0) > 0.55)
    g = smooth(rng, 96, 96, 8.0) > 0.5
    g[:20, :] = True
    add("blob_top_edge", g, pred=np.clip(g * 0.8 + smooth(rng, 96, 96) * 0.3, 0, 1))
    add("sparse_37x83", rng.random((37, 83)) < 0.01)
    add("dense_83x37", rng.random((83, 37)) < 0.3)
    add("very_sparse_96", rng.random((96, 96)) < 0.002)
    add("all_foreground", np.ones((20, 28), bool))
    add("empty_gt", np.zeros((20, 28), bool))
    g = np.zeros((32, 40), bool)
    g[8:20, 10:30] = True
    add("constant_pred", g, pred=np.full((32, 40), 0.5))
    g = np.zeros((30, 30), bool)
    g[0, 0] = True
    add("corner_pixel", g)
    add("diagonal_line", np.eye(41, dtype=bool))
    return out


def scipy_edt(bg):
    dst, idx = ndimage.distance_transform_edt(bg, return_indices=True)
    return dst, idx[0] * bg.shape[1] + idx[1]


def scipy_conv(et, k):
    return ndimage.convolve(et, weights=k, mode="constant", cval=0)


def main():
    data = {}
    names = []
    for name, p8, g8 in cases():
        names.append(name)
        data[f"pred_{name}"], data[f"gt_{name}"] = p8, g8
        data[f"q_{name}"] = np.float64(R.step(p8, g8, edt=scipy_edt, conv=scipy_conv))
        if (g8 > 128).any():
            dst, idx = ndimage.distance_transform_edt(~(g8 > 128), return_indices=True)
            data[f"idx_{name}"], data[f"dst_{name}"] = idx.astype(np.int16), dst
    data["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "wfm.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
