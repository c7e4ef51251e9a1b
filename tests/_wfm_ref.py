"""NumPy fp64 restatement of py_sod_metrics 1.3.1 ``WeightedFmeasure`` (beta^2 = 1) and of the reference's wrapper around it
(twig/metric/WeightedFmeasure.py).  Test helper only: the package never imports it, and it needs no scipy.

The Euclidean transform is restated as the two-phase integer rule that reproduces ``scipy.ndimage.distance_transform_edt(gt == 0,
return_indices=True)``, its choice among equidistant foreground pixels included (tests/golden/wfm.npz holds scipy's own output):
  phase 1, per column: the nearest foreground pixel of the pixel's own column, the smaller row on a tie;
  phase 2, per row: the column j minimising (x - j)^2 + (y - cy[y, j])^2 over the columns that have a candidate, the smallest j on
  a tie.
The 7x7 convolution is a plain 49-tap zero-padded sum, rows outer, columns inner - the order the kernel adds in."""
from __future__ import annotations

import numpy as np

from _sod_metrics_ref import _prepare_data, quantise

EPS = np.spacing(1)
_NONE = 1 << 30            # squared row distance of a column without a candidate (any real one is below 2^29)
_CHUNK = 1 << 25           # elements of one (rows, x, j) cost block: 128 MB of int32


def column_candidates(mask: np.ndarray) -> np.ndarray:
    """cy [H, W] int64: row of the nearest foreground pixel of the same column (smaller row on a tie), -1 without one."""
    H, W = mask.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(mask, rows, -1), axis=0)
    dn = np.minimum.accumulate(np.where(mask, rows, 2 * H)[::-1], axis=0)[::-1]
    take_dn = (dn < 2 * H) & ((up < 0) | (dn - rows < rows - up))
    return np.where(take_dn, dn, up)


def edt_nearest(mask: np.ndarray):
    """(dist2, index) int32 [H, W]: squared distance to the nearest foreground pixel and its flat index y * W + x; -1 in both for
    a mask without foreground."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    dist2 = np.full((H, W), -1, np.int32)
    index = np.full((H, W), -1, np.int32)
    if not mask.any():
        return dist2, index
    cy = column_candidates(mask)
    dy2 = np.where(cy >= 0, (np.arange(H, dtype=np.int64)[:, None] - cy) ** 2, _NONE).astype(np.int32)
    cols = np.arange(W, dtype=np.int32)
    xc = max(1, min(W, _CHUNK // W))
    rc = max(1, _CHUNK // (W * xc))
    for x0 in range(0, W, xc):
        dx2 = (cols[x0:x0 + xc, None] - cols[None, :]) ** 2                      # [x, j]
        for r0 in range(0, H, rc):
            cost = dx2[None] + dy2[r0:r0 + rc, None, :]                          # [r, x, j]
            j = cost.argmin(axis=2)                                              # first minimum: the smallest j
            r = np.arange(r0, min(H, r0 + rc))[:, None]
            dist2[r0:r0 + rc, x0:x0 + xc] = np.take_along_axis(cost, j[..., None], axis=2)[..., 0]
            index[r0:r0 + rc, x0:x0 + xc] = cy[r, j] * W + j
    return dist2, index


def gauss7() -> np.ndarray:
    """matlab_style_gauss2D((7, 7), sigma=5)"""
    y, x = np.ogrid[-3.0:4.0, -3.0:4.0]
    h = np.exp(-(x * x + y * y) / (2.0 * 5 * 5))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    s = h.sum()
    if s != 0:
        h /= s
    return h


def convolve7(a: np.ndarray, k: np.ndarray) -> np.ndarray:
    """49 taps, zero padding (scipy.ndimage.convolve(a, k, mode="constant", cval=0) for the symmetric k, in a fixed order)."""
    H, W = a.shape
    pad = np.zeros((H + 6, W + 6), np.float64)
    pad[3:3 + H, 3:3 + W] = a
    out = np.zeros((H, W), np.float64)
    for i in range(7):
        for j in range(7):
            out = out + k[i, j] * pad[i:i + H, j:j + W]
    return out


def cal_wfm(pred: np.ndarray, gt: np.ndarray, edt=None, conv=None) -> float:
    """The package's cal_wfm on prepared data (pred fp64 in [0, 1], gt bool with at least one foreground pixel).  ``edt(bg) ->
    (Dst, flat Idx)`` and ``conv(Et, K)`` default to the restatements above (the fixture generator passes scipy's)."""
    H, W = gt.shape
    if edt is None:
        d2, flat = edt_nearest(gt)
        Dst = np.sqrt(d2.astype(np.float64))
    else:
        Dst, flat = edt(gt == 0)
    E = np.abs(pred - gt)
    Et = np.copy(E)
    Et[gt == 0] = E.ravel()[flat[gt == 0]]
    K = gauss7()
    EA = convolve7(Et, K) if conv is None else conv(Et, K)
    MIN_E_EA = np.where(gt & (EA < E), EA, E)
    B = np.where(gt == 0, 2 - np.exp(np.log(0.5) / 5 * Dst), np.ones_like(E))
    Ew = MIN_E_EA * B
    TPw = np.sum(gt) - np.sum(Ew[gt == 1])
    FPw = np.sum(Ew[gt == 0])
    R = 1 - np.mean(Ew[gt == 1])
    P = TPw / (TPw + FPw + EPS)
    return float(2 * R * P / (R + P + EPS))


def step(p8: np.ndarray, g8: np.ndarray, edt=None, conv=None) -> float:
    """WeightedFmeasure.step for one uint8 pair: the image's Q."""
    pred, gt = _prepare_data(p8, g8)
    if not gt.any():
        return 0.0
    return cal_wfm(pred, gt, edt, conv)


def per_image(pred_f32, gt_f32) -> float:
    return step(quantise(pred_f32), quantise(gt_f32))


class Wrapper:
    """twig/metric/WeightedFmeasure.py: every image of the batch stepped, one running get_results()["wfm"] appended per batch,
    compute_metrics = mean of those values."""

    def __init__(self):
        self.wfms, self.results = [], []

    def process(self, pred_b, gt_b):
        pred_b, gt_b = np.asarray(pred_b, np.float32), np.asarray(gt_b, np.float32)
        for x, y in zip(pred_b.reshape(len(pred_b), *pred_b.shape[-2:]), gt_b.reshape(len(gt_b), *gt_b.shape[-2:])):
            self.wfms.append(per_image(x, y))
        self.results.append(float(np.mean(np.array(self.wfms, np.float64))))

    def compute_metrics(self) -> dict:
        return {"WeightedFmeasure": float(sum(self.results) / len(self.results))}

    def summary(self) -> dict:
        return {"wFmeasure": float(np.mean(np.array(self.wfms, np.float64)))}
