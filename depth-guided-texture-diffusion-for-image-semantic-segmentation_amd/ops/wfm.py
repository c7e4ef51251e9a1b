"""Weighted F-measure of py_sod_metrics 1.3.1 per image on the device, and the exact nearest-foreground transform under it
(csrc/wfm.hip, include/dgtd.h)."""
from __future__ import annotations

from typing import Tuple

import torch

from .. import _lib as L
from .sod_metrics import _maps

WFM_STATE = 2        # DGTD_WFM_STATE
EDT_MAX_W = 16384    # DGTD_EDT_MAX_W


def edt_nearest(mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dist2, index), both int32 of ``mask``'s shape ([B,H,W] or [H,W], non-zero = foreground): the squared Euclidean distance to
    the nearest foreground pixel and its flat index ``y * W + x`` within the image, with scipy's
    ``distance_transform_edt(mask == 0, return_indices=True)`` choice among equidistant pixels.  -1 in both for an image without
    foreground.  Two launches on the current stream, no synchronisation.  Raises for a side above ``EDT_MAX_W``."""
    L.check_cuda(mask)
    if mask.ndim not in (2, 3):
        raise L.DgtdError(f"edt_nearest takes a [B,H,W] or [H,W] mask, got shape {tuple(mask.shape)}")
    m = (mask != 0).to(torch.uint8).reshape(-1, *mask.shape[-2:]).contiguous()
    B, H, W = m.shape
    dist2 = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    index = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    L.call("dgtd_edt_nearest", L.ptr(m), L.ptr(dist2), L.ptr(index), B, H, W, L.stream_ptr())
    return dist2.reshape(mask.shape), index.reshape(mask.shape)


def weighted_fmeasure_rows(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """[B] fp64: the package's per-image weighted F-measure of ``pred`` (probabilities in [0, 1], fp32 / bf16 / fp16) against ``gt``
    (fp32 in [0, 1]), both [B,1,H,W] or [B,H,W], quantised to uint8 the way the reference's wrapper does.  One workspace memset and
    five launches on the current stream, no synchronisation."""
    pred, gt = _maps(pred, gt)
    B, H, W = pred.shape
    out = torch.empty(B, dtype=torch.float64, device=pred.device)
    ws = torch.empty(L.load().dgtd_wfm_workspace(B, H, W), dtype=torch.uint8, device=pred.device)
    L.call("dgtd_wfm", L.ptr(pred), L.dtype_code(pred), L.ptr(gt), L.ptr(out), L.ptr(ws), B, H, W, L.stream_ptr())
    return out


def weighted_fmeasure_accumulate(out: torch.Tensor, state: torch.Tensor, slot: torch.Tensor) -> None:
    """state [WFM_STATE] fp64 = {n, sum wfm} += the values of ``out`` (in order); slot [1] fp64 = the mean over every image
    accumulated so far - the running value the wrapper appends per process() call.  One launch, no synchronisation."""
    L.check_cuda(out, state, slot)
    assert out.dtype == state.dtype == slot.dtype == torch.float64 and out.ndim == 1
    assert state.numel() == WFM_STATE and slot.numel() >= 1
    L.call("dgtd_wfm_accumulate", L.ptr(out), out.shape[0], L.ptr(state), L.ptr(slot), L.stream_ptr())
