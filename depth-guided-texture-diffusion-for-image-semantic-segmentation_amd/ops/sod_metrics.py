"""S-, E-, F-measure and MAE of py_sod_metrics 1.3.1 per image on the device (csrc/sod_metrics.hip, include/dgtd.h)."""
from __future__ import annotations

from typing import NamedTuple, Sequence, Tuple

import torch

from .. import _lib as L

ROW = 1028       # DGTD_SODM_ROW
STATE = 520      # DGTD_SODM_STATE


class SodMetrics(NamedTuple):
    """Per-image fp64 device tensors; curves are [B, 256] with index i <-> threshold 255 - i (py_sod_metrics' order)."""
    mae: torch.Tensor
    sm: torch.Tensor
    adp_em: torch.Tensor
    adp_fm: torch.Tensor
    em_curve: torch.Tensor
    fm_curve: torch.Tensor
    precision: torch.Tensor
    recall: torch.Tensor


def _maps(pred: torch.Tensor, gt: torch.Tensor):
    L.check_cuda(pred, gt)
    if pred.ndim == 4:
        if pred.shape[1] != 1:
            raise L.DgtdError(f"sod_metrics takes one-channel maps, got pred of shape {tuple(pred.shape)}")
        pred = pred.squeeze(1)
    if gt.ndim == 4:
        gt = gt.squeeze(1)
    if pred.ndim != 3 or gt.shape != pred.shape:
        raise L.DgtdError(f"sod_metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must both be [B,1,H,W] or [B,H,W]")
    L.dtype_code(pred)
    return pred.contiguous(), gt.float().contiguous()


def sod_metrics_rows(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """[B, ROW] fp64 rows {mae, sm, adp_em, adp_fm, em_curve[256], fm_curve[256], precision[256], recall[256]}: four launches on the
    current stream (workspace memset, stats, histogram, finalise), no synchronisation."""
    pred, gt = _maps(pred, gt)
    B, H, W = pred.shape
    out = torch.empty(B, ROW, dtype=torch.float64, device=pred.device)
    ws = torch.empty(L.load().dgtd_sod_metrics_workspace(B), dtype=torch.uint8, device=pred.device)
    L.call("dgtd_sod_metrics", L.ptr(pred), L.dtype_code(pred), L.ptr(gt), L.ptr(out), L.ptr(ws), B, H, W, L.stream_ptr())
    return out


def split_rows(out: torch.Tensor) -> SodMetrics:
    return SodMetrics(out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4:260], out[:, 260:516], out[:, 516:772], out[:, 772:1028])


def sod_metrics(pred: torch.Tensor, gt: torch.Tensor) -> SodMetrics:
    """Per-image metrics of ``pred`` (probabilities in [0, 1], fp32 / bf16 / fp16) against ``gt`` (fp32 in [0, 1]), both
    [B,1,H,W] or [B,H,W], any H and W.  Both maps are quantised to uint8 the way the reference's wrappers do
    ((x * 255).astype(np.uint8), gt > 128)."""
    return split_rows(sod_metrics_rows(pred, gt))


class RaggedMaps(NamedTuple):
    """A batch of uint8 maps, each at its own size: map j is ``sizes[j] = (H, W)`` bytes at ``offsets[j]`` of ``pred8`` (the prediction
    bytes, what ``ops.predict_maps`` returns) and at the same offset of ``gt8`` (the ground truth, foreground where the byte is above
    128).  Both are flat uint8 device tensors in the packing of ``_lib.predict_maps_layout``; ``sizes`` and ``offsets`` live on the
    host."""
    pred8: torch.Tensor
    gt8: torch.Tensor
    sizes: Sequence[Tuple[int, int]]
    offsets: Sequence[int]


def sod_metrics_ragged_rows(maps: RaggedMaps) -> torch.Tensor:
    """[n, ROW] fp64 rows (the layout of ``sod_metrics_rows``) of the ``n`` maps, each scored at its own size on its bytes as they are
    (no quantisation on this path).  The job table goes up in one asynchronous copy from pinned memory (the ring of
    ``ops.predict_maps``), then four launches on the current stream (workspace memset, stats, histogram, finalise); no
    synchronisation, so the call can be captured in a graph after one eager call."""
    from .predict_maps import upload_job_table
    pred8, gt8 = maps.pred8, maps.gt8
    L.check_cuda(pred8, gt8)
    if pred8.dtype != torch.uint8 or gt8.dtype != torch.uint8 or pred8.ndim != 1 or gt8.ndim != 1 or gt8.device != pred8.device:
        raise L.DgtdError("sod_metrics_ragged takes two flat uint8 tensors on one device")
    sizes = [(int(h), int(w)) for (h, w) in maps.sizes]
    offsets = [int(o) for o in maps.offsets]
    n = len(sizes)
    if len(offsets) != n or not 1 <= n <= L.PREDICT_MAPS_MAX_JOBS:
        raise L.DgtdError(f"sod_metrics_ragged: {n} sizes and {len(offsets)} offsets, a call takes 1..{L.PREDICT_MAPS_MAX_JOBS} maps")
    out = torch.empty(n, ROW, dtype=torch.float64, device=pred8.device)
    ws = torch.empty(L.load().dgtd_sod_metrics_workspace(n), dtype=torch.uint8, device=pred8.device)
    dev_table, pinned = upload_job_table(pred8.device, sizes, offsets, [0] * n)
    L.call("dgtd_sod_metrics_ragged", L.ptr(pred8), L.ptr(gt8), min(pred8.numel(), gt8.numel()), L.ptr(dev_table), pinned.data_ptr(), n,
           L.ptr(out), L.ptr(ws), L.stream_ptr())
    return out


def sod_metrics_ragged(maps: RaggedMaps) -> SodMetrics:
    """Per-image metrics of a ragged batch of uint8 maps: what ``sod_metrics`` gives for each image alone at its own size."""
    return split_rows(sod_metrics_ragged_rows(maps))


def sod_metrics_accumulate(out: torch.Tensor, state: torch.Tensor, slot: torch.Tensor) -> None:
    """state [STATE] fp64 += the rows of ``out`` (in order); slot [3] fp64 = (mean sm, max mean em curve, max mean fm curve) over every
    image accumulated so far - the running values the wrappers append per process() call.  One launch, no synchronisation."""
    L.check_cuda(out, state, slot)
    assert out.dtype == state.dtype == slot.dtype == torch.float64 and out.shape[1] == ROW
    assert state.numel() == STATE and slot.numel() >= 3
    L.call("dgtd_sod_metrics_accumulate", L.ptr(out), out.shape[0], L.ptr(state), L.ptr(slot), L.stream_ptr())
