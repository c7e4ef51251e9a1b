"""Prediction maps of a batch, each at its image's own size, as one packed uint8 buffer (csrc/predict_maps.hip, include/dgtd.h):
the resize to the original resolution, the sigmoid and ``save_image``'s quantisation (or the min-max rule of the field's test
scripts) for every sample of the batch in one launch (three with min-max), so that ONE device-to-host copy carries the batch."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib as L

_RING = 4            # pinned job tables per device, reused round-robin behind an event each
_rings: dict = {}
_captured: list = []  # job tables a captured graph reads at every replay: they live as long as the process


class _Slot:
    def __init__(self):
        self.pinned: Optional[torch.Tensor] = None
        self.uploaded = torch.cuda.Event()      # the upload has read the pinned table: the host may write the next one into it
        self.busy = False


def _pinned_table(device: torch.device, nbytes: int, capturing: bool) -> Tuple[torch.Tensor, Optional[_Slot]]:
    ring = _rings.setdefault(device, {"slots": [_Slot() for _ in range(_RING)], "next": 0, "spare": None})
    if capturing:
        # the copy node reads the table at every replay, so it is never reused: the capture takes the spare table an earlier eager
        # call set aside (pinned memory cannot be allocated while a stream captures, and a captured call is warmed up eagerly anyway)
        t, ring["spare"] = ring["spare"], None
        if t is None or t.numel() < nbytes:
            t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)      # raises under torch's default capture mode
        _captured.append(t)
        return t, None
    if ring["spare"] is None or ring["spare"].numel() < nbytes:
        ring["spare"] = torch.empty(max(4096, 1 << (nbytes - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
    slot = ring["slots"][ring["next"] % _RING]
    ring["next"] += 1
    if slot.busy and not slot.uploaded.query():      # four calls later the upload has long run: the host waits only when it has not
        slot.uploaded.synchronize()
    if slot.pinned is None or slot.pinned.numel() < nbytes:
        slot.pinned = torch.empty(max(4096, 1 << (nbytes - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
    return slot.pinned, slot


def upload_job_table(device: torch.device, sizes, offsets, batch_index) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(dev_table, pinned)``: the ``dgtd_predict_job`` table of ``sizes[j] = (H, W)`` at ``offsets[j]`` (plane ``batch_index[j]``) written
    into a pinned table of the ring and sent to a fresh device tensor in ONE asynchronous copy on the current stream.  The entries read
    ``dev_table`` on the device and ``pinned.data_ptr()`` on the host.  Shared by every op that takes this job table
    (``predict_maps``, ``sod_metrics_ragged_rows``); legal while the stream captures after one eager call on the device."""
    n = len(sizes)
    nbytes = n * ctypes.sizeof(L.PredictJob)
    pinned, slot = _pinned_table(device, nbytes, torch.cuda.is_current_stream_capturing())
    table = (L.PredictJob * n).from_buffer(pinned.numpy())
    for j, ((H, W), off, b) in enumerate(zip(sizes, offsets, batch_index)):
        jb = table[j]
        jb.out_off, jb.H, jb.W, jb.batch = off, H, W, b
        jb.reserved[0] = jb.reserved[1] = jb.reserved[2] = 0
    dev_table = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dev_table.copy_(pinned[:nbytes], non_blocking=True)
    if slot is not None:
        slot.uploaded.record()
        slot.busy = True
    return dev_table, pinned


def predict_maps(logits: torch.Tensor, sizes: Sequence[Tuple[int, int]], batch_index: Optional[Sequence[int]] = None, minmax: bool = False,
                 out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[int]]:
    """``(packed, offsets)``: map j, ``sizes[j] = (H, W)``, is ``packed[offsets[j] : offsets[j] + H * W]`` viewed ``[H, W]``, the
    bilinear resize (``F.interpolate(align_corners=False)``) of ``logits[batch_index[j]]`` followed by the sigmoid and
    ``floor(clamp(255 * s + 0.5, 0, 255))``, or with ``minmax`` by ``(s - min) / (max - min + 1e-8)`` over the map first.
    ``logits``: ``[B,1,S,S]`` or ``[B,S,S]``, contiguous, fp32 / bf16 / fp16, on the HIP device.  ``batch_index`` defaults to
    ``0 .. len(sizes) - 1``.  ``out``: a uint8 device buffer of at least ``predict_maps_layout(sizes)[1]`` bytes to fill instead of a
    fresh one; bytes between the maps are left as they are.  The job table goes up in one asynchronous copy from pinned memory, then
    one launch (three with ``minmax``) on the current stream; nothing waits for the device, so the call can be captured in a graph (after one eager call, which also sets aside the pinned table
    the captured copy will read at every replay)."""
    L.check_cuda(logits)
    if logits.ndim == 4 and logits.shape[1] == 1:
        logits = logits[:, 0]
    if logits.ndim != 3 or logits.shape[-1] != logits.shape[-2]:
        raise L.DgtdError(f"predict_maps takes [B,1,S,S] or [B,S,S] logits, got shape {tuple(logits.shape)}")
    if not logits.is_contiguous():
        raise L.DgtdError("dgtd ops need contiguous tensors")
    B, S = int(logits.shape[0]), int(logits.shape[-1])
    sizes = [(int(h), int(w)) for (h, w) in sizes]
    n = len(sizes)
    batch_index = list(range(n)) if batch_index is None else [int(b) for b in batch_index]
    if len(batch_index) != n:
        raise L.DgtdError(f"predict_maps: {n} sizes but {len(batch_index)} batch indices")
    offsets, total = L.predict_maps_layout(sizes)
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=logits.device)
    elif out.dtype != torch.uint8 or out.device != logits.device or not out.is_contiguous() or out.numel() < total:
        raise L.DgtdError(f"predict_maps: out must be a contiguous uint8 tensor of at least {total} bytes on {logits.device}")
    dev_table, pinned = upload_job_table(logits.device, sizes, offsets, batch_index)
    ws = ws_bytes = None
    if minmax:
        ws_bytes = int(L.load().dgtd_predict_maps_workspace(n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=logits.device)
    L.call("dgtd_predict_maps", L.ptr(logits), L.dtype_code(logits), B, S, L.ptr(dev_table), pinned.data_ptr(), n, L.ptr(out), out.numel(),
           int(bool(minmax)), L.ptr(ws), ws_bytes or 0, L.stream_ptr())
    return out, offsets
