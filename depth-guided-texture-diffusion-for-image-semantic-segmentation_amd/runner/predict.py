"""Prediction maps on disk: one grey-level PNG per image, at that image's own resolution, named by the image's stem - the folder
every evaluation toolbox of salient / camouflaged object detection reads, and the ``_output.png`` the reference's predict mode
writes as a side effect (twig/model/cod.py:156-217).  Per batch: ``ops.predict_maps`` (resize, sigmoid and quantisation of every
sample into one packed uint8 buffer), ONE device-to-host copy into a pinned staging buffer, and the PNG encode of the previous batch
in a pool of threads while the device runs the next forward."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

import torch

NORMALIZE = ("none", "minmax")


def parse_save_maps(block) -> Optional[dict]:
    """``val_cfg.save_maps`` of the YAML -> ``{"out_dir": str or None, "minmax": bool}`` (``None`` without the block).  Keys:
    ``out_dir`` (a path) and ``normalize`` (``none``: ``save_image``'s rule; ``minmax``: ``(s - min) / (max - min + 1e-8)`` per map
    first).  An unknown key or value raises."""
    if block is None:
        return None
    if not isinstance(block, dict):
        raise TypeError(f"val_cfg.save_maps must be a mapping, got {block!r}")
    unknown = set(block) - {"out_dir", "normalize"}
    if unknown:
        raise KeyError(f"val_cfg.save_maps: unknown key(s) {sorted(unknown)}; known: out_dir, normalize")
    norm = block.get("normalize", "none")
    norm = "none" if norm is None else norm          # YAML reads a bare `none` as the string, `null` / `~` as None
    if norm not in NORMALIZE:
        raise ValueError(f"val_cfg.save_maps.normalize must be one of {NORMALIZE}, got {norm!r}")
    out_dir = block.get("out_dir")
    if out_dir is not None and not isinstance(out_dir, (str, os.PathLike)):
        raise TypeError(f"val_cfg.save_maps.out_dir must be a path, got {out_dir!r}")
    return {"out_dir": None if out_dir is None else os.fspath(out_dir), "minmax": norm == "minmax"}


def map_path(out_dir: str, raw) -> str:
    """``out_dir/<stem of raw>.png``."""
    return os.path.join(out_dir, os.path.splitext(os.path.basename(str(raw)))[0] + ".png")


def encode_png(buf, H: int, W: int, path: str, tag: str) -> str:
    """Write the ``H * W`` bytes of ``buf`` as a mode-L PNG to a temporary name beside ``path`` and rename it into place: a reader
    never sees half a file, and a sample written twice (``DefaultSampler`` repeats some across ranks) ends up with identical bytes."""
    from PIL import Image
    tmp = f"{path}.{tag}.tmp"
    try:
        Image.frombuffer("L", (W, H), buf, "raw", "L", 0, 1).save(tmp, format="PNG")
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


class _Stage:
    """One pinned staging buffer and what is in it."""

    def __init__(self):
        self.pinned: Optional[torch.Tensor] = None
        self.copied = torch.cuda.Event() if torch.cuda.is_available() else None
        self.jobs: list = []          # (path, H, W, offset) of the batch whose bytes are (on their way) in the buffer
        self.futures: list = []       # the encodes reading the buffer

    def room(self, nbytes: int) -> torch.Tensor:
        if self.pinned is None or self.pinned.numel() < nbytes:
            self.pinned = torch.empty(max(1 << 16, 1 << (int(nbytes) - 1).bit_length()), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return self.pinned


class MapWriter:
    """``submit(batch, logits)`` per batch, ``close()`` at the end; ``paths`` lists the files written, in order.

    Two pinned staging buffers (grown to a power of two, then reused) alternate.  ``submit`` runs ``ops.predict_maps`` on the batch's
    logits (``cod.forward(mode='tensor')``), enqueues one device-to-host copy of the packed maps and an event, and returns without
    waiting for either; it then hands the PREVIOUS batch, whose copy has long landed, to ``workers`` encode THREADS (never
    processes), which run while the device computes the next forward.  A sample is written at ``batch['size'][i]``
    (``DeviceLoader(with_sizes=True)``; ``submit(..., packed=...)`` takes maps that are already computed), or at the logits' own ``S x S`` when the batch has no sizes (synthetic data, datasets
    without ``decode``).  ``close()`` encodes what is left, joins the pool and re-raises the first encode error."""

    def __init__(self, out_dir: str, minmax: bool = False, workers: int = 8):
        self.out_dir, self.minmax = os.fspath(out_dir), bool(minmax)
        os.makedirs(self.out_dir, exist_ok=True)
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), 16)), thread_name_prefix="dgtd-png")
        self.stages = [_Stage(), _Stage()]
        self.batches = 0
        self.paths: List[str] = []
        self._done: list = []          # futures of every encode, in order
        self._seq = 0

    # -------------------------------------------------------------- device side
    def submit(self, batch: dict, logits: torch.Tensor, packed=None) -> None:
        """``packed = (bytes, offsets)``: the result of an ``ops.predict_maps`` call the caller has already made on these logits and
        sizes (validation at the images' own size scores those bytes); the writer then skips its own call."""
        from .. import ops
        raws = list(batch["raw"])
        S = int(logits.shape[-1])
        sizes = [tuple(int(v) for v in hw) for hw in batch["size"]] if batch.get("size") is not None else [(S, S)] * len(raws)
        if len(sizes) != len(raws) or len(raws) != logits.shape[0]:
            raise ValueError(f"MapWriter.submit: {len(raws)} names, {len(sizes)} sizes, {logits.shape[0]} logit maps")
        st = self.stages[self.batches % 2]
        self._wait_encodes(st)                                   # the encodes of two batches ago read this buffer
        packed, offsets = ops.predict_maps(logits, sizes, minmax=self.minmax) if packed is None else packed
        self._to_host(st.room(packed.numel()), packed)
        st.copied.record()
        st.jobs = [(map_path(self.out_dir, r), h, w, off) for r, (h, w), off in zip(raws, sizes, offsets)]
        self.batches += 1
        self._encode(self.stages[self.batches % 2])              # the previous batch

    @staticmethod
    def _to_host(pinned: torch.Tensor, packed: torch.Tensor) -> None:
        """THE device-to-host copy of a batch (asynchronous: pinned destination)."""
        pinned[:packed.numel()].copy_(packed, non_blocking=True)

    # -------------------------------------------------------------- host side
    def _encode(self, st: _Stage, wait: bool = True) -> None:
        """Hand the batch in ``st`` to the pool (after its copy has landed)."""
        if not st.jobs:
            return
        if wait and st.copied is not None:
            st.copied.synchronize()
        self.put(st, st.pinned.numpy(), st.jobs)
        st.jobs = []

    def put(self, st: _Stage, host, jobs) -> None:
        """Enqueue the encodes of ``jobs`` = ``(path, H, W, offset)`` over the packed bytes ``host`` (a uint8 array that stays
        unchanged until they finish)."""
        pid = os.getpid()
        for path, h, w, off in jobs:
            self._seq += 1
            f = self.pool.submit(encode_png, host[off:off + h * w].data, h, w, path, f"{pid}.{self._seq}")
            st.futures.append(f)
            self._done.append(f)
            self.paths.append(path)

    @staticmethod
    def _wait_encodes(st: _Stage) -> None:
        for f in st.futures:
            f.exception()                                        # wait; errors are raised by close()
        st.futures = []

    def close(self) -> List[str]:
        """Drain: encode the last batch, wait for every encode, stop the threads, raise the first encode error.  Returns ``paths``."""
        try:
            for st in self.stages:                               # only the last batch's stage still holds jobs
                self._encode(st)
            errors = [f.exception() for f in self._done]
        finally:
            self.pool.shutdown(wait=True)
        for e in errors:
            if e is not None:
                raise e
        return self.paths


# ------------------------------------------------------------------------------------------------ scoring a folder of maps
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def _by_stem(folder: str) -> dict:
    return {os.path.splitext(f)[0]: os.path.join(folder, f) for f in sorted(os.listdir(folder)) if f.lower().endswith(IMAGE_EXTENSIONS)}


def _same_size(pred_path: str, gt_path: str) -> None:
    """Headers only: a map whose size differs from its ground truth's is refused before anything is scored."""
    from PIL import Image
    with Image.open(pred_path) as p, Image.open(gt_path) as g:
        if p.size != g.size:
            raise ValueError(f"{pred_path} is {p.size[1]}x{p.size[0]} but its ground truth {gt_path} is {g.size[1]}x{g.size[0]}: evaluation "
                             "toolboxes resize the map here; this package scores each map at its own size and refuses")


def _decode_pair(pred_path: str, gt_path: str):
    import numpy as np
    from PIL import Image
    with Image.open(pred_path) as im:
        p = np.asarray(im.convert("L"))
    with Image.open(gt_path) as im:
        g = np.asarray(im.convert("L"))
    return p, g


def score_maps(pred_dir: str, gt_dir: str, device="cuda", batch: int = 16, workers: int = 8) -> dict:
    """Score a folder of grey-level prediction maps (from any source) against a folder of ground truths, each pair at its own size:
    the ``summary()`` table of the device evaluators (Smeasure, MAE, adpEm, meanEm, maxEm, adpFm, meanFm, maxFm) over every GT of
    ``gt_dir``.  Pairs are matched by file stem and scored in sorted order of the stems; the files are decoded in ``workers`` threads,
    packed (``_lib.predict_maps_layout``), uploaded once per batch of ``batch`` pairs and scored by ``dgtd_sod_metrics_ragged``.  A GT
    without a map raises ``FileNotFoundError`` listing the stems; a map whose size differs from its GT's raises ``ValueError``."""
    from .. import _lib as L
    from ..ops.sod_metrics import RaggedMaps
    from .sod_metrics import SodAccumulator
    preds, gts = _by_stem(os.fspath(pred_dir)), _by_stem(os.fspath(gt_dir))
    missing = [s for s in sorted(gts) if s not in preds]
    if missing:
        raise FileNotFoundError(f"{pred_dir} has no map for {len(missing)} ground truth(s) of {gt_dir}: {', '.join(missing)}")
    stems = sorted(gts)
    if not stems:
        raise FileNotFoundError(f"{gt_dir} holds no image files")
    workers = max(1, min(int(workers), 16))
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="dgtd-score") as pool:
        for f in [pool.submit(_same_size, preds[s], gts[s]) for s in stems]:
            f.result()
    device = torch.device(device)
    if device.type != "cuda":
        raise L.DgtdError("score_maps scores on the HIP device")
    batch = max(1, min(int(batch), L.PREDICT_MAPS_MAX_JOBS))
    acc = SodAccumulator()
    pinned, uploaded = None, torch.cuda.Event()
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="dgtd-score") as pool, torch.cuda.device(device):
        chunks = [stems[i:i + batch] for i in range(0, len(stems), batch)]
        decoding = [pool.submit(_decode_pair, preds[s], gts[s]) for s in chunks[0]]
        for k in range(len(chunks)):
            pairs = [f.result() for f in decoding]
            decoding = [pool.submit(_decode_pair, preds[s], gts[s]) for s in chunks[k + 1]] if k + 1 < len(chunks) else []
            sizes = [p.shape for p, _ in pairs]
            offsets, total = L.predict_maps_layout(sizes)
            half = (total + 255) & ~255                          # [pred maps | gt maps]: ONE upload carries both halves
            if k:
                uploaded.synchronize()                           # the previous upload has read the pinned buffer
            if pinned is None or pinned.numel() < 2 * half:
                pinned = torch.empty(max(1 << 16, 1 << (2 * half - 1).bit_length()), dtype=torch.uint8, pin_memory=True)
            host = pinned.numpy()
            for (p, g), off in zip(pairs, offsets):
                host[off:off + p.size] = p.reshape(-1)
                host[half + off:half + off + g.size] = g.reshape(-1)
            dev = torch.empty(2 * half, dtype=torch.uint8, device=device)
            dev.copy_(pinned[:2 * half], non_blocking=True)
            uploaded.record()
            acc.step(k, RaggedMaps(dev[:total], dev[half:half + total], sizes, offsets))
    return acc.summary()
