"""Synthetic RGB-D batches with the reference datasets' dict contract (twig/dataset/sod_train.py:55-83):
{'raw': str, 'input': [3,S,S] ImageNet-normalised, 'label': [1,S,S] in {0,1}, 'depth': [1,S,S] in [0,1]},
delivered as LISTS of per-sample tensors the way mmengine's pseudo_collate hands them to cod.forward; the sampler; and the device
input pipeline: per image (``device_preprocess``) and per batch of a folder dataset (``DeviceLoader``, stacked tensors)."""
from __future__ import annotations

import torch
import torch.nn.functional as F


class DefaultSampler:
    """mmengine.dataset.DefaultSampler as both configs select it (config/sod.yml:24-26, :35-37): a permutation seeded with
    ``seed + epoch`` (identical on every rank) when ``shuffle``, padded by repetition to a multiple of the world size
    (``round_up``), of which rank r takes ``indices[r::world]``."""

    def __init__(self, length: int, shuffle: bool = True, seed: int = 0, rank: int = 0, world: int = 1, round_up: bool = True):
        self.length, self.shuffle, self.seed, self.rank, self.world, self.round_up = int(length), shuffle, int(seed), rank, world, round_up
        self.epoch = 0
        if round_up:
            self.num_samples = -(-self.length // world)
            self.total_size = self.num_samples * world
        else:
            self.num_samples = -(-(self.length - rank) // world)
            self.total_size = self.length

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return self.num_samples

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            indices = torch.randperm(self.length, generator=g).tolist()
        else:
            indices = list(range(self.length))
        if self.round_up:
            indices = (indices * int(self.total_size / len(indices) + 1))[:self.total_size]
        return iter(indices[self.rank:self.total_size:self.world])


def batches(dataset, sampler, batch_size: int, device=None, drop_last: bool = False):
    """Batches in the form mmengine's pseudo_collate hands to ``cod.forward``: a dict of per-key LISTS of per-sample values."""
    cur = []
    for idx in sampler:
        cur.append(dataset[idx])
        if len(cur) == batch_size:
            yield _collate(cur, device)
            cur = []
    if cur and not drop_last:
        yield _collate(cur, device)


def _collate(items, device):
    out = {}
    for k in items[0]:
        vals = [it[k] for it in items]
        out[k] = [v.to(device, non_blocking=True) for v in vals] if (device is not None and torch.is_tensor(vals[0])) else vals
    return out


from .registry import export  # noqa: E402


@export
class SyntheticRGBD:
    def __init__(self, size: int, batch: int, rank: int = 0, device="cuda", seed: int = 1234, length: int = 1 << 20):
        self.size, self.batch, self.rank, self.device, self.seed, self.length = size, batch, rank, device, seed, length

    def __len__(self) -> int:
        return self.length

    def __getitem__(self, index: int):
        """Dataset view (twig/dataset/sod_train.py:55-83 contract): the sample depends on the index only; which rank sees it is
        the sampler's business."""
        rank, self.rank = self.rank, 0
        try:
            return self.sample(index)
        finally:
            self.rank = rank

    def sample(self, index: int):
        g = torch.Generator(device="cpu").manual_seed(self.seed + self.rank * 10 ** 6 + index)
        S, lo = self.size, max(self.size // 16, 2)
        x = torch.randn(3, S, S, generator=g)
        d = F.interpolate(torch.rand(1, 1, lo, lo, generator=g), size=(S, S), mode="bilinear", align_corners=False)[0]
        l = (F.interpolate(torch.rand(1, 1, lo, lo, generator=g), size=(S, S), mode="bilinear", align_corners=False)[0] > 0.6).float()
        return {"raw": f"synthetic/{self.rank}/{index}.png", "input": x, "label": l, "depth": d.clamp_(0, 1)}

    def batch_at(self, step: int):
        items = [self.sample(step * self.batch + i) for i in range(self.batch)]
        to = lambda k: [it[k].to(self.device, non_blocking=True) for it in items]
        return {"raw": [it["raw"] for it in items], "input": to("input"), "label": to("label"), "depth": to("depth")}


# ------------------------------------------------------------------------------------------------ device-side input pipeline
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def device_preprocess(img_u8: torch.Tensor, size: int, normalize: bool = False, flip: bool = False,
                      out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """One decoded image, uint8 [H, W, C] or [H, W] on the HIP device -> float [C, size, size]: the reference's per-sample transform
    chain RandomHorizontalFlip -> Resize((size, size)) (Pillow BILINEAR, antialiased) -> ToTensor (-> Normalize with the ImageNet
    statistics) of twig/dataset/sod_train.py:31-54, bit-exact, as three small launches (csrc/preprocess_batch.hip)."""
    import ctypes
    from .. import _lib as L
    if img_u8.dtype != torch.uint8 or not img_u8.is_cuda:
        raise L.DgtdError("device_preprocess takes a uint8 image on the HIP device")
    x = img_u8.contiguous()
    if x.ndim == 2:
        x = x.unsqueeze(-1)
    H, W, Cc = x.shape
    out = torch.empty(Cc, size, size, dtype=out_dtype, device=x.device)
    ws = torch.empty(L.load().dgtd_preprocess_workspace(H, W, Cc, size), dtype=torch.uint8, device=x.device)
    if normalize:
        if Cc != 3:
            raise L.DgtdError("Normalize applies to the 3-channel RGB image (sod_train.py:35-36)")
        mean = (ctypes.c_float * 3)(*IMAGENET_MEAN)
        std = (ctypes.c_float * 3)(*IMAGENET_STD)
    else:
        mean = std = None
    L.call("dgtd_preprocess", L.ptr(x), L.ptr(out), mean, std, L.ptr(ws), H, W, Cc, size, int(flip), L.dtype_code(out), L.stream_ptr())
    return out


def device_sample(rgb_u8: torch.Tensor, gt_u8: torch.Tensor, depth_u8: torch.Tensor, size: int, flip: bool,
                  out_dtype: torch.dtype = torch.float32) -> dict:
    """The dict of sod_train.py:76-83 for one sample; ``flip`` is the ONE coin the reference shares between image, GT and depth
    by re-seeding before each transform (:65-75)."""
    return {"input": device_preprocess(rgb_u8, size, True, flip, out_dtype), "label": device_preprocess(gt_u8, size, False, flip, out_dtype),
            "depth": device_preprocess(depth_u8, size, False, flip, out_dtype)}


# ------------------------------------------------------------------------------------------------ batched device input pipeline
class _StageSet:
    """One pinned staging buffer ``[job table | planes]``, its device twin and a workspace, grown on demand (to a power of two of at
    least 1 MiB, so the buffers settle after the first batches) and reused from batch to batch."""

    def __init__(self, device):
        self.device = device
        self.pinned = self.dev = self.ws = None
        self.uploaded = torch.cuda.Event()      # the upload has read the pinned buffer: the host may write the next batch into it
        self.done = torch.cuda.Event()          # the three kernels have run: a consumer stream may read the outputs
        self.busy = False
        self.njobs = self.in_bytes = self.planes_bytes = 0

    @staticmethod
    def _capacity(n: int) -> int:
        return max(1 << 20, 1 << (int(n) - 1).bit_length())

    def pack(self, samples, size: int) -> None:
        """Host side: descriptors and plane bytes of one batch into the pinned buffer.  ``samples``: ``(rgb, gt, depth, flip)`` per
        sample as ``dataset.decode`` returns them."""
        import ctypes
        from .. import _lib as L
        planes, flips, norm, sel, bidx = [], [], [], [], []
        for b, (rgb, gt, dep, flip) in enumerate(samples):
            for arr, s in ((rgb, L.OUT_INPUT), (gt, L.OUT_LABEL), (dep, L.OUT_DEPTH)):
                planes.append(arr if arr.ndim == 3 else arr[:, :, None])
                flips.append(bool(flip)), norm.append(s == L.OUT_INPUT), sel.append(s), bidx.append(b)
        shapes = [p.shape for p in planes]
        lay = L.preprocess_batch_layout(shapes, size)
        table_bytes = len(planes) * ctypes.sizeof(L.PreprocessJob)
        self.njobs, self.planes_bytes, self.ws_bytes = len(planes), lay["planes_bytes"], lay["workspace_bytes"]
        self.table_bytes, self.in_bytes = table_bytes, table_bytes + lay["planes_bytes"]
        if self.busy:
            self.uploaded.synchronize()
        if self.pinned is None or self.pinned.numel() < self.in_bytes:
            self.pinned = torch.empty(self._capacity(self.in_bytes), dtype=torch.uint8, pin_memory=True)
        host = self.pinned.numpy()
        L.fill_preprocess_jobs((L.PreprocessJob * len(planes)).from_buffer(host), shapes, lay, flips, norm, sel, bidx)
        for p, off in zip(planes, lay["src"]):
            host[table_bytes + off: table_bytes + off + p.size] = p.reshape(-1)
        # where each sample's decoded GT plane (plane 3b + 1, one channel, as decoded: never flipped) lies in the staging buffer
        self.gt_planes = [(table_bytes + lay["src"][3 * b + 1], planes[3 * b + 1].size) for b in range(len(samples))]

    def launch(self, batch: int, size: int, out_dtype: torch.dtype, gt8_layout=None):
        """Device side, on the current stream: ONE upload (table and planes together), then the three launches of
        ``dgtd_preprocess_batch`` into fresh output tensors.  ``gt8_layout = (offsets, total)``: a fourth fresh tensor, uint8
        ``[total]``, receives every sample's GT plane at its offset, copied device to device out of the staging buffer (one small
        copy per sample, no second upload), before ``done`` is recorded."""
        import ctypes
        from .. import _lib as L
        if self.dev is None or self.dev.numel() < self.pinned.numel():
            self.dev = torch.empty(self.pinned.numel(), dtype=torch.uint8, device=self.device)
        if self.ws is None or self.ws.numel() < self.ws_bytes:
            self.ws = torch.empty(self._capacity(self.ws_bytes), dtype=torch.uint8, device=self.device)
        self.dev[:self.in_bytes].copy_(self.pinned[:self.in_bytes], non_blocking=True)
        self.uploaded.record()
        self.busy = True
        out = [torch.empty(batch, c, size, size, dtype=out_dtype, device=self.device) for c in (3, 1, 1)]
        mean, std = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
        L.call("dgtd_preprocess_batch", self.dev.data_ptr() + self.table_bytes, self.planes_bytes, self.dev.data_ptr(), self.pinned.data_ptr(),
               self.njobs, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), batch, size, mean, std, self.ws.data_ptr(), self.ws.numel(),
               L.dtype_code(out[0]), L.stream_ptr())
        if gt8_layout is not None:
            offsets, total = gt8_layout
            gt8 = torch.empty(total, dtype=torch.uint8, device=self.device)
            for (src, n), off in zip(self.gt_planes, offsets):
                gt8[off:off + n].copy_(self.dev[src:src + n], non_blocking=True)
            out.append(gt8)
        self.done.record()
        return out


class DeviceLoader:
    """Batches of a folder dataset (``runner.datasets``: anything with ``decode(index, epoch)`` and ``image_size``) preprocessed on the
    device: yields ``{'raw': [paths], 'input': Tensor[B,3,S,S], 'label': Tensor[B,1,S,S], 'depth': Tensor[B,1,S,S]}`` in
    ``out_dtype``, bit-equal to the stacked host path ``dataset[i]``.  Per batch: the decodes run in a pool of
    ``min(num_workers, 16)`` THREADS (never processes: a forked child of a process that holds the GPU is not safe), the decoded
    planes and their job table go through one pinned staging buffer in ONE asynchronous copy, and ``dgtd_preprocess_batch`` writes the
    three batch tensors in three launches; no per-sample tensors, no ``torch.stack``.

    ``prefetch=True``: two staging sets alternate; the decodes of the next two batches are in flight and the upload and kernels of
    batch k+1 are enqueued on a side stream BEFORE batch k is handed out, so they run while batch k trains.  (To enqueue them the
    host waits for batch k+1's decodes first; the decode that overlaps with the training of batch k is batch k+2's, and the first
    yield of an epoch waits for two batches of decode.)  An event orders the consumer's stream behind the preprocess of the batch
    it receives.  ``prefetch=False``: everything on the current stream.

    The yielded tensors are FRESH allocations per batch (only the staging sets are reused), so a consumer may keep them as long as it
    likes.  ``sampler.epoch`` reaches ``decode`` (the flip coin); the last partial batch is yielded unless ``drop_last``.

    ``with_sizes=True`` adds ``'size': [(H, W), ...]`` to the batch dict: the shape of each sample's decoded GT plane before the
    resize, i.e. the resolution a prediction map is written at (``runner.predict.MapWriter``).  The default leaves the dict as it is.

    ``with_gt8=True`` implies ``with_sizes`` and adds ``'gt8'``: a fresh uint8 device tensor per batch holding the decoded GT planes at
    their own size (as decoded, never flipped), packed by ``_lib.predict_maps_layout(batch['size'])`` - the ground-truth half of
    ``ops.RaggedMaps``.  It is filled from the staging buffer that is already on the device, on the stream the preprocess runs on, and
    handed to the consumer's stream like the other outputs.  Without the flag the batch dict and the launches are what they are."""

    def __init__(self, dataset, sampler, batch_size: int, device="cuda", out_dtype: torch.dtype = torch.float32, num_workers: int = 8,
                 prefetch: bool = True, drop_last: bool = False, with_sizes: bool = False, with_gt8: bool = False):
        from concurrent.futures import ThreadPoolExecutor
        from .. import _lib as L
        if not callable(getattr(dataset, "decode", None)):
            raise TypeError("DeviceLoader needs a dataset with decode(index, epoch) (runner.datasets); use batches(...) otherwise")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.DgtdError("DeviceLoader preprocesses on the HIP device; on CPU use batches(...) over the dataset's host path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.dataset, self.sampler, self.batch_size, self.out_dtype = dataset, sampler, int(batch_size), out_dtype
        self.prefetch, self.drop_last, self.size = bool(prefetch), bool(drop_last), int(dataset.image_size)
        self.with_gt8 = bool(with_gt8)
        self.with_sizes = bool(with_sizes) or self.with_gt8
        self.num_threads = max(1, min(int(num_workers), 16))
        self.pool = ThreadPoolExecutor(max_workers=self.num_threads, thread_name_prefix="dgtd-decode")
        self.sets = [_StageSet(self.device), _StageSet(self.device)]
        self.side = torch.cuda.Stream(self.device) if self.prefetch else None

    def close(self) -> None:
        """Stop the decode threads (pending decodes are dropped).  The loader is not usable afterwards."""
        self.pool.shutdown(wait=True, cancel_futures=True)

    def __del__(self):
        pool = getattr(self, "pool", None)
        if pool is not None:
            pool.shutdown(wait=False, cancel_futures=True)

    def __len__(self) -> int:
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _stage(self, k: int, indices, futures):
        """Collect batch k's decodes, pack them and enqueue upload + preprocess (on the side stream when prefetching)."""
        from .. import _lib as L
        st = self.sets[k % 2]
        samples = [f.result() for f in futures]
        st.pack(samples, self.size)
        sizes = [tuple(int(v) for v in gt.shape[:2]) for (_, gt, _, _) in samples]
        layout = L.predict_maps_layout(sizes) if self.with_gt8 else None
        with torch.cuda.device(self.device):
            if self.side is not None:
                with torch.cuda.stream(self.side):
                    out = st.launch(len(indices), self.size, self.out_dtype, layout)
            else:
                out = st.launch(len(indices), self.size, self.out_dtype, layout)
        return [self.dataset.images[i] for i in indices], out, st, sizes

    def _hand_out(self, staged) -> dict:
        raw, out, st, sizes = staged
        if self.side is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(st.done)
            for t in out:
                t.record_stream(cur)        # allocated on the side stream, consumed on this one
        batch = {"raw": raw, "input": out[0], "label": out[1], "depth": out[2]}
        if self.with_sizes or self.with_gt8:
            batch["size"] = sizes
        if self.with_gt8:
            batch["gt8"] = out[3]
        return batch

    def __iter__(self):
        epoch = int(getattr(self.sampler, "epoch", 0))
        idx = list(self.sampler)
        chunks = [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]
        if chunks and self.drop_last and len(chunks[-1]) < self.batch_size:
            chunks.pop()
        decoding, submitted = [], 0

        def fill():
            nonlocal submitted
            while submitted < len(chunks) and len(decoding) < (2 if self.prefetch else 1):
                decoding.append((submitted, chunks[submitted], [self.pool.submit(self.dataset.decode, i, epoch) for i in chunks[submitted]]))
                submitted += 1

        fill()
        staged = self._stage(*decoding.pop(0)) if decoding else None
        while staged is not None:
            fill()
            cur = staged
            if self.prefetch:
                staged = self._stage(*decoding.pop(0)) if decoding else None
                fill()
                yield self._hand_out(cur)
            else:
                yield self._hand_out(cur)
                staged = self._stage(*decoding.pop(0)) if decoding else None
