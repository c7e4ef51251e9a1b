#!/usr/bin/env python3
"""Price the output tail of prediction: a batch of 8 logit maps at 384x384 -> eight grey-level maps of different sizes around 480x640
on the host (and, in the second leg, as PNG files).

Two paths, alternating inside each repeat, every timed window ending in a device synchronise, median of ``--repeats`` windows:
  * torch: per sample ``F.interpolate(bilinear) -> sigmoid -> mul(255) -> add(0.5) -> clamp(0, 255) -> to(uint8) -> .cpu()`` (what a user
    would write after ``mode='tensor'``); with the encode, ``PIL.Image.fromarray(...).save`` per sample in the calling thread.
  * ours: ``ops.predict_maps`` (one launch) + ONE device-to-host copy into pinned memory; with the encode, ``runner.MapWriter`` (the
    copy of batch k and the encode of batch k-1 overlap whatever the device does next).
``forward_ms`` is ``cod.forward(mode='tensor')`` of the same batch (bf16, eval, random weights), the work the tail follows.
Prints one JSON line.  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgtd  # noqa: E402

SIZES = [(480, 640), (427, 640), (640, 480), (500, 375), (375, 500), (480, 639), (333, 500), (600, 800)]


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--iters", type=int, default=200, help="batches per timed window without the encode")
    ap.add_argument("--png-iters", type=int, default=20, help="batches per timed window with the encode")
    ap.add_argument("--forward-iters", type=int, default=10, help="forwards per timed window (0: skip the forward)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict_maps needs the HIP device")
    dgtd._lib.load()
    from PIL import Image
    S, B = a.size, len(SIZES)
    g = torch.Generator().manual_seed(0)
    lo = torch.randn(B, 1, S // 16, S // 16, generator=g) * 4.0          # smooth maps, as a model's are (noise would overstate the PNG encode)
    logits = F.interpolate(lo, size=(S, S), mode="bicubic", align_corners=False).cuda().contiguous()
    offsets, total = dgtd._lib.predict_maps_layout(SIZES)
    pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    keep = {}

    def torch_maps():
        keep["torch"] = [F.interpolate(logits[i:i + 1], size=hw, mode="bilinear", align_corners=False).sigmoid().mul(255).add(0.5).clamp(0, 255)
                         .to(torch.uint8).cpu() for i, hw in enumerate(SIZES)]

    def our_maps():
        packed, _ = dgtd.ops.predict_maps(logits, SIZES)
        pinned.copy_(packed, non_blocking=True)

    torch_maps(), our_maps()
    torch.cuda.synchronize()
    diff = [int((t[0, 0].numpy().astype(np.int16) - pinned[o:o + h * w].reshape(h, w).numpy().astype(np.int16)).__abs__().max())
            for t, (h, w), o in zip(keep["torch"], SIZES, offsets)]
    differing = sum(int((t[0, 0].numpy() != pinned[o:o + h * w].reshape(h, w).numpy()).sum()) for t, (h, w), o in zip(keep["torch"], SIZES, offsets))
    res = {"logits": [B, S, S], "sizes": SIZES, "bytes_out": sum(h * w for h, w in SIZES), "max_level_diff_vs_torch": max(diff),
           "bytes_differing_vs_torch": differing}
    ms = {"torch": [], "ours": []}
    for _ in range(a.repeats):
        ms["torch"].append(timed(torch_maps, a.iters))
        ms["ours"].append(timed(our_maps, a.iters))
    res["no_encode_ms_per_batch"] = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    res["no_encode_spread"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}

    with tempfile.TemporaryDirectory() as tmp:
        batch = {"raw": [f"img_{i}.jpg" for i in range(B)], "size": SIZES}

        def torch_png():
            torch_maps()
            for i, t in enumerate(keep["torch"]):
                Image.fromarray(t[0, 0].numpy()).save(os.path.join(tmp, "torch", f"img_{i}.png"))

        def our_window(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = dgtd.runner.MapWriter(os.path.join(tmp, "ours"), workers=a.workers)
            for _ in range(iters):
                w.submit(batch, logits)
            w.close()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / iters

        os.makedirs(os.path.join(tmp, "torch"))
        torch_png(), our_window(2)
        ms = {"torch": [], "ours": []}
        for _ in range(a.repeats):
            ms["torch"].append(timed(torch_png, a.png_iters))
            ms["ours"].append(our_window(a.png_iters))
    res["with_encode_ms_per_batch"] = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    res["with_encode_spread"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}
    res["encode_threads"] = max(1, min(a.workers, 16))

    if a.forward_iters:
        torch.manual_seed(0)
        net = dgtd.nn.cod(img_size=S, compute_dtype=torch.bfloat16, drop_path_rate=0.0).cuda().eval()
        b = dgtd.runner.SyntheticRGBD(S, B).batch_at(0)
        x, l, d = (torch.stack(b[k]) for k in ("input", "label", "depth"))
        with torch.no_grad():
            fwd = lambda: net(None, x, l, d, mode="tensor")
            out = fwd()
            res["forward_logits_dtype"] = str(out.dtype).replace("torch.", "")
            timed(fwd, 3)
            res["forward_ms"] = round(statistics.median(timed(fwd, a.forward_iters) for _ in range(a.repeats)), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
