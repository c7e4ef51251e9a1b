#!/usr/bin/env python3
"""Price the device input pipeline: images/s of the per-sample path (three host-to-device copies + ``device_sample`` per sample, then
``torch.stack``) against the batched path (one upload + ``dgtd_preprocess_batch``), at 480x640 -> 512, batch 8, bf16.

Two legs, both paths alternating inside each repeat:
  * decode excluded: the decoded uint8 arrays already sit in pinned memory; what is timed is packing / copying and the kernels.
  * decode included: PNG files written by this tool to a temporary folder, read through ``runner.datasets.SOD_TRAIN``; the
    per-sample path decodes in the calling thread (what ``batches(...)`` over a device dataset would do), the batched path is
    ``DeviceLoader`` with its decode threads and prefetch.
Every timed window ends in a device synchronise.  Prints one JSON line; ``step_images_per_s`` is the training step's rate from the
README, for comparison.  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgtd  # noqa: E402
from dgtd.runner.data import _StageSet  # noqa: E402

STEP_IMAGES_PER_S = 274.0


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=800, help="batches per timed window of the decode-excluded leg")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--files", type=int, default=64, help="triples written for the decode-included leg")
    ap.add_argument("--epochs", type=int, default=4, help="passes over the files per timed window of the decode-included leg")
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_pipeline needs the HIP device")
    dgtd._lib.load()
    warnings.filterwarnings("ignore", message="The given NumPy array is not writable")     # PIL hands out read-only arrays; nothing writes to them
    H, W, S, B, dt = a.height, a.width, a.size, a.batch, torch.bfloat16
    rng = np.random.default_rng(0)
    arrays = [(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8))
              for _ in range(B)]
    flips = [bool(i % 2) for i in range(B)]
    pinned = [[torch.from_numpy(x).pin_memory() for x in tri] for tri in arrays]
    keep = []                                                     # the last outputs of each path, compared after the timing

    def per_sample():
        items = [dgtd.runner.device_sample(*(t.cuda(non_blocking=True) for t in tri), S, f, dt) for tri, f in zip(pinned, flips)]
        keep[:] = [{k: torch.stack([it[k] for it in items]) for k in ("input", "label", "depth")}]

    st = _StageSet(torch.device("cuda", torch.cuda.current_device()))
    samples = [(p[0].numpy(), p[1].numpy(), p[2].numpy(), f) for p, f in zip(pinned, flips)]

    def batched():
        st.pack(samples, S)
        out = st.launch(B, S, dt)
        keep[1:] = [dict(zip(("input", "label", "depth"), out))]

    per_sample(), batched()
    torch.cuda.synchronize()
    same = all(torch.equal(keep[0][k], keep[1][k]) for k in keep[0])
    res = {"shape": [H, W], "size": S, "batch": B, "dtype": "bf16", "paths_bit_equal": same, "step_images_per_s": STEP_IMAGES_PER_S}
    rates = {"per_sample": [], "batched": []}
    for _ in range(a.repeats):
        rates["per_sample"].append(B * a.iters / timed(per_sample, a.iters))
        rates["batched"].append(B * a.iters / timed(batched, a.iters))
    res["no_decode_images_per_s"] = {k: round(statistics.median(v), 1) for k, v in rates.items()}
    res["no_decode_spread"] = {k: [round(min(v), 1), round(max(v), 1)] for k, v in rates.items()}

    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image
        for d in ("RGB", "GT", "depth"):
            os.makedirs(os.path.join(tmp, d))
        for i in range(a.files):
            # smooth content (a PNG of noise does not compress and would overstate the decode): low-resolution noise, enlarged
            lo = [rng.integers(0, 256, (H // 16, W // 16, c), dtype=np.uint8).squeeze() for c in (3, 1, 1)]
            for d, x in zip(("RGB", "GT", "depth"), lo):
                Image.fromarray(x).resize((W, H), Image.BICUBIC).save(os.path.join(tmp, d, f"{i:04d}.png"))
        ds = dgtd.runner.datasets.SOD_TRAIN(tmp, "depth", "train", S)
        sampler = dgtd.runner.DefaultSampler(len(ds), shuffle=True, seed=0)
        loader = dgtd.runner.DeviceLoader(ds, sampler, B, "cuda", dt, num_workers=a.workers, prefetch=True)

        def per_sample_files():
            cur = []
            for i in sampler:
                rgb, gt, dep, flip = ds.decode(i, sampler.epoch)
                cur.append(dgtd.runner.device_sample(*(torch.from_numpy(x).cuda(non_blocking=True) for x in (rgb, gt, dep)), S, flip, dt))
                if len(cur) == B:
                    keep[:1] = [{k: torch.stack([it[k] for it in cur]) for k in ("input", "label", "depth")}]
                    cur = []

        def batched_files():
            for b in loader:
                keep[1:] = [b]

        per_sample_files(), batched_files()
        rates = {"per_sample": [], "batched": []}
        n = (len(ds) // B) * B
        for _ in range(a.repeats):
            rates["per_sample"].append(n * a.epochs / timed(per_sample_files, a.epochs))
            rates["batched"].append(n * a.epochs / timed(batched_files, a.epochs))
        loader.close()
    res["decode_images_per_s"] = {k: round(statistics.median(v), 1) for k, v in rates.items()}
    res["decode_spread"] = {k: [round(min(v), 1), round(max(v), 1)] for k, v in rates.items()}
    res["decode_threads"] = loader.num_threads
    print(json.dumps(res))


if __name__ == "__main__":
    main()
