#!/usr/bin/env python3
"""Price the scoring of a validation batch at each image's own size: 16 maps with sides drawn from 300-1100 (seeded).

Two paths over the same batch, in alternating windows inside one call, each window timed with device events after a warm-up, median
and [min, max] of ``--repeats`` windows:
  * ragged: ``ops.predict_maps`` (16 logit maps -> packed bytes) -> ``dgtd_sod_metrics_ragged`` -> ``dgtd_sod_metrics_accumulate``, the
    chain ``val_cfg: {score_size: original}`` runs per batch; also without the ``predict_maps`` leg.
  * loop:   per image ``dgtd_sod_metrics(B=1)`` on float maps of the same sizes (already on the device) -> accumulate - the only way
    to score ragged sizes without the ragged entry.  The dense entry is the same code before and after the ragged entry was added.
Both are run on smooth maps (a sigmoid of up-sampled noise) and on saturated maps (every pixel 0 or 255, the case that serialises a
histogram on two bins).  Prints one JSON line.  Needs the GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dgtd  # noqa: E402


def window(fn, iters):
    """ms per call of ``fn`` over ``iters`` back-to-back calls, between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=384, help="side of the logit maps")
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50, help="batches per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score_size needs the HIP device")
    dgtd._lib.load()
    S, n = a.size, a.maps
    M = sys.modules[dgtd.ops.__name__ + ".sod_metrics"]     # the module (dgtd.ops.sod_metrics is the function of that name)
    rng = np.random.default_rng(0)
    sizes = [(int(h), int(w)) for h, w in rng.integers(300, 1101, (n, 2))]
    g = torch.Generator().manual_seed(0)
    res = {"maps": n, "logits": [n, S, S], "sizes": sizes, "pixels": sum(h * w for h, w in sizes), "iters": a.iters, "repeats": a.repeats}
    for kind in ("smooth", "saturated"):
        lo = torch.randn(n, 1, S // 16, S // 16, generator=g) * (4.0 if kind == "smooth" else 4000.0)   # x1000: the sigmoid saturates
        logits = F.interpolate(lo, size=(S, S), mode="bicubic", align_corners=False).cuda().contiguous()
        glo = torch.randn(n, 1, 6, 6, generator=g)
        offsets, total = dgtd._lib.predict_maps_layout(sizes)
        packed, _ = dgtd.ops.predict_maps(logits, sizes)
        gt8 = torch.zeros(total, dtype=torch.uint8, device="cuda")
        pf, gf = [], []
        for j, ((h, w), off) in enumerate(zip(sizes, offsets)):
            gj = (F.interpolate(glo[j:j + 1], size=(h, w), mode="bilinear", align_corners=False)[0, 0] > 0.3).cuda()
            gt8[off:off + h * w] = (gj.to(torch.uint8) * 255).reshape(-1)
            gf.append(gj.float()[None].contiguous())
            pf.append(((packed[off:off + h * w].float() + 0.5) / 255).reshape(1, h, w).contiguous())   # quantises back to the same bytes
        state, slot = torch.zeros(M.STATE, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
        keep = {}

        def ragged_chain():
            p8, _ = dgtd.ops.predict_maps(logits, sizes)
            keep["ragged"] = M.sod_metrics_ragged_rows(M.RaggedMaps(p8, gt8, sizes, offsets))
            M.sod_metrics_accumulate(keep["ragged"], state, slot)

        def ragged_metrics():
            keep["ragged"] = M.sod_metrics_ragged_rows(M.RaggedMaps(packed, gt8, sizes, offsets))
            M.sod_metrics_accumulate(keep["ragged"], state, slot)

        def dense_loop():
            rows = [M.sod_metrics_rows(p, t) for p, t in zip(pf, gf)]
            for r in rows:
                M.sod_metrics_accumulate(r, state, slot)
            keep["loop"] = rows

        paths = {"ragged_chain": ragged_chain, "ragged_metrics_only": ragged_metrics, "dense_loop": dense_loop}
        for fn in paths.values():                                 # warm-up of every shape the windows use
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(keep["ragged"], torch.cat(keep["loop"])))
        hist = torch.bincount(packed.long(), minlength=256)
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):                                # alternating windows
            for k, fn in paths.items():
                ms[k].append(window(fn, a.iters))
        res[kind] = {"share_of_bytes_in_bins_0_and_255": round(float(hist[0] + hist[255]) / float(hist.sum()), 4), "rows_equal_dense_loop": same,
                     "ms_per_batch": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                     "spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
