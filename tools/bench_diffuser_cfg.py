#!/usr/bin/env python
"""Cost of a texture-diffuser ablation: device time (the library's own HIP-event pairs around each C entry, dgtd_profile_enable) of the
state forward / backward and of the tail at B = 8, S = 512 for the kernels specialised for (12, 7, 4, 24), the run-time parameterised
family at the same point, and other configurations.

    python tools/bench_diffuser_cfg.py [--configs 12,7,4,24 60,11,4,24] [--iters 50] [--batch 8] [--size 512]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dgtd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="*", default=["12,7,4,24", "22,9,6,24", "60,11,4,24"])
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=512)
args = ap.parse_args()
B, S = args.batch, args.size


L = dgtd._lib
g = torch.Generator().manual_seed(0)
x_hp = torch.randn(B, 3, S, S, generator=g).abs().cuda()
depth = torch.rand(B, 1, S, S, generator=g).cuda()
image = torch.randn(B, 3, S, S, generator=g).cuda()
gout = torch.randn(B, 3, S, S, generator=g).cuda()
print(f"B={B} S={S}; mean device us per call over {args.iters} calls")
for cfg in args.configs:
    G, K, steps, LAT = map(int, cfg.split(","))
    T = K * K
    p = [torch.randn(LAT * T, 3, 1, 1, generator=g) / 3 ** 0.5, 0.05 * torch.randn(LAT * T, generator=g), torch.randn(LAT, 1, 1, 1, generator=g),
         0.05 * torch.randn(LAT, generator=g), torch.randn(3, LAT, 1, 1, generator=g) / LAT ** 0.5, 0.05 * torch.randn(3, generator=g)]
    p = [t.cuda().requires_grad_() for t in p]
    families = [("generic", True)] if dgtd.ops.uses_generic(G, K, steps, LAT) else [("specialised", False), ("generic", True)]
    for name, generic in families:
        def step():
            x4 = dgtd.ops.diffuser_state(x_hp, depth, *p[:4], grid=G, k=K, steps=steps, _generic=generic)
            torch.autograd.grad(dgtd.ops.diffuse_tail(x4, p[4], p[5], image, _generic=generic), p, gout)

        for _ in range(5):
            step()
        torch.cuda.synchronize()
        L.profile_native(True)
        for _ in range(args.iters):
            step()
            L.load().dgtd_profile_empty(L.stream_ptr())     # the event pair's own floor, carried by every figure
        prof = L.profile_native_summary()
        L.profile_native(False)
        us = {}
        for key, e in prof.items():
            us[key.split("[")[0].replace("dgtd_", "").replace("_cfg", "")] = 1e3 * e["ms"] / e["calls"]
        print(f"({G:2d},{K:2d},{steps:2d},{LAT:2d}) {name:11s}  " + "  ".join(f"{k} {us[k]:8.1f}" for k in ("diffuser_fwd", "diffuser_bwd", "diffuse_tail_fwd", "diffuse_tail_bwd", "profile_empty")))
