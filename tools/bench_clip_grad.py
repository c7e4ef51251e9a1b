"""What optim_wrapper.clip_grad costs in FlatAdamW.step(): the real model's buckets (dgtd.nn.cod, 114 M parameters) with random
gradients, bf16 and fp16 + loss scaler, each with clipping off, by norm and by value.  The step alone is timed (no forward / backward)
with HIP events over back-to-back steps after a warm-up, the variants interleaved round by round in one process, median and minimum;
then one profiled step per mode gives the device time of the norm launches and their share of the HBM rate.
    python tools/bench_clip_grad.py [--rounds 7] [--iters 20]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dgtd  # noqa: E402

L = dgtd._lib
HBM_PEAK = 8.0e12


def timeit(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters     # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    for dtype in (torch.bfloat16, torch.float16):
        torch.manual_seed(0)
        net = dgtd.nn.cod(compute_dtype=dtype).cuda().train()
        red = dgtd.dist.GradReducer(net, working_dtype=dtype)
        scaler = dgtd.runner.LossScaler("cuda") if dtype == torch.float16 else None
        scale = scaler.get_scale() if scaler is not None else 1.0
        n = 0
        for b in red.buckets:               # gradients in the parameters' slots only: the alignment padding stays zero
            for off, size in zip(b["offsets"], b["sizes"]):
                b["flat"][off:off + size].copy_(torch.randn(size, device="cuda") * (1e-3 * scale))
                n += size
        # lr 0: the masters stay where they are however many steps are timed; the kernels do the same work
        variants = {"off": None, "norm": {"max_norm": 1.0, "norm_type": 2}, "value": {"type": "value", "clip_value": 5e-4}}
        opts = {k: dgtd.runner.FlatAdamW(red, lr=0.0, scaler=scaler, graph_safe=True, clip_grad=v) for k, v in variants.items()}
        for o in opts.values():
            for _ in range(3):
                o.step()
        torch.cuda.synchronize()
        assert opts["norm"]._clip_state[1].item() < 1.0, "the coefficient should be at work"
        times = {k: [] for k in opts}
        for _ in range(args.rounds):
            for k, o in opts.items():
                times[k].append(timeit(o.step, args.iters))
        name = "bf16" if dtype == torch.bfloat16 else "fp16 + loss scaler"
        runs = sum(len(r) for r in opts["off"].runs)
        print(f"{name}: {n / 1e6:.1f} M gradient elements in {len(red.buckets)} buckets, {runs} AdamW launches per step, "
              f"grad_norm {opts['norm'].grad_norm():.4f}, steps taken {opts['norm'].steps}")
        base = statistics.median(times["off"])
        for k, v in times.items():
            med = statistics.median(v)
            print(f"  clip {k:5s}: FlatAdamW.step() median {med:.4f} ms  min {min(v):.4f} ms  ({med - base:+.4f} ms, {100.0 * (med - base) / base:+.1f} % vs off)")
        for k in ("off", "norm"):
            L.profile_native(True)
            opts[k].step()
            summ = L.profile_native_summary()
            L.profile_native(False)
            for key in ("dgtd_grad_norm_partial", "dgtd_grad_clip_finalize", "dgtd_found_inf", "dgtd_adamw_flat"):
                rec = [e for kk, e in summ.items() if kk.startswith(key)]
                if rec:
                    ms, amount, calls = sum(e["ms"] for e in rec), sum(e["amount"] for e in rec), sum(e["calls"] for e in rec)
                    print(f"  profiled step, clip {k:4s}: {key:24s} {calls:3d} launches {ms:.4f} ms  {amount / 1e6:8.1f} MB  "
                          f"{amount / (ms * 1e-3) / 1e9:7.1f} GB/s = {100.0 * amount / (ms * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")
        del opts, red, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
