"""What custom_hooks: EMAHook costs in FlatAdamW.step(): the real model's buckets (dgtd.nn.cod, 114 M parameters) with random gradients,
bf16 and fp16 + loss scaler, each with the average off, fused into the AdamW launches (dgtd_adamw_flat_ema: +8 B/element) and standalone
(the step without it followed by one dgtd_ema_flat per bucket: +12 B/element).  The step alone is timed (no forward / backward) with HIP
events over back-to-back steps after a warm-up, the variants interleaved round by round in one process, median and minimum; then one
profiled step per variant gives the device time of the launches and their share of the HBM rate.
    python tools/bench_ema.py [--rounds 7] [--iters 20]"""
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
        off_opt = dgtd.runner.FlatAdamW(red, lr=0.0, scaler=scaler, graph_safe=True)
        fused = dgtd.runner.FlatAdamW(red, lr=0.0, scaler=scaler, graph_safe=True, ema={"type": "EMAHook", "momentum": 0.0002})
        coef = torch.tensor([0.0002], device="cuda")      # the standalone form reads a coefficient of its own: a real update every step
        avgs = [torch.zeros_like(b["mflat"]) for b in red.buckets]

        def standalone():
            off_opt.step()
            for b, e in zip(red.buckets, avgs):
                L.call("dgtd_ema_flat", b["mflat"].data_ptr(), e.data_ptr(), e.numel(), coef.data_ptr(), L.stream_ptr())

        variants = {"off": off_opt.step, "fused": fused.step, "standalone": standalone}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert fused.ema_steps == 3 and 0.0 < fused.ema_state[0].item() < 1.0, "the fused form should be past its first (copying) update"
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timeit(fn, args.iters))
        name = "bf16" if dtype == torch.bfloat16 else "fp16 + loss scaler"
        runs = sum(len(r) for r in off_opt.runs)
        padded = sum(b["mflat"].numel() for b in red.buckets)
        print(f"{name}: {n / 1e6:.1f} M parameters ({padded / 1e6:.1f} M elements with padding) in {len(red.buckets)} buckets, "
              f"{runs} AdamW launches per step")
        base = statistics.median(times["off"])
        for k, v in times.items():
            med = statistics.median(v)
            extra = {"off": 0.0, "fused": 8.0, "standalone": 12.0}[k] * padded
            rate = f", extra traffic {extra / 1e9:.2f} GB at {extra / ((med - base) * 1e-3) / 1e12:.2f} TB/s" if med > base and extra else ""
            print(f"  ema {k:10s}: step median {med:.4f} ms  min {min(v):.4f} ms  ({med - base:+.4f} ms, {100.0 * (med - base) / base:+.1f} % vs off{rate})")
        for k, fn in variants.items():
            L.profile_native(True)
            fn()
            summ = L.profile_native_summary()
            L.profile_native(False)
            for key in ("dgtd_adamw_flat", "dgtd_ema_flat", "dgtd_ema_schedule", "dgtd_found_inf"):
                rec = [e for kk, e in summ.items() if kk.startswith(key)]
                if rec:
                    ms, amount, calls = sum(e["ms"] for e in rec), sum(e["amount"] for e in rec), sum(e["calls"] for e in rec)
                    print(f"  profiled step, ema {k:10s}: {key:18s} {calls:3d} launches {ms:.4f} ms  {amount / 1e6:8.1f} MB  "
                          f"{amount / (ms * 1e-3) / 1e9:7.1f} GB/s = {100.0 * amount / (ms * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")
        del variants, off_opt, fused, avgs, red, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
