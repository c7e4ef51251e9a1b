"""csrc/gemm_wgrad.hip against the library path of the deferred weight-gradient phase (flush_gemms in csrc_torch/bindings.cpp: hipBLASLt
strided-batched GEMM, with its token split into 16-bit partials + sum where it applies) at the model's weight-gradient shapes (config 2:
512x512, batch 8).  Both paths run through the same binding entry (torch.ops.dgtd.wgrad_batched) in one process, the switch flipped in
between; device time from HIP events over back-to-back launches after a warm-up, interleaved rounds, median.
    python tools/bench_wgrad_own.py [--rounds 5] [--iters 10] [--dtype bf16]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dgtd  # noqa: E402
from dgtd.ops import _native as NAT  # noqa: E402

L = dgtd._lib


def shapes():
    """(name, batch, M, N, K): dW[N,K] = dY[M,N]^T X[M,K] for `batch` layers of one run"""
    out = []
    for st, (b, M, C) in enumerate([(3, 131072, 128), (3, 32768, 256), (27, 8192, 512), (3, 2048, 1024)]):
        out += [(f"cnx{st}.pwconv1", b, M, 4 * C, C), (f"cnx{st}.pwconv2", b, M, C, 4 * C)]
    for st, (b, M, C, r) in enumerate([(3, 131072, 64, 8), (4, 32768, 128, 8), (6, 8192, 320, 4), (3, 2048, 512, 4)], 1):
        out += [(f"pvt{st}.q", b, M, C, C), (f"pvt{st}.kv", b, 2048, 2 * C, C), (f"pvt{st}.proj", b, M, C, C),
                (f"pvt{st}.fc1", b, M, r * C, C), (f"pvt{st}.fc2", b, M, C, r * C)]
    return out


def timeit(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters     # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    code = L.dtype_code(torch.empty(1, dtype=dt))
    nat = NAT.ops()
    assert nat is not None, "the C++ bindings are needed: both paths are routed there"
    lib = L.load()
    was = nat.own_wgrad()
    print(f"{'shape':13s} {'b':>2s} {'M':>6s} {'N':>4s} {'K':>4s} {'S':>2s} | {'own us':>8s} {'TF/s':>5s} {'GB/s':>5s} | {'lib us':>8s} {'TF/s':>5s} | lib/own | rel-L2 own vs lib, max |own - fp32| / max |fp32|")
    tot_own = tot_lib = 0.0
    try:
        for name, b, M, N, K in shapes():
            torch.manual_seed(0)
            dy = (torch.randn(b, M, N, device="cuda") * 0.1).to(dt)
            x = (torch.randn(b, M, K, device="cuda") * 0.5).to(dt)
            assert lib.dgtd_gemm_wgrad_supported(M, N, K, code), (name, M, N, K)
            S = lib.dgtd_gemm_wgrad_workspace(b, M, N, K) // (b * N * K * 4)
            calls = nat.own_wgrad_calls()

            def own():
                nat.set_own_wgrad(True)
                return nat.wgrad_batched(dy, x)

            def libp():
                nat.set_own_wgrad(False)
                return nat.wgrad_batched(dy, x)

            d_own, d_lib = own().float(), libp().float()
            assert nat.own_wgrad_calls() == calls + 1, "the own kernel did not run"
            ref = dy[0].float().t() @ x[0].float()
            rel = float((d_own - d_lib).norm() / d_lib.norm())
            e32 = float((d_own[0] - ref).abs().max() / ref.abs().max())
            del d_own, d_lib, ref
            t_own, t_lib = [], []
            for _ in range(args.rounds):
                t_own.append(timeit(own, args.iters))
                t_lib.append(timeit(libp, args.iters))
            to, tl = sorted(t_own)[len(t_own) // 2], sorted(t_lib)[len(t_lib) // 2]
            fl, by = 2.0 * b * M * N * K, 2.0 * b * (M * N + M * K + N * K)
            tot_own += to
            tot_lib += tl
            print(f"{name:13s} {b:2d} {M:6d} {N:4d} {K:4d} {S:2d} | {to:8.1f} {fl / to / 1e6:5.0f} {by / to / 1e3:5.0f} | {tl:8.1f} {fl / tl / 1e6:5.0f} | {tl / to:7.2f} | {rel:.2e} {e32:.2e}",
                  flush=True)
            del dy, x
    finally:
        nat.set_own_wgrad(was)
    print(f"sum: own {tot_own:.0f} us, library {tot_lib:.0f} us")


if __name__ == "__main__":
    main()
