"""The stand-in model of tests/test_clip_grad_gpu.py, and - run as a program - the subprocess body of its fused-communication test:
a world-1 RCCL process group (DGTD_FORCE_ALLREDUCE=1) so the N > 1 form of the captured step (collectives inside the graph, AdamW
joining bucket after bucket: ``comm="fused"``) runs with clip_grad by norm on a one-GPU box, against the eager step.
Prints one JSON line: losses and gradient norms of both."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stand_in(dgtd, dtype):
    """What GraphedTrainStep uses of dgtd.nn.cod - ``high_pass(input)`` and ``forward(None, input, label, depth, mode="loss", x_hp=...)
    -> {"loss": ...}`` - around a few dgtd.nn layers on 8x8 token maps [B, 64, 128]."""
    import torch

    class StandIn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.shared = dgtd.nn.Linear(128, 128)
            self.norm = dgtd.nn.LayerNorm(128, eps=1e-6)
            self.dw = dgtd.nn.DWConv(128)
            self.out = dgtd.nn.Linear(128, 128)

        def high_pass(self, input):
            return 0.5 * input.float()

        def _trunk(self, x):
            h = self.shared(self.shared(x))
            h = self.dw(self.norm(h), 8, 8, gelu=True)
            return dgtd.ops.linear_residual(h, *dgtd.nn.wb(self.out), x, None)

        def forward(self, raw, input, label, depth, mode="loss", x_hp=None):
            x = input + (self.high_pass(input) if x_hp is None else x_hp) + depth
            if dtype == torch.float32:
                y = self._trunk(x)
            else:
                with torch.autocast("cuda", dtype=dtype):
                    y = self._trunk(x.to(dtype))
            return {"loss": ((y.float() - label) ** 2).mean()}

    torch.manual_seed(3)
    return StandIn().cuda().train()


def batches(n, B=2):
    """Batches of growing magnitude, so the gradient norm differs from step to step."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda: torch.randn(B, 64, 128, device="cuda", generator=g)
    return [{"input": rnd() * (1.0 + 0.5 * i), "label": rnd(), "depth": 0.1 * rnd()} for i in range(n)]


def eager_step(net, red, opt, b):
    red.zero_grad()
    loss = net(None, b["input"], b["label"], b["depth"], mode="loss")["loss"]
    loss.backward()
    red.finish()
    opt.sync_lr()
    opt.step()
    return loss.item(), opt.grad_norm()


def main():
    os.environ["DGTD_FORCE_ALLREDUCE"] = "1"
    os.environ.setdefault("MIOPEN_DEBUG_CONV_WINOGRAD", "0")
    os.environ.setdefault("DGTD_GEMM_CANDIDATES", "4")
    os.environ.setdefault("MASTER_PORT", sys.argv[1])
    sys.path.insert(0, ROOT)
    import torch
    import dgtd
    rank, local, world = dgtd.dist.init_process_group()
    assert world == 1 and torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl"
    dtype = torch.bfloat16
    data = batches(3)

    def make(clip):
        net = stand_in(dgtd, dtype)
        red = dgtd.dist.GradReducer(net, bucket_bytes=32 << 10, working_dtype=dtype, exclude_prefixes=())
        assert red._force and red.overlap and red.comm_stream is not None and len(red.buckets) >= 2 and red.comm16
        return net, red, dgtd.runner.FlatAdamW(red, lr=1e-3, custom_keys={}, graph_safe=True, clip_grad=clip)

    probe = make({"max_norm": 1e30})
    clip = {"max_norm": 0.5 * eager_step(*probe, data[0])[1], "norm_type": 2}      # half the first step's norm: clipping is active
    del probe
    net_e, red_e, opt_e = make(clip)
    eager = [eager_step(net_e, red_e, opt_e, b) for b in data]
    print("eager done", flush=True)
    net_g, red_g, opt_g = make(clip)
    stepper = dgtd.runner.GraphedTrainStep(net_g, red_g, opt_g, warmup=1, comm="fused")
    stepper.capture(data[0])
    assert stepper.mode == "fused" and stepper.graph_opt is None
    print("fused: captured", flush=True)
    fused = []
    for b in data:
        loss = stepper(b).item()
        fused.append((loss, opt_g.grad_norm()))
    torch.cuda.synchronize()
    out = {"max_norm": clip["max_norm"], "steps": opt_g.steps,
           "eager": {"losses": [l for l, _ in eager], "norms": [n for _, n in eager]},
           "fused": {"losses": [l for l, _ in fused], "norms": [n for _, n in fused]}}
    assert all(math.isfinite(v) for v in out["fused"]["losses"])
    stepper.release()
    print("RESULT " + json.dumps(out), flush=True)
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
