"""GPU: routing of the Linear weight gradients to the package's own kernel (dgtd_gemm_wgrad_batched, csrc/gemm_wgrad.hip) behind the
process-wide switch DGTD_OWN_WGRAD / set_own_wgrad(): the deferred strided-batched runs (flush_gemms) and the per-layer path (gemm_dw)
of csrc_torch/bindings.cpp."""
import gc
import math

import pytest
import torch

from oracle import filler

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


def test_own_wgrad_matches_library_path_in_the_model(dgtd):
    """The body of test_batched_weight_gradient_gemms_match_per_layer_path (S = 64, B = 2, bf16, no DropPath, reducer, two steps), once
    with the switch off and once with it on.  The kernel runs only with the switch on; at S = 64 the last two ConvNeXt stages have
    M = 32 and 8 tokens, which dgtd_gemm_wgrad_supported refuses, so they must fall back to the library path.  The 152 Linear weight
    gradients agree to rel-L2 < 1e-2 and all gradients to rtol 3e-2 / atol 1e-5: the bounds that test uses between its two library
    paths (16-bit rounding differences between two correct accumulation orders).  Nothing stays parked, the arenas die with the model."""
    from dgtd.ops import _native as N
    nat = N.ops()
    assert nat is not None
    assert N.BATCH_WGRAD
    S, B = 64, 2
    x, d, l = (t.cuda() for t in filler.synthetic_batch(B, S, seed=5))
    grads, calls, fallbacks = {}, {}, {}
    base = nat.arena_bytes()
    was = nat.own_wgrad()
    try:
        for own in (False, True):
            N.set_own_wgrad(own)
            assert nat.own_wgrad() == own and N.OWN_WGRAD == own
            net = dgtd.nn.cod(drop_path_rate=0.0, compute_dtype=torch.bfloat16)
            filler.fill_module(net)
            net = net.cuda().train()
            red = dgtd.dist.GradReducer(net, working_dtype=torch.bfloat16)
            c0, f0 = nat.own_wgrad_calls(), nat.own_wgrad_fallbacks()
            for _ in range(2):                                       # second step reuses the arenas
                red.zero_grad()
                loss = net(None, x, l, d, mode="loss")["loss"]
                loss.backward()
                red.finish()
            assert nat.pending_reductions() == 0
            calls[own], fallbacks[own] = nat.own_wgrad_calls() - c0, nat.own_wgrad_fallbacks() - f0
            grads[own] = {k: p.grad.float().clone() for k, p in net.named_parameters() if p.grad is not None}
            assert nat.arena_bytes() > base
            del net, red, loss
            gc.collect()
    finally:
        N.set_own_wgrad(was)
    assert nat.arena_bytes() == base, "arenas must die with the model"
    assert calls[False] == 0 and fallbacks[False] == 0, (calls, fallbacks)
    # per step at least pwconv1 + pwconv2 of ConvNeXt stages 0 and 1 (512 and 128 tokens) on the kernel, and of stages 2 and 3 (32 and 8) refused
    assert calls[True] >= 2 * 4, calls
    assert fallbacks[True] >= 2 * 4, fallbacks
    pw = [k for k in grads[True] if k.endswith("weight") and (".pwconv" in k or (".block" in k and any(t in k for t in (".attn.q.", ".attn.kv.", ".attn.proj.", ".mlp.fc1.", ".mlp.fc2."))))]
    assert len(pw) == 72 + 80, len(pw)
    assert set(grads[True]) == set(grads[False])
    for k in pw:
        a, b = grads[True][k], grads[False][k]
        assert (a - b).norm() / b.norm() < 1e-2, k
    for k in grads[True]:
        torch.testing.assert_close(grads[True][k], grads[False][k], rtol=3e-2, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


def test_own_wgrad_in_a_captured_step(dgtd):
    """One GraphedTrainStep capture and three replays with the switch on (S = 64, B = 2, bf16: the size and the tolerance of
    test_graphed_step_matches_eager): the workspace is allocated at the call, so the kernel is capturable; losses are finite and
    follow an eager run with the switch on."""
    from dgtd.ops import _native as N
    nat = N.ops()
    assert nat is not None
    S, B, W = 64, 2, 2
    dtype = torch.bfloat16
    data = dgtd.runner.SyntheticRGBD(S, B, device="cuda")
    batches = [data.batch_at(i) for i in range(3)]

    def make():
        torch.manual_seed(0)
        net = dgtd.nn.cod(drop_path_rate=0.0, compute_dtype=dtype)
        filler.fill_module(net)
        net = net.cuda().train()
        red = dgtd.dist.GradReducer(net, working_dtype=dtype)
        opt = dgtd.runner.FlatAdamW(red, lr=1e-4, graph_safe=True)
        return net, red, opt

    was = nat.own_wgrad()
    try:
        N.set_own_wgrad(True)
        net_e, red_e, opt_e = make()
        c0 = nat.own_wgrad_calls()
        want = []
        for i in range(3):
            red_e.zero_grad()
            loss = net_e(batches[i]["raw"], batches[i]["input"], batches[i]["label"], batches[i]["depth"], mode="loss")["loss"]
            loss.backward()
            red_e.finish()
            opt_e.sync_lr()
            opt_e.step()
            want.append(loss.item())
        assert nat.own_wgrad_calls() - c0 >= 3 * 4

        net_g, red_g, opt_g = make()
        stepper = dgtd.runner.GraphedTrainStep(net_g, red_g, opt_g, warmup=W)
        c1 = nat.own_wgrad_calls()
        stepper.capture(batches[0])
        assert nat.own_wgrad_calls() - c1 >= 4, "the captured step did not go through the own kernel"
        got = [stepper(batches[i]).item() for i in range(3)]
        torch.cuda.synchronize()
        assert opt_g.steps == opt_e.steps == 3
        for a_, b_ in zip(got, want):
            assert math.isfinite(a_) and abs(a_ - b_) <= 2e-2 * max(1.0, abs(b_)), (got, want)
        if hasattr(stepper, "release"):
            stepper.release()
    finally:
        N.set_own_wgrad(was)
