"""GPU: the ``diffuser`` option through the modules - whole-model parity against the patched oracle, the modules honouring their own
arguments, and a non-default configuration inside the captured training step."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cod_cpu, filler

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3       # the project's fp32 gate, as in tests/test_model_gpu.py
PE = "hitnet.backbone.prompt_encoder."
DIFFUSER_PARAMS = [PE + n for n in ("propagation_weight_regressor.reg.weight", "propagation_weight_regressor.reg.bias", "encoder1.weight",
                                    "encoder1.bias", "message_passing.conv.weight", "message_passing.conv.bias")]


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


def test_whole_model_vs_patched_oracle(dgtd, monkeypatch):
    """cod(diffuser={grid: 9, k: 5, max_step: 2}) at 64^2, fp32, against the oracle's whole model with DIFFUSE_GRID / K / STEPS patched
    (its LATENT stays 24: the oracle ties it to the decoders).  Eval logits within 1e-3; train-mode loss and the six diffuser
    parameter gradients at the bound of tests/test_model_gpu.py::test_whole_model_train_loss_and_grads (gradient norms, 2e-2 for the
    two tensors whose gradient is a cancelling sum over every pixel, 2e-3 otherwise)."""
    S, B = 64, 2
    monkeypatch.setattr(cod_cpu, "DIFFUSE_GRID", 9)
    monkeypatch.setattr(cod_cpu, "DIFFUSE_K", 5)
    monkeypatch.setattr(cod_cpu, "DIFFUSE_STEPS", 2)
    ref = cod_cpu.cod(S)
    filler.fill_module(ref)
    net = dgtd.nn.cod(img_size=S, compute_dtype=torch.float32, drop_path_rate=0.0, diffuser={"grid": 9, "k": 5, "max_step": 2})
    net.load_state_dict(ref.state_dict())
    net = net.cuda()
    assert net.hitnet.backbone.prompt_encoder.propagation_weight_regressor.reg.weight.shape == (24 * 25, 3, 1, 1)
    x, d, l = filler.synthetic_batch(B, S, seed=S)

    ref.eval(), net.eval()
    with torch.no_grad():
        _, P1r, P2r = ref.hitnet(x, d)
        _, P1, P2 = net.hitnet(x.cuda(), d.cuda())
    ref_logit, logit = (P1r[-1] + P2r).numpy(), (P1[-1] + P2).cpu().numpy()
    print(f"  eval logits: max |diff| {np.abs(logit - ref_logit).max():.3e}")
    assert np.abs(logit - ref_logit).max() <= LOGIT_TOL

    ref.train(), net.train()
    want_loss = ref(None, x, l, d, mode="loss")["loss"]
    want_loss.backward()
    loss = net(None, x.cuda(), l.cuda(), d.cuda(), mode="loss")["loss"]
    loss.backward()
    print(f"  train loss: {loss.item():.6f} vs {want_loss.item():.6f}")
    assert abs(loss.item() - want_loss.item()) <= LOGIT_TOL
    rp, np_ = dict(ref.named_parameters()), dict(net.named_parameters())
    cancelling = ("prompt_encoder.encoder1.", "prompt_encoder.message_passing.conv.")
    bad = []
    for k in DIFFUSER_PARAMS:
        want, got = rp[k].grad.double().norm().item(), np_[k].grad.double().norm().item()
        print(f"  |grad| {k}: {got:.6e} vs {want:.6e}")
        rtol = 2e-2 if any(c in k for c in cancelling) else 2e-3
        if abs(got - want) > rtol * want + 1e-6:
            bad.append((k, got, want))
    assert not bad, bad


def test_prompt_encoder_honours_its_arguments(dgtd):
    """prompt_encoder(24, ..., grid=9, k=5, max_step=2, diffuser_latent=16) on the device equals its own torch composition (nearest
    and bilinear F.interpolate, the regressor conv, this package's MessagePassing.forward) on the same parameters, within the op
    tolerances; three tensors change shape, no state-dict key changes."""
    M = dgtd.nn.modules
    S, B = 64, 2
    default_keys = set(M.prompt_encoder(24, [64, 128, 320, 512], [3, 4, 6, 3], True).state_dict())
    torch.manual_seed(0)
    pe = M.prompt_encoder(24, [64, 128, 320, 512], [3, 4, 6, 3], True, grid=9, k=5, max_step=2, diffuser_latent=16)
    sd = pe.state_dict()
    assert set(sd) == default_keys
    assert sd["propagation_weight_regressor.reg.weight"].shape == (16 * 25, 3, 1, 1)
    assert sd["encoder1.weight"].shape == (16, 1, 1, 1)
    assert sd["message_passing.conv.weight"].shape == (3, 16, 1, 1)
    assert sd["encoder2.fusion_conv.weight"].shape[0] == 24
    pe.encoder2 = torch.nn.Identity()                      # only the front end is under test
    filler.fill_module(pe, PE)
    host = copy.deepcopy(pe)                               # CPU tensors take the modules' torch path
    x, d, _ = filler.synthetic_batch(B, S, seed=9)
    x_hp = M.fft_highpass(x, pe.freq_nums)
    mp = host.message_passing
    mp.img_size = S
    assert (mp.k, mp.max_step, host.grid) == (5, 2, 9)
    with torch.no_grad():
        weights = host.propagation_weight_regressor(F.interpolate(x_hp, size=[9, 9]))
        e1 = F.interpolate(host.encoder1(d), size=(9, 9), mode="bilinear", align_corners=False)
        want = mp(e1, weights) + x
        _, got = pe.cuda()(x.cuda(), d.cuda(), x_hp=x_hp.cuda())
    print(f"  fused: max |diff| {(got.cpu() - want).abs().max().item():.3e}")
    torch.testing.assert_close(got.cpu(), want, atol=2e-5, rtol=2e-5)


def test_captured_step_with_a_non_default_diffuser(dgtd):
    """One GraphedTrainStep at 64^2, batch 2, bf16 with diffuser = {grid: 22, k: 9, max_step: 6}: the capture succeeds (the workspaces
    come from the caller, nothing synchronises), three replays give finite losses, and the first replay matches an eager step from the
    same weights and batch at the bf16 bound of tests/test_train_gpu.py::test_graphed_step_matches_eager."""
    S, B = 64, 2
    data = dgtd.runner.SyntheticRGBD(S, B, device="cuda")
    batches = [data.batch_at(i) for i in range(3)]

    def make():
        torch.manual_seed(0)
        net = dgtd.nn.cod(drop_path_rate=0.0, compute_dtype=torch.bfloat16, diffuser={"grid": 22, "k": 9, "max_step": 6})
        filler.fill_module(net)
        net = net.cuda().train()
        red = dgtd.dist.GradReducer(net, working_dtype=torch.bfloat16)
        return net, red, dgtd.runner.FlatAdamW(red, lr=1e-4, graph_safe=True)

    net_e, red_e, opt_e = make()
    red_e.zero_grad()
    b = batches[0]
    want = net_e(b["raw"], b["input"], b["label"], b["depth"], mode="loss")["loss"]
    want.backward()
    red_e.finish()
    want = want.item()
    g = net_e.hitnet.backbone.prompt_encoder.propagation_weight_regressor.reg.weight.grad
    assert g is not None and g.shape == (24 * 81, 3, 1, 1) and torch.isfinite(g).all() and g.abs().sum() > 0

    net_g, red_g, opt_g = make()
    stepper = dgtd.runner.GraphedTrainStep(net_g, red_g, opt_g, warmup=2)
    stepper.capture(batches[0])
    got = [stepper(batches[i]).item() for i in range(3)]
    print(f"  replays {got}  eager first step {want}")
    assert all(math.isfinite(v) for v in got), got
    assert abs(got[0] - want) <= 2e-2 * max(1.0, abs(want)), (got, want)
