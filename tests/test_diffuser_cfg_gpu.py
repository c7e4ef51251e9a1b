"""GPU: the texture diffuser ops with a run-time grid, neighbourhood, step count and latent width (csrc/diffuser_cfg.hip) against the
CPU oracle with its four constants patched (oracle/cod_cpu.py:28-31), against the kernels specialised for (12, 7, 4, 24), and
their refusals.  Tolerances are those of tests/test_ops_gpu.py::test_diffuser_front_end_vs_oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ["propagation_weight_regressor.reg.weight", "propagation_weight_regressor.reg.bias", "encoder1.weight",
         "encoder1.bias", "message_passing.conv.weight", "message_passing.conv.bias"]


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


def _close_out(got, want):
    torch.testing.assert_close(got, want, atol=2e-5, rtol=2e-5)


def _close_grads(got, want):
    for n, a, b in zip(NAMES, got, want):
        a, b = a.cpu(), b.cpu()
        err, scale = (a - b).abs().max().item(), b.abs().max().item()
        print(f"  grad {n}: max |diff| {err:.3e}  (|want|_max {scale:.3e})")
        torch.testing.assert_close(a, b, atol=2e-4 * max(1.0, scale), rtol=2e-3, msg=lambda m, n=n: f"{n}: {m}")


# (G, K, steps, LAT, S, B): what each row is the smallest case for
CASES = [
    (5, 3, 1, 4, 32, 1),       # minimum everything; 25 cells < one wave
    (13, 5, 3, 20, 64, 2),     # odd grid; non-integer nearest and bilinear scales
    (22, 9, 6, 24, 96, 2),     # G^2 = 484 > 256 threads and not a multiple of 64
    (36, 7, 4, 28, 64, 2),     # G^2 = 1296 > one workgroup: threads loop over cells; LAT != 24
    (60, 11, 2, 24, 64, 1),    # largest K, near-largest G; the K/2 = 5 border band
    (12, 7, -1, 24, 64, 1),    # max_step < 0 -> as many steps as the grid is wide (12)
    (40, 7, 4, 24, 32, 1),     # G > S: both resamplings go the other way
    (64, 3, 16, 8, 64, 1),     # domain corner; G = S, scale exactly 1
    (12, 7, 0, 24, 64, 1),     # no propagation
]


@pytest.mark.parametrize("G,K,steps,LAT,S,B", CASES, ids=[",".join(map(str, c)) for c in CASES])
def test_diffuser_cfg_vs_patched_oracle(dgtd, monkeypatch, G, K, steps, LAT, S, B):
    """diffuser_state + diffuse_tail at a non-default configuration against the oracle's PromptEncoder front end with LATENT /
    DIFFUSE_GRID / DIFFUSE_K / DIFFUSE_STEPS patched: output and the six parameter gradients.  With steps == 0 x4 is the initial state
    and both regressor gradients are exact zeros."""
    from oracle import cod_cpu, filler
    real_steps = G if steps < 0 else steps
    monkeypatch.setattr(cod_cpu, "LATENT", LAT)
    monkeypatch.setattr(cod_cpu, "DIFFUSE_GRID", G)
    monkeypatch.setattr(cod_cpu, "DIFFUSE_K", K)
    monkeypatch.setattr(cod_cpu, "DIFFUSE_STEPS", real_steps)
    monkeypatch.setattr(cod_cpu, "ShapePropEncoder", lambda *a, **k: torch.nn.Identity())  # only the front end is under test
    pe = cod_cpu.PromptEncoder(S)
    filler.fill_module(pe, "hitnet.backbone.prompt_encoder.")
    g = torch.Generator().manual_seed(1000 * G + S)
    image = torch.randn(B, 3, S, S, generator=g)
    depth = torch.rand(B, 1, S, S, generator=g)
    gout = torch.randn(B, 3, S, S, generator=g)
    x_hp, fused = pe(image, depth)
    params = dict(pe.named_parameters())
    assert params[NAMES[0]].shape == (LAT * K * K, 3, 1, 1) and params[NAMES[4]].shape == (3, LAT, 1, 1)
    want = torch.autograd.grad(fused, [params[n] for n in NAMES], gout, allow_unused=True)
    want = [torch.zeros_like(params[n]) if w is None else w for n, w in zip(NAMES, want)]

    assert dgtd.ops.uses_generic(G, K, real_steps, LAT)
    dev = [params[n].detach().cuda().requires_grad_() for n in NAMES]
    x4 = dgtd.ops.diffuser_state(x_hp.cuda(), depth.cuda(), dev[0], dev[1], dev[2], dev[3], grid=G, k=K, steps=steps)
    assert x4.shape == (B, LAT, G, G)
    out = dgtd.ops.diffuse_tail(x4, dev[4], dev[5], image.cuda())
    print(f"  out: max |diff| {(out.cpu() - fused.detach()).abs().max().item():.3e}")
    _close_out(out.cpu(), fused.detach())
    got = torch.autograd.grad(out, dev, gout.cuda())
    _close_grads(got, want)
    if real_steps == 0:
        e1 = torch.nn.functional.interpolate(pe.encoder1(depth), size=(G, G), mode="bilinear", align_corners=False)
        _close_out(x4.detach().cpu(), e1.detach())
        assert torch.count_nonzero(got[0]) == 0 and torch.count_nonzero(got[1]) == 0


def _random_case(G, K, LAT, S, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x_hp = r(B, 3, S, S).abs().cuda()
    depth = torch.rand(B, 1, S, S, generator=g).cuda()
    image, gout = r(B, 3, S, S).cuda(), r(B, 3, S, S).cuda()
    params = [r(LAT * K * K, 3, 1, 1) / 3 ** 0.5, 0.05 * r(LAT * K * K), r(LAT, 1, 1, 1), 0.05 * r(LAT), r(3, LAT, 1, 1) / LAT ** 0.5, 0.05 * r(3)]
    return x_hp, depth, image, gout, [p.cuda() for p in params]


def test_generic_kernels_at_the_default_point(dgtd):
    """The run-time parameterised family at (12, 7, 4, 24) against the kernels specialised for it, same inputs: output and gradients.
    ``uses_generic`` is False exactly there."""
    u = dgtd.ops.uses_generic
    assert u(12, 7, 4, 24) is False
    assert u(13, 7, 4, 24) is True and u(12, 5, 4, 24) is True and u(12, 7, 3, 24) is True and u(12, 7, 4, 20) is True
    x_hp, depth, image, gout, params = _random_case(12, 7, 24, 64, 2, seed=7)
    res = []
    for generic in (False, True):
        dev = [p.clone().requires_grad_() for p in params]
        x4 = dgtd.ops.diffuser_state(x_hp, depth, *dev[:4], _generic=generic)
        out = dgtd.ops.diffuse_tail(x4, dev[4], dev[5], image, _generic=generic)
        res.append((x4.detach(), out.detach(), torch.autograd.grad(out, dev, gout)))
    (x4_s, out_s, g_s), (x4_g, out_g, g_g) = res
    print(f"  x4: max |diff| {(x4_g - x4_s).abs().max().item():.3e}   out: {(out_g - out_s).abs().max().item():.3e}")
    _close_out(x4_g, x4_s)
    _close_out(out_g, out_s)
    _close_grads(g_g, g_s)


def test_forward_is_bit_reproducible(dgtd):
    """No atomics in the forward: two runs of (36, 7, 4, 28), S = 64, B = 2 are identical."""
    x_hp, depth, image, _, params = _random_case(36, 7, 28, 64, 2, seed=11)
    runs = []
    for _ in range(2):
        x4 = dgtd.ops.diffuser_state(x_hp, depth, *params[:4], grid=36, k=7, steps=4)
        runs.append((x4, dgtd.ops.diffuse_tail(x4, params[4], params[5], image)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("bad", ["k=4", "k=13", "grid=65", "grid=1", "steps=65", "reg_w rows"])
def test_refusals_leave_the_library_usable(dgtd, bad):
    """Outside the domain, or with a regressor that does not match latent * k^2: DgtdError before any launch, from the Python op and (for
    the domain) from the C entry itself; a valid call afterwards still works."""
    L = dgtd._lib
    G, K, steps, LAT, S, B = 9, 5, 2, 8, 32, 1
    cfg = dict(grid=G, k=K, steps=steps)
    if bad != "reg_w rows":
        key, val = bad.split("=")
        cfg[key] = int(val)
    x_hp, depth, image, _, params = _random_case(cfg["grid"], cfg["k"], LAT, S, B, seed=3)
    if bad == "reg_w rows":
        params[0] = params[0][:-1]
    with pytest.raises(L.DgtdError):
        dgtd.ops.diffuser_state(x_hp, depth, *params[:4], **cfg)
    if bad != "reg_w rows":
        assert L.load().dgtd_diffuser_cfg_workspace(B, S, cfg["grid"], cfg["k"], cfg["steps"], LAT, 0) == -1
        with pytest.raises(L.DgtdError):   # the C entry refuses on its own: null pointers are never touched
            L.call("dgtd_diffuser_cfg_fwd", None, None, None, None, None, None, None, None, B, S, cfg["grid"], cfg["k"], cfg["steps"], LAT,
                   L.stream_ptr())
        with pytest.raises(L.DgtdError):
            L.call("dgtd_diffuser_cfg_bwd", None, None, None, None, None, None, None, None, None, None, None, None, B, S, cfg["grid"],
                   cfg["k"], cfg["steps"], LAT, L.stream_ptr())
    x_hp, depth, image, _, params = _random_case(G, K, LAT, S, B, seed=3)
    x4 = dgtd.ops.diffuser_state(x_hp, depth, *params[:4], grid=G, k=K, steps=steps)
    out = dgtd.ops.diffuse_tail(x4, params[4], params[5], image)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and x4.shape == (B, LAT, G, G)
