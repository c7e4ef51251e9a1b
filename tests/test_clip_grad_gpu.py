"""GPU: gradient clipping on the device (mmengine's ``optim_wrapper.clip_grad``, config/cod.yml:108-110) - the norm kernels against
NumPy fp64, the found_inf they fold in, FlatAdamW with clip_grad against torch's utilities + torch.optim.AdamW (fp32 buckets, fp16 with
the loss scaler, the 16-bit payload), and the clipped step captured in a hipGraph (world 1 and fused communication)."""
import copy
import importlib.util
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS32 = 2.0 ** -23          # the fp64 sum's own error is ~1e-16 relative; the ONE rounding to fp32 costs <= 2^-24: bound 2^-23
SIZES = (1, 3, 5, 255, 1027, 1_000_003)
OFFSETS = (0, 1, 2, 3)      # elements: the unaligned head and tail (fp32: 0-3 scalars, 16-bit: up to 7)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
L2, INF = 0, 1


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


W = _load("_clip_grad_worker")


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def pool():
    """One random vector per dtype (device) with its exact fp64 image (host), shared by the kernel tests and never written."""
    g = torch.Generator(device="cuda").manual_seed(7)
    out = {}
    for k, dt in DTYPES.items():
        t = (torch.randn(SIZES[-1] + OFFSETS[-1], device="cuda", generator=g) * 3.0).to(dt)
        out[k] = (t, t.double().cpu().numpy())
    return out


def _grid(n):
    return max(1, min(1024, -(-n // 4096)))


def _partial(dgtd, t, kind, ws, k, grid):
    L = dgtd._lib
    L.call("dgtd_grad_norm_partial", t.data_ptr(), L.dtype_code(t), t.numel(), kind, ws.data_ptr() + 8 * k, grid, L.stream_ptr())
    return k + grid


def _finalize(dgtd, ws, k, kind, max_norm, amp=None):
    L = dgtd._lib
    cs = torch.full((2,), -1.0, device="cuda")
    L.call("dgtd_grad_clip_finalize", ws.data_ptr(), k, kind, max_norm, None if amp is None else amp.data_ptr(), cs.data_ptr(), L.stream_ptr())
    return cs.cpu().numpy()


def _ref(x64, kind):
    return float(np.sqrt(np.sum(x64 * x64))) if kind == L2 else float(np.max(np.abs(x64)))


def _check(got, want, kind, what):
    print(f"{what}: got {got!r} want {want!r} rel {abs(float(got) - want) / want:.3e}")
    if kind == INF:
        assert got == np.float32(want), what                 # a maximum of representable values: exact
    else:
        assert abs(float(got) - want) <= EPS32 * want, what


def _coef(total, max_norm):
    return min(np.float32(1.0), np.float32(max_norm) / (np.float32(total) + np.float32(1e-6)))


@pytest.mark.parametrize("kind", [L2, INF], ids=["l2", "inf"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_norm_kernels_match_numpy_fp64(dgtd, pool, dt, kind):
    """Every size x start offset on its own, then the partials of all six sizes ('buckets') through ONE finalize; two grids for the
    large size (the unrolled loop runs several times per lane with the small one); a grid larger than the work; a second run
    bit-identical down to the partials."""
    t, x64 = pool[dt]
    ws = torch.full((4096,), float("nan"), dtype=torch.float64, device="cuda")
    max_norm = 100.0
    for off in OFFSETS:
        k_all, parts = 0, []
        ws_all = torch.full((2048,), float("nan"), dtype=torch.float64, device="cuda")
        for n in SIZES:
            for grid in {_grid(n), 16 if n > 4096 else 3}:
                k = _partial(dgtd, t[off:off + n], kind, ws, 0, grid)
                cs = _finalize(dgtd, ws, k, kind, max_norm)
                want = _ref(x64[off:off + n], kind)
                _check(cs[0], want, kind, f"{dt} kind {kind} n {n} offset {off} grid {grid}")
                assert abs(cs[1] - _coef(cs[0], max_norm)) <= EPS32 * cs[1], (cs, _coef(cs[0], max_norm))
                assert cs[1] < 1.0 or cs[0] <= max_norm
            k_all = _partial(dgtd, t[off:off + n], kind, ws_all, k_all, _grid(n))
            parts.append(x64[off:off + n])
        first = ws_all[:k_all].clone()
        cs = _finalize(dgtd, ws_all, k_all, kind, max_norm)
        _check(cs[0], _ref(np.concatenate(parts), kind), kind, f"{dt} kind {kind} all sizes offset {off}")
        ws_all.fill_(float("nan"))
        k2 = 0
        for n in SIZES:
            k2 = _partial(dgtd, t[off:off + n], kind, ws_all, k2, _grid(n))
        cs2 = _finalize(dgtd, ws_all, k2, kind, max_norm)
        assert k2 == k_all and torch.equal(first.view(torch.int64), ws_all[:k_all].view(torch.int64))
        assert cs.tobytes() == cs2.tobytes()


def test_l2_norm_of_large_fp32_elements_does_not_overflow(dgtd):
    """|g| = 3e19: every square (9e38) is beyond fp32, the norm (9.6e20) is not."""
    n = 1027
    g = torch.Generator(device="cuda").manual_seed(11)
    t = torch.where(torch.rand(n, device="cuda", generator=g) < 0.5, -1.0, 1.0) * 3e19
    assert torch.isinf((t * t).sum())
    ws = torch.zeros(8, dtype=torch.float64, device="cuda")
    cs = _finalize(dgtd, ws, _partial(dgtd, t, L2, ws, 0, 1), L2, 1.0)
    want = _ref(t.double().cpu().numpy(), L2)
    assert math.isfinite(cs[0])
    _check(cs[0], want, L2, "3e19")
    assert 0.0 < cs[1] < 1e-20


@pytest.mark.parametrize("kind", [L2, INF], ids=["l2", "inf"])
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_finalize_folds_found_inf(dgtd, pool, dt, kind):
    """With amp_state the finalize IS the step's inf / NaN check: one inf, then one NaN, in the unaligned head, the 16-byte body and
    the tail each raise amp_state[3]; finite data leaves it alone and reports 1/scale times the raw norm."""
    src, x64 = pool[dt]
    n, off, scale = 1030, 1, 1024.0                           # fp32: head 3, body 256 x 4, tail 3; fp16: head 7, body 127 x 8, tail 7
    ws = torch.zeros(8, dtype=torch.float64, device="cuda")
    amp = lambda: torch.tensor([scale, 0.0, 1.0 / scale, 0.0, 0.0], device="cuda")
    a = amp()
    cs = _finalize(dgtd, ws, _partial(dgtd, src[off:off + n], kind, ws, 0, 2), kind, 1.0, a)
    assert a.tolist() == [scale, 0.0, 1.0 / scale, 0.0, 0.0]
    _check(cs[0], _ref(x64[off:off + n], kind) / scale, kind, f"{dt} finite, unscaled")
    for pos in (1, 500, n - 1):
        for bad in (float("inf"), float("-inf"), float("nan")):
            t = src[:off + n].clone()
            t[off + pos] = bad
            a = amp()
            cs = _finalize(dgtd, ws, _partial(dgtd, t[off:], kind, ws, 0, 2), kind, 1.0, a)
            assert a[3].item() == 1.0 and a[0].item() == scale, (pos, bad, a.tolist())
            assert not math.isfinite(cs[0]) and math.isnan(cs[0]) == math.isnan(bad), (pos, bad, cs)


# ---------------------------------------------------------------------------------------------------------------- FlatAdamW vs torch
def _toy(dgtd, working_dtype, clip, scaler=None, **kw):
    """The construction of test_loss_scaler_matches_torch_grad_scaler: a toy Sequential, here in several buckets with two lr multipliers."""
    torch.manual_seed(0)
    net = torch.nn.Sequential(dgtd.nn.modules.Linear(32, 48), torch.nn.LayerNorm(48), dgtd.nn.modules.Linear(48, 7)).cuda()
    twin = copy.deepcopy(net)
    red = dgtd.dist.GradReducer(net, working_dtype=working_dtype, exclude_prefixes=(), bucket_bytes=64)
    assert len(red.buckets) >= 3
    keys = {"0.": 0.25}
    opt = dgtd.runner.FlatAdamW(red, lr=1e-2, weight_decay=0.1, custom_keys=keys, scaler=scaler, clip_grad=clip, **kw)
    assert len(opt.param_groups) == 2
    tparams = dict(twin.named_parameters())
    names = [n for b in red.buckets for n in b["names"]]
    topt = torch.optim.AdamW([{"params": [tparams[n] for n in names if not n.startswith("0.")], "lr": 1e-2},
                              {"params": [tparams[n] for n in names if n.startswith("0.")], "lr": 0.25e-2}], lr=1e-2, weight_decay=0.1)
    return net, red, opt, tparams, topt


def _write_grads(red, tparams, gen, factor, poison=None):
    """Random gradients x ``factor`` into every parameter's slot of the flat buckets (the alignment padding stays zero, as the
    reducer leaves it) and, as clones, into the torch twin; returns their exact fp64 L2 norm."""
    sq = 0.0
    for bi, b in enumerate(red.buckets):
        for i, (n, off, size, shape) in enumerate(zip(b["names"], b["offsets"], b["sizes"], b["shapes"])):
            g = torch.randn(size, device="cuda", generator=gen) * 0.1 * factor
            if poison is not None and bi == 1 and i == 0:
                g[size // 2] = poison
            b["flat"][off:off + size].copy_(g)
            if tparams is not None:
                tparams[n].grad = g.view(shape).clone()
            sq += float((g.double() ** 2).sum())
    return math.sqrt(sq)


# gradients of norm ~0.1 * sqrt(2000) * factor = 4.5 * factor against max_norm 3: clipped at factor 1 and 3, untouched at 0.2 and 0.05
FACTORS = (1.0, 0.2, 3.0, 0.05, 1.0, 0.2)


@pytest.mark.parametrize("clip", [{"max_norm": 3.0, "norm_type": 2}, {"type": "value", "clip_value": 0.1}], ids=["norm", "value"])
def test_flat_adamw_clip_matches_torch(dgtd, clip):
    net, red, opt, tparams, topt = _toy(dgtd, torch.bfloat16, clip)
    gen = torch.Generator(device="cuda").manual_seed(2)
    coefs = []
    for step in range(6):
        want = _write_grads(red, tparams, gen, FACTORS[step])
        params = [p for g in topt.param_groups for p in g["params"]]
        if clip.get("type") == "value":
            torch.nn.utils.clip_grad_value_(params, clip["clip_value"])
            assert opt.grad_norm() is None
        else:
            torch.nn.utils.clip_grad_norm_(params, clip["max_norm"])
        opt.step()
        topt.step()
        if clip.get("type") != "value":
            got = opt.grad_norm()
            print(f"step {step}: grad_norm {got!r} fp64 {want!r} rel {abs(got - want) / want:.3e} coef {opt._clip_state[1].item()!r}")
            assert abs(got - want) <= EPS32 * want
            coefs.append(opt._clip_state[1].item())
            assert abs(coefs[-1] - float(_coef(got, clip["max_norm"]))) <= EPS32 * coefs[-1]
    if coefs:
        assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs      # active on some steps, inactive on others
    for n, p in net.named_parameters():
        torch.testing.assert_close(p, tparams[n], rtol=2e-5, atol=2e-6, msg=lambda m, n=n: f"{n}: {m}")
    lin = net[0]
    torch.testing.assert_close(lin._w.float(), lin.weight.detach().bfloat16().float(), rtol=0, atol=0)


@pytest.mark.parametrize("graph_safe", [False, True])
def test_coefficient_one_is_bit_identical_to_no_clipping(dgtd, graph_safe):
    runs = []
    for clip in (None, {"max_norm": 1e30}):
        net, red, opt, _, _ = _toy(dgtd, torch.bfloat16, clip, graph_safe=graph_safe)
        gen = torch.Generator(device="cuda").manual_seed(2)
        for step in range(3):
            _write_grads(red, None, gen, FACTORS[step])
            opt.step()
        if clip is not None:
            assert opt._clip_state[1].item() == 1.0
        runs.append((red, opt))
    (ra, oa), (rb, ob) = runs
    for a, b, sa, sb in zip(ra.buckets, rb.buckets, oa.state, ob.state):
        assert torch.equal(a["mflat"], b["mflat"]) and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
        assert (a["wflat"] is None) == (b["wflat"] is None) and (a["wflat"] is None or torch.equal(a["wflat"], b["wflat"]))


def test_fp16_loss_scaler_with_norm_clip_matches_grad_scaler(dgtd, monkeypatch):
    """GradScaler.unscale_ -> clip_grad_norm_ -> step -> update on identical scaled gradients: 9 steps, an inf at step 1 and a NaN at
    step 5 (skipped, scale halved), the norm pass standing in for the found_inf pass."""
    scaler = dgtd.runner.LossScaler("cuda", init_scale=1024.0, growth_interval=3)
    clip = {"max_norm": 3.0}
    net, red, opt, tparams, topt = _toy(dgtd, torch.float16, clip, scaler=scaler)
    ts = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=3)
    ts.scale(torch.zeros(1, device="cuda"))
    called, real = [], dgtd._lib.call
    monkeypatch.setattr(dgtd._lib, "call", lambda name, *a, **k: (called.append(name), real(name, *a, **k))[1])
    gen = torch.Generator(device="cuda").manual_seed(2)
    factors, coefs = FACTORS + (3.0, 0.2, 1.0), []
    for step in range(9):
        scale_now = scaler.get_scale()
        assert scale_now == ts.get_scale(), (step, scale_now, ts.get_scale())
        poison = {1: float("inf"), 5: float("nan")}.get(step)
        want = _write_grads(red, tparams, gen, factors[step] * scale_now, poison) / scale_now
        opt.step()
        ts.unscale_(topt)
        torch.nn.utils.clip_grad_norm_([p for g in topt.param_groups for p in g["params"]], clip["max_norm"])
        ts.step(topt)
        ts.update()
        if poison is None:
            got = opt.grad_norm()
            print(f"step {step}: unscaled grad_norm {got!r} fp64 {want!r} coef {opt._clip_state[1].item()!r}")
            assert abs(got - want) <= EPS32 * want
            coefs.append(opt._clip_state[1].item())
        else:
            assert not math.isfinite(opt.grad_norm())
    assert scaler.get_scale() == ts.get_scale()
    assert opt.steps == 7
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    assert "dgtd_found_inf" not in called and called.count("dgtd_grad_clip_finalize") == 9 and "dgtd_grad_norm_partial" in called
    for n, p in net.named_parameters():
        torch.testing.assert_close(p, tparams[n], rtol=2e-5, atol=2e-6, msg=lambda m, n=n: f"{n}: {m}")
    lin = net[0]
    torch.testing.assert_close(lin._w.float(), lin.weight.detach().half().float(), rtol=0, atol=0)


@pytest.mark.parametrize("mode", ["norm", "value"])
def test_clipped_adamw_reads_the_16bit_payload_like_its_fp32_image(dgtd, mode):
    """The clipped entry with a bf16 run (the all-reduce payload) and with the same values widened to fp32: bit-identical masters,
    moments and working copies; unaligned start, a working copy and a coefficient < 1."""
    L = dgtd._lib
    n, off = 1027, 1
    g = torch.Generator(device="cuda").manual_seed(4)
    g16 = (torch.randn(n + off, device="cuda", generator=g) * 0.3).bfloat16()
    coef = torch.tensor([0.37], device="cuda")
    out = []
    for direct in (True, False):
        gg = torch.Generator(device="cuda").manual_seed(9)
        p = torch.randn(n + off, device="cuda", generator=gg)
        m, v = torch.randn(n + off, device="cuda", generator=gg) * 0.01, torch.rand(n + off, device="cuda", generator=gg) * 0.01
        w = torch.zeros(n + off, device="cuda", dtype=torch.bfloat16)
        g32 = g16.float()
        L.call("dgtd_adamw_flat_clip", p.data_ptr() + 4 * off, None if direct else g32.data_ptr() + 4 * off,
               g16.data_ptr() + 2 * off if direct else None, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off, w.data_ptr() + 2 * off, L.BF16, n,
               1e-2, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.001, None, None, coef.data_ptr() if mode == "norm" else None,
               0.0 if mode == "norm" else 0.2, L.stream_ptr())
        torch.cuda.synchronize()
        out.append((p, m, v, w))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    p, m, v, w = out[0]
    assert w[0].item() == 0.0 and torch.equal(w[off:], p[off:].bfloat16())
    # the update saw the clipped gradient: m = m0 + 0.1 (g' - m0)
    gg = torch.Generator(device="cuda").manual_seed(9)
    torch.randn(n + off, device="cuda", generator=gg)
    m0 = torch.randn(n + off, device="cuda", generator=gg) * 0.01
    gc = g16.float() * 0.37 if mode == "norm" else g16.float().clamp(-0.2, 0.2)
    torch.testing.assert_close(m[off:], (m0 + (1.0 - 0.9) * (gc - m0))[off:], rtol=1e-6, atol=1e-8)
    with pytest.raises(L.DgtdError):          # both forms at once: an argument error
        L.call("dgtd_adamw_flat_clip", p.data_ptr(), g16.float().data_ptr(), None, m.data_ptr(), v.data_ptr(), None, L.BF16, 8,
               1e-2, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.001, None, None, coef.data_ptr(), 0.2, L.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------- captured step
def _padding_is_zero(red):
    for b in red.buckets:
        pad = torch.ones_like(b["flat"], dtype=torch.bool)
        for off, size in zip(b["offsets"], b["sizes"]):
            pad[off:off + size] = False
        if bool(b["flat"][pad].count_nonzero()) or (b["g16"] is not None and bool(b["g16"][pad[:b["n_work"]]].count_nonzero())):
            return False
    return True


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_graphed_step_with_norm_clip_matches_eager(dgtd, dtype):
    """The clipped step captured as ONE hipGraph: 4 replays follow 4 eager steps (tolerances of test_graphed_step_matches_eager), the
    norm read back after every replay is that step's (it moves from step to step: nothing of it is frozen into the graph), with
    max_norm at half the first step's norm so the coefficient is at work."""
    data = W.batches(4)

    def make(clip):
        net = W.stand_in(dgtd, dtype)
        red = dgtd.dist.GradReducer(net, bucket_bytes=32 << 10, working_dtype=dtype, exclude_prefixes=())
        assert len(red.buckets) >= 2
        return net, red, dgtd.runner.FlatAdamW(red, lr=1e-3, custom_keys={}, graph_safe=True, clip_grad=clip)

    probe = make({"max_norm": 1e30})
    first = W.eager_step(*probe, data[0])[1]
    assert _padding_is_zero(probe[1]), "the reducer leaves the alignment padding of the buckets zero"
    clip = {"max_norm": 0.5 * first}
    net_e, red_e, opt_e = make(clip)
    want = []
    for i, b in enumerate(data):
        want.append(W.eager_step(net_e, red_e, opt_e, b))
        if i == 0:                                            # max_norm / norm = 1/2: the coefficient is at work
            assert abs(want[0][1] - first) <= 1e-4 * first and abs(opt_e._clip_state[1].item() - 0.5) < 1e-3
    net_g, red_g, opt_g = make(clip)
    stepper = dgtd.runner.GraphedTrainStep(net_g, red_g, opt_g, warmup=2)
    stepper.capture(data[0])
    got = []
    for b in data:
        loss = stepper(b).item()
        got.append((loss, opt_g.grad_norm()))
    print(f"[{dtype}] eager {want}\n[{dtype}] graph {got}")
    assert opt_g.steps == opt_e.steps == 4
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    for (la, na), (lb, nb) in zip(got, want):
        assert math.isfinite(la) and abs(la - lb) <= tol * max(1.0, abs(lb)), (got, want)
        assert abs(np.float32(na) - np.float32(nb)) <= 1e-4 * nb, (got, want)
    norms = [n for _, n in got]
    assert len(set(norms)) == 4 and max(norms) > 1.05 * min(norms), norms
    if dtype == torch.float32:
        for (k, p), (_, q) in zip(net_g.named_parameters(), net_e.named_parameters()):
            torch.testing.assert_close(p, q, rtol=1e-2, atol=5e-4, msg=lambda m, k=k: f"{k}: {m}")
    stepper.release()


def test_fused_communication_with_norm_clip():
    """comm="fused" (collectives captured inside the graph, AdamW joining bucket after bucket, the working-copy segment read from the
    16-bit payload) with clip_grad by norm, in a process of its own with a world-1 RCCL group: 3 steps taken, losses finite and
    within 2e-2 of the eager run's, a finite positive gradient norm after every step."""
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "_clip_grad_worker.py"), str(port)],
                       env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(out)
    assert out["steps"] == 3
    for a_, b_ in zip(out["fused"]["losses"], out["eager"]["losses"]):
        assert math.isfinite(a_) and abs(a_ - b_) <= 2e-2 * max(1.0, abs(b_)), out
    assert all(math.isfinite(n) and n > 0.0 for n in out["fused"]["norms"]), out
    assert out["fused"]["norms"][0] > out["max_norm"], out       # the coefficient was at work
