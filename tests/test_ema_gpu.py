"""GPU: the moving average of the weights on the device (mmengine's ``EMAHook``) - the schedule kernel against the table of
include/dgtd.h, the fused AdamW + EMA launch against its unfused self and an fp64 update, ``dgtd_ema_flat`` / ``dgtd_ema_swap``,
``FlatAdamW(ema=...)`` (slots without a gradient, fp16 with skipped steps, float buffers) and the captured step."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = ("ExponentialMovingAverage", "MomentumAnnealingEMA", "StochasticWeightAverage")
EPS_C = 2.0 ** -23      # the coefficient: the fp64 rule rounded once to fp32 (2^-24), and the fp32 image of the momentum (2^-24)
EPS_E = 2.0 ** -22      # one update e + c (p - e): three fp32 roundings of at most 2^-24 max(|e|, |p|) each, one more for an (un)contracted multiply-add
LEAD, GUARD = 4, 8      # guard elements before (a whole 16 bytes: the phase is the offset's) and after every range


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


C = _load("test_clip_grad_gpu")          # its sizes, offsets, _toy and _write_grads; its stand-in model through C.W
SIZES, OFFSETS = C.SIZES, C.OFFSETS


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def pool():
    """Random operands for the largest size (with guards), shared by the kernel tests and never written: p, g, m, v, e."""
    g = torch.Generator(device="cuda").manual_seed(13)
    n = LEAD + OFFSETS[-1] + SIZES[-1] + GUARD
    rnd = lambda s: torch.randn(n, device="cuda", generator=g) * s
    return {"p": rnd(1.0), "g": rnd(0.3), "m": rnd(0.01), "v": rnd(0.01).abs(), "e": rnd(1.0)}


def rule(kind, momentum, gamma, interval, begin_iter, iterations, enabled=True):
    """The table of include/dgtd.h in fp64: (coef, steps after, iters after) per iteration."""
    steps, out = 0, []
    for it in range(iterations):
        coef = 1.0
        if enabled and it >= begin_iter:
            if steps == 0:
                coef = 1.0
            elif steps % interval == 0:
                coef = (momentum, max(momentum, gamma / (gamma + steps)), 1.0 / (steps // interval + 1))[kind]
            else:
                coef = 0.0
            steps += 1
        out.append((coef, steps, it + 1))
    return out


def _coef_ok(got, want):
    return got == want if want in (0.0, 1.0) else abs(got - want) <= EPS_C * want


# ---------------------------------------------------------------------------------------------------------------- 1. schedule
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_schedule_kernel_follows_the_table(dgtd, kind):
    L = dgtd._lib
    for interval in (1, 3):
        for begin_iter in (0, 4):
            st = torch.tensor([-1.0, 0.0, 0.0, 1.0], device="cuda")
            want = rule(kind, 0.05, 0.25, interval, begin_iter, 12)
            for it in range(12):
                L.call("dgtd_ema_schedule", st.data_ptr(), kind, 0.05, 0.25, interval, begin_iter, L.stream_ptr())
                coef, steps, iters, enabled = st.tolist()
                print(f"kind {kind} interval {interval} begin {begin_iter} iter {it}: coef {coef!r} want {want[it][0]!r} steps {steps} iters {iters}")
                assert (steps, iters, enabled) == (want[it][1], want[it][2], 1.0)
                assert _coef_ok(coef, want[it][0]), (coef, want[it])
    st = torch.tensor([-1.0, 0.0, 0.0, 0.0], device="cuda")          # disabled: a copy, nothing counted
    for it in range(5):
        L.call("dgtd_ema_schedule", st.data_ptr(), kind, 0.05, 0.25, 1, 0, L.stream_ptr())
        assert st.tolist() == [1.0, 0.0, float(it + 1), 0.0]
    st[3] = 1.0
    L.call("dgtd_ema_schedule", st.data_ptr(), kind, 0.05, 0.25, 1, 0, L.stream_ptr())
    assert st.tolist() == [1.0, 1.0, 6.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------- 2. kernels
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _check_average(e_new, e_old, p, c, lo, hi, what):
    """e_new against the rule applied in fp64 to (e_old, p) on [lo, hi); everything outside bit-unchanged (the NaN guards stay NaN)."""
    outside = torch.ones(e_new.numel(), dtype=torch.bool, device="cuda")
    outside[lo:hi] = False
    assert torch.equal(_bits(e_new)[outside], _bits(e_old)[outside]), what + ": wrote outside its range"
    assert bool(torch.isnan(e_new[outside]).all())
    got, old, pp = e_new[lo:hi], e_old[lo:hi], p[lo:hi]
    if c == 0.0:
        assert torch.equal(_bits(got), _bits(old)), what + ": c = 0 leaves the average alone"
    elif c == 1.0:
        assert torch.equal(_bits(got), _bits(pp)), what + ": c = 1 copies"
    else:
        want = old.double() + c * (pp.double() - old.double())
        err = (got.double() - want).abs()
        bound = EPS_E * torch.maximum(old.abs(), pp.abs()).double()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{what}: c {c!r} worst error / bound {worst:.3f}")
        assert bool((err <= bound).all()), what


def _operands(pool, off, n, wdt):
    lo = LEAD + off
    tot = lo + n + GUARD
    t = {k: pool[k][:tot].clone() for k in ("p", "g", "m", "v", "e")}
    t["e"][:lo] = float("nan")
    t["e"][lo + n:] = float("nan")
    t["w"] = torch.zeros(tot, device="cuda", dtype=wdt)
    t["g16"] = t["g"].to(wdt)
    return t, lo


COEFS = (0.0, 1.0, 0.0002, 0.5)


@pytest.mark.parametrize("variant", ["f32", "g16", "clip", "amp", "skipped"])
def test_fused_kernel_against_its_unfused_self(dgtd, pool, variant):
    """dgtd_adamw_flat_ema and dgtd_adamw_flat_clip on identical inputs, every size x start offset, with a bf16 working copy: p, m, v, w
    bit-identical (the average does not disturb AdamW), e against fp64 from the returned p.  ``skipped``: amp[3] = 1, nothing but e moves."""
    L = dgtd._lib
    st = L.stream_ptr()
    clip = torch.tensor([0.37], device="cuda")
    for n in SIZES:
        for off in OFFSETS:
            for c in COEFS:
                coef = torch.tensor([c], device="cuda")
                c32 = float(coef.item())                      # what the kernel reads
                amp = None
                if variant in ("amp", "skipped"):
                    amp = torch.tensor([1024.0, 0.0, 1.0 / 1024.0, 1.0 if variant == "skipped" else 0.0, 3.0], device="cuda")
                out = []
                for ema in (False, True):
                    t, lo = _operands(pool, off, n, torch.bfloat16)
                    direct = variant == "g16"
                    args = [t["p"].data_ptr() + 4 * lo, None if direct else t["g"].data_ptr() + 4 * lo,
                            t["g16"].data_ptr() + 2 * lo if direct else None, t["m"].data_ptr() + 4 * lo, t["v"].data_ptr() + 4 * lo,
                            t["w"].data_ptr() + 2 * lo, L.BF16, n, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.001,
                            None if amp is None else amp.data_ptr(), None, clip.data_ptr() if variant == "clip" else None, 0.0]
                    if ema:
                        L.call("dgtd_adamw_flat_ema", *args, t["e"].data_ptr() + 4 * lo, coef.data_ptr(), st)
                    else:
                        L.call("dgtd_adamw_flat_clip", *args, st)
                    out.append(t)
                a, b = out
                what = f"{variant} n {n} offset {off}"
                for k in ("p", "m", "v", "w"):
                    assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs between the fused and the unfused launch"
                e0 = _operands(pool, off, n, torch.bfloat16)[0]["e"]
                assert torch.equal(_bits(a["e"]), _bits(e0))                     # the unfused launch knows no average
                if variant == "skipped":
                    for k in ("p", "m", "v"):
                        assert torch.equal(b[k], pool[k][:b[k].numel()]), f"{what}: {k} moved on a skipped step"
                    assert not bool(b["w"].count_nonzero())
                else:
                    assert not torch.equal(b["p"][lo:lo + n], pool["p"][lo:lo + n])
                    assert torch.equal(b["w"][lo:lo + n], b["p"][lo:lo + n].bfloat16()) and not bool(b["w"][:lo].count_nonzero())
                _check_average(b["e"], e0, b["p"], c32, lo, lo + n, what)


@pytest.mark.parametrize("shift", [0, 1], ids=["same_phase", "phases_differ"])
def test_ema_flat_and_swap(dgtd, pool, shift):
    """The update without AdamW and the in-place exchange, every size x start offset; ``phases_differ``: e starts one element later than p
    (both kernels only need 4-byte alignment there; a working copy needs the shared phase and is left out)."""
    L = dgtd._lib
    st = L.stream_ptr()
    for n in SIZES:
        for off in OFFSETS:
            t, lo = _operands(pool, off, n, torch.bfloat16)
            e_all = torch.full((t["e"].numel() + 1,), float("nan"), device="cuda")
            e_all[lo + shift:lo + shift + n] = pool["e"][lo:lo + n]
            p_in_e = torch.zeros_like(e_all)
            p_in_e[lo + shift:lo + shift + n] = t["p"][lo:lo + n]
            for c in COEFS:
                coef = torch.tensor([c], device="cuda")
                e = e_all.clone()
                L.call("dgtd_ema_flat", t["p"].data_ptr() + 4 * lo, e.data_ptr() + 4 * (lo + shift), n, coef.data_ptr(), st)
                assert torch.equal(t["p"], pool["p"][:t["p"].numel()])
                _check_average(e, e_all, p_in_e, float(coef.item()), lo + shift, lo + shift + n, f"ema_flat n {n} offset {off} shift {shift}")
            # swap: once (p <- e, e <- p, w = half(new p)), twice (identity)
            p, e, w = t["p"].clone(), e_all.clone(), t["w"].clone()
            wp = (w.data_ptr() + 2 * lo) if shift == 0 else None
            swap = lambda: L.call("dgtd_ema_swap", p.data_ptr() + 4 * lo, e.data_ptr() + 4 * (lo + shift), wp, L.BF16, n, st)
            swap()
            assert torch.equal(_bits(p[lo:lo + n]), _bits(e_all[lo + shift:lo + shift + n])) and torch.equal(_bits(e[lo + shift:lo + shift + n]), _bits(t["p"][lo:lo + n]))
            assert torch.equal(p[:lo], t["p"][:lo]) and torch.equal(p[lo + n:], t["p"][lo + n:])
            assert bool(torch.isnan(e[:lo + shift]).all()) and bool(torch.isnan(e[lo + shift + n:]).all())
            if shift == 0:
                assert torch.equal(w[lo:lo + n], p[lo:lo + n].bfloat16()) and not bool(w[:lo].count_nonzero()) and not bool(w[lo + n:].count_nonzero())
            swap()
            assert torch.equal(_bits(p), _bits(t["p"])) and torch.equal(_bits(e), _bits(e_all))
            if shift == 0:
                assert torch.equal(w[lo:lo + n], t["p"][lo:lo + n].bfloat16())


def test_argument_errors(dgtd, pool):
    L = dgtd._lib
    st = L.stream_ptr()
    t, lo = _operands(pool, 0, 255, torch.bfloat16)
    coef = torch.tensor([0.5], device="cuda")
    ptr = lambda k, o=0: t[k].data_ptr() + (2 if k == "w" else 4) * (lo + o)

    def fused(n=255, e=ptr("e"), c=coef.data_ptr(), p=ptr("p"), g=ptr("g"), g16=None):
        L.call("dgtd_adamw_flat_ema", p, g, g16, ptr("m"), ptr("v"), ptr("w"), L.BF16, n, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.001, None, None,
               None, 0.0, e, c, st)
    for bad in (dict(e=ptr("e", 1)), dict(n=0), dict(n=-4), dict(p=None), dict(g=None), dict(c=None), dict(g16=ptr("w"))):
        with pytest.raises(L.DgtdError):
            fused(**bad)
    for args in ((None, ptr("e"), 255, coef.data_ptr()), (ptr("p"), None, 255, coef.data_ptr()), (ptr("p"), ptr("e"), 0, coef.data_ptr()),
                 (ptr("p"), ptr("e"), 255, None), (ptr("p") + 2, ptr("e"), 255, coef.data_ptr())):
        with pytest.raises(L.DgtdError):
            L.call("dgtd_ema_flat", *args, st)
    for args in ((None, ptr("e"), None, L.BF16, 255), (ptr("p"), None, None, L.BF16, 255), (ptr("p"), ptr("e"), None, L.BF16, 0),
                 (ptr("p"), ptr("e", 1), ptr("w"), L.BF16, 255), (ptr("p"), ptr("e"), ptr("w", 1), L.BF16, 255),
                 (ptr("p"), ptr("e"), ptr("w"), L.F32, 255), (ptr("p"), ptr("p"), None, L.BF16, 255)):
        with pytest.raises(L.DgtdError):
            L.call("dgtd_ema_swap", *args, st)
    state = torch.tensor([1.0, 0.0, 0.0, 1.0], device="cuda")
    for args in ((None, 0, 0.1, 1.0, 1, 0), (state.data_ptr(), 3, 0.1, 1.0, 1, 0), (state.data_ptr(), 0, 0.0, 1.0, 1, 0),
                 (state.data_ptr(), 0, 1.0, 1.0, 1, 0), (state.data_ptr(), 1, 0.1, 0.0, 1, 0), (state.data_ptr(), 0, 0.1, 1.0, 0, 0),
                 (state.data_ptr(), 0, 0.1, 1.0, 1, -1)):
        with pytest.raises(L.DgtdError):
            L.call("dgtd_ema_schedule", *args, st)
    torch.cuda.synchronize()
    assert state.tolist() == [1.0, 0.0, 0.0, 1.0]                   # a refused call launches nothing
    assert torch.equal(t["p"], pool["p"][:t["p"].numel()])


# ---------------------------------------------------------------------------------------------------------------- 3. FlatAdamW
class Tracker:
    """The fp64 loop of tests 3-5: fed the masters (any list of tensors) and the device coefficient after every step."""

    def __init__(self, masters):
        self.e = [m.double().clone() for m in masters]
        self.updates, self.big = 0, max(float(m.abs().max()) for m in masters)

    def step(self, masters, c):
        if c != 0.0:
            self.updates += 1
            self.e = [p.double().clone() if c == 1.0 else e + c * (p.double() - e) for e, p in zip(self.e, masters)]
        self.big = max([self.big] + [float(m.abs().max()) for m in masters] + [float(e.abs().max()) for e in self.e])

    def check(self, got, what):
        """T updates, each off by at most EPS_E x the largest magnitude seen; an update contracts earlier errors by 1 - c: they at most add."""
        bound = self.updates * EPS_E * self.big
        worst = max(float((g.double() - e).abs().max()) for g, e in zip(got, self.e))
        print(f"{what}: {self.updates} updates, largest magnitude {self.big:.4f}, worst error {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound, what


def _padding_mask(b):
    pad = torch.ones_like(b["mflat"], dtype=torch.bool)
    for off, size in zip(b["offsets"], b["sizes"]):
        pad[off:off + size] = False
    return pad


MISSING = (0, 0)          # (bucket, slot) that gets no gradient: the last Linear's bias, ahead of its weight in the first bucket


def _grads_with_one_missing(red, gen, factor, poison=None):
    C._write_grads(red, None, gen, factor, poison)
    b = red.buckets[MISSING[0]]
    off, size = b["offsets"][MISSING[1]], b["sizes"][MISSING[1]]
    b["flat"][off:off + size].zero_()                          # what the reducer's gather leaves for a parameter unused this step
    b["missing"] = (MISSING[1],)


def test_flat_adamw_with_ema_on_toy(dgtd, monkeypatch):
    """bf16 toy, >= 3 buckets, two lr groups, 8 steps with interval 2, begin_iter 2, MomentumAnnealingEMA: every element of every average
    (padding and a slot without gradient included) against the fp64 loop over the recorded masters and coefficients; the masters
    bit-identical to a twin without EMA, whose launches are the ones FlatAdamW issued before EMA existed."""
    cfg = {"type": "EMAHook", "ema_type": TYPES[1], "momentum": 0.1, "gamma": 1.0, "interval": 2, "begin_iter": 2}
    called, real = [], dgtd._lib.call
    monkeypatch.setattr(dgtd._lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    runs = {}
    for key, ema in (("ema", cfg), ("off", None)):
        net, red, opt, _, _ = C._toy(dgtd, torch.bfloat16, None, ema=ema)
        gen = torch.Generator(device="cuda").manual_seed(2)
        del called[:]
        if ema is not None:
            assert len(opt.ema_bufs) == len(red.buckets) >= 3 and opt.ema_state.tolist() == [1.0, 0.0, 0.0, 1.0]
            assert all(torch.equal(e, b["mflat"]) for e, b in zip(opt.ema_bufs, red.buckets))
            track = Tracker([b["mflat"] for b in red.buckets])
            want = rule(1, 0.1, 1.0, 2, 2, 8)
        for step in range(8):
            _grads_with_one_missing(red, gen, C.FACTORS[step % len(C.FACTORS)])
            opt.step()
            if ema is not None:
                coef, steps, iters, _ = opt.ema_state.tolist()
                assert (steps, iters) == (want[step][1], want[step][2]) and _coef_ok(coef, want[step][0]), (step, coef, want[step])
                track.step([b["mflat"] for b in red.buckets], coef)
        runs[key] = (red, opt, list(called))
    red, opt, names = runs["ema"]
    assert opt.ema_steps == 6 and opt.ema_iters == 8 and opt.steps == 8
    track.check(opt.ema_bufs, "toy")
    assert track.updates == 5 and any(0.1 < c[0] < 1.0 for c in want)
    for b, e in zip(red.buckets, opt.ema_bufs):
        assert not bool(e[_padding_mask(b)].count_nonzero()), "the padding of the average stays zero"
    b = red.buckets[MISSING[0]]
    sl = slice(b["offsets"][MISSING[1]], b["offsets"][MISSING[1]] + b["sizes"][MISSING[1]])
    assert torch.equal(opt.ema_bufs[MISSING[0]][sl], b["mflat"][sl]) and bool(b["mflat"][sl].count_nonzero())   # never updated: its average is itself
    n_runs = sum(len(opt._merge(s, bb["n_work"], set(bb["missing"]))) for s, bb in zip(opt.slots, red.buckets))
    assert names.count("dgtd_ema_schedule") == 8 and names.count("dgtd_adamw_flat_ema") == 8 * n_runs and names.count("dgtd_ema_flat") == 8
    assert set(names) == {"dgtd_ema_schedule", "dgtd_adamw_flat_ema", "dgtd_ema_flat"}
    red0, opt0, names0 = runs["off"]
    assert names0 == ["dgtd_adamw_flat_amp"] * (8 * n_runs), names0[:12]
    for a, b0, sa, sb in zip(red.buckets, red0.buckets, opt.state, opt0.state):
        assert torch.equal(a["mflat"], b0["mflat"])
        assert (a["wflat"] is None) == (b0["wflat"] is None) and (a["wflat"] is None or torch.equal(a["wflat"], b0["wflat"]))
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert opt0.ema_steps == 0 and opt0.ema_bufs == [] and opt0.ema_state is None


# ---------------------------------------------------------------------------------------------------------------- 4. fp16 + loss scaler
def test_skipped_fp16_steps_still_update_the_average(dgtd):
    """An inf at step 1 (and one at step 3, where the average has left the weights): the optimizer skips them, the average does not."""
    scaler = dgtd.runner.LossScaler("cuda", init_scale=1024.0, growth_interval=100)
    net, red, opt, _, _ = C._toy(dgtd, torch.float16, None, scaler=scaler, ema={"momentum": 0.25})
    gen = torch.Generator(device="cuda").manual_seed(2)
    track = Tracker([b["mflat"] for b in red.buckets])
    for step in range(5):
        before = [b["mflat"].clone() for b in red.buckets]
        e_before = [e.clone() for e in opt.ema_bufs]
        poison = float("inf") if step in (1, 3) else None
        C._write_grads(red, None, gen, C.FACTORS[step] * scaler.get_scale(), poison)
        opt.step()
        coef = opt.ema_state[0].item()
        assert coef == (1.0 if step == 0 else float(np.float32(0.25)))
        track.step([b["mflat"] for b in red.buckets], coef)
        if poison is not None:
            for b, p0, e0, e in zip(red.buckets, before, e_before, opt.ema_bufs):
                assert torch.equal(b["mflat"], p0)                                        # the masters did not move ...
                want = e0.double() + coef * (p0.double() - e0.double())                    # ... and the average moved towards them
                assert bool(((e.double() - want).abs() <= EPS_E * torch.maximum(e0.abs(), p0.abs()).double()).all())
            if step == 3:
                assert any(not torch.equal(e, e0) for e, e0 in zip(opt.ema_bufs, e_before))
        assert opt.ema_steps == step + 1
    assert opt.steps == 3 and opt.ema_steps == 5 and scaler.get_scale() == 256.0
    track.check(opt.ema_bufs, "fp16")


# ---------------------------------------------------------------------------------------------------------------- 5. captured step
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_graphed_step_replays_the_schedule(dgtd, dtype):
    W = C.W
    data = W.batches(4)
    net = W.stand_in(dgtd, dtype)
    red = dgtd.dist.GradReducer(net, bucket_bytes=32 << 10, working_dtype=dtype, exclude_prefixes=())
    opt = dgtd.runner.FlatAdamW(red, lr=1e-3, custom_keys={}, graph_safe=True,
                                ema={"ema_type": TYPES[1], "momentum": 0.1, "gamma": 1.0, "begin_iter": 1})
    masters = lambda: [b["mflat"] for b in red.buckets]
    start = [m.clone() for m in masters()]
    stepper = dgtd.runner.GraphedTrainStep(net, red, opt, warmup=2)
    stepper.capture(data[0])
    assert opt.ema_steps == 0 and opt.ema_iters == 0 and opt.steps == 0                    # the warm-up left no trace
    assert all(torch.equal(e, s) and torch.equal(m, s) for e, m, s in zip(opt.ema_bufs, masters(), start))
    track = Tracker(masters())
    want = rule(1, 0.1, 1.0, 1, 1, 4)
    for i, b in enumerate(data):
        loss = stepper(b).item()
        coef, steps, iters, _ = opt.ema_state.tolist()
        print(f"[{dtype}] replay {i}: loss {loss:.5f} coef {coef!r} steps {steps} iters {iters}")
        assert math.isfinite(loss) and (steps, iters) == (want[i][1], want[i][2]) and _coef_ok(coef, want[i][0]), (i, coef, want[i])
        track.step(masters(), coef)
    assert [w[0] for w in want] == [1.0, 1.0, 0.5, 1.0 / 3.0] and opt.ema_steps == 3
    track.check(opt.ema_bufs, f"graph {dtype}")
    assert any(not torch.equal(e, m) for e, m in zip(opt.ema_bufs, masters()))
    # validation between replays: swap, an eval-mode forward, swap back - every bit as before, and the graph still runs
    state = lambda: ([m.clone() for m in masters()] + [e.clone() for e in opt.ema_bufs]
                     + [b["wflat"].clone() for b in red.buckets if b["wflat"] is not None] + [bf.clone() for bf in net.buffers()])
    before = state()
    opt.swap_ema()
    assert all(torch.equal(m, e0) for m, e0 in zip(masters(), before[len(red.buckets):2 * len(red.buckets)]))
    for b_ in red.buckets:
        if b_["wflat"] is not None:
            assert torch.equal(b_["wflat"], b_["mflat"][:b_["n_work"]].to(dtype))
    net.eval()
    with torch.no_grad():
        val = net(None, data[1]["input"], data[1]["label"], data[1]["depth"], mode="loss")["loss"].item()
    net.train()
    opt.swap_ema()
    assert math.isfinite(val) and all(torch.equal(_bits(a), _bits(b_)) for a, b_ in zip(state(), before))
    assert math.isfinite(stepper(data[0]).item()) and opt.ema_steps == 4
    stepper.release()


# ---------------------------------------------------------------------------------------------------------------- 6. float buffers
def test_update_buffers_averages_the_float_buffers(dgtd):
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.bn = torch.nn.BatchNorm2d(16)
            self.scale = torch.nn.Parameter(torch.ones(16))

        def forward(self, x):
            assert dgtd.ops.batch_norm_supported(x, self.bn)
            return dgtd.ops.batch_norm(x, self.bn) * self.scale.view(1, -1, 1, 1)

    torch.manual_seed(1)
    net = Net().cuda().train()
    red = dgtd.dist.GradReducer(net, exclude_prefixes=())
    with pytest.raises(ValueError):                                   # whose buffers?
        dgtd.runner.FlatAdamW(red, lr=1e-2, custom_keys={}, ema={"momentum": 0.25, "update_buffers": True})
    opt = dgtd.runner.FlatAdamW(red, lr=1e-2, custom_keys={}, ema={"momentum": 0.25, "update_buffers": True}, module=net)
    names = ("bn.running_mean", "bn.running_var")
    assert set(opt.ema_tensors()) == {"bn.weight", "bn.bias", "scale"} | set(names)
    live = lambda: [dict(net.named_buffers())[n] for n in names]
    track = Tracker(live())
    g = torch.Generator(device="cuda").manual_seed(3)
    for step in range(4):
        x = (torch.randn(2, 16, 8, 8, device="cuda", generator=g) * (1.0 + step) + step).contiguous(memory_format=torch.channels_last)
        red.zero_grad()
        (net(x) ** 2).mean().backward()
        red.finish()
        opt.step()
        track.step(live(), opt.ema_state[0].item())
    assert int(net.bn.num_batches_tracked) == 4 and net.bn.num_batches_tracked.dtype == torch.int64      # integer buffers are left alone
    avg = [opt.ema_tensors()[n] for n in names]
    track.check(avg, "buffers")
    assert all(not torch.equal(a, l) for a, l in zip(avg, live()))
    raw, kept = [l.clone() for l in live()], [a.clone() for a in avg]
    opt.swap_ema()
    assert all(torch.equal(l, k) for l, k in zip(live(), kept)) and all(torch.equal(opt.ema_tensors()[n], r) for n, r in zip(names, raw))
    assert int(net.bn.num_batches_tracked) == 4
    opt.swap_ema()
    assert all(torch.equal(l, r) for l, r in zip(live(), raw)) and all(torch.equal(opt.ema_tensors()[n], k) for n, k in zip(names, kept))
