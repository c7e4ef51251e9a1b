"""CPU: mmengine's ``EMAHook`` (``custom_hooks``) - the keys the runner accepts, the schedule (coefficient and ``steps`` per iteration)
against a restatement of the table in include/dgtd.h, and the runner's torch path (``EmaTorch`` beside torch.optim.AdamW): the average
against an fp64 loop, validation with the averaged weights, the checkpoint layout and its round trip."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("ExponentialMovingAverage", "MomentumAnnealingEMA", "StochasticWeightAverage")
EPS = 2.0 ** -22        # one update e + c (p - e): three fp32 roundings of at most 2^-24 max(|e|, |p|) each, one more for an (un)contracted multiply-add


@pytest.fixture(scope="module")
def dgtd():
    import __graft_entry__ as ge
    ge.build()
    import dgtd as m
    return m


def test_defaults_and_accepted_spellings(dgtd):
    parse = dgtd.runner.parse_ema
    assert parse(None) is None
    want = {"ema_type": TYPES[0], "kind": 0, "momentum": 0.0002, "gamma": 100.0, "interval": 1, "update_buffers": False,
            "begin_iter": 0, "begin_epoch": 0, "strict_load": False}
    assert parse({}) == want and parse({"type": "EMAHook"}) == want and parse({"type": "EMAHook", "priority": "NORMAL"}) == want
    got = parse({"type": "EMAHook", "ema_type": TYPES[1], "momentum": 0.001, "gamma": 50, "interval": 3, "update_buffers": True,
                 "begin_iter": 7, "strict_load": True})
    assert got == {"ema_type": TYPES[1], "kind": 1, "momentum": 0.001, "gamma": 50.0, "interval": 3, "update_buffers": True,
                   "begin_iter": 7, "begin_epoch": 0, "strict_load": True}
    assert parse({"ema_type": TYPES[2], "begin_epoch": 2})["kind"] == 2
    assert parse({"begin_iter": 0, "begin_epoch": 3})["begin_epoch"] == 3


@pytest.mark.parametrize("bad", [
    "EMAHook", {"type": "our_init"}, {"ema_type": "EMA"}, {"ema_type": None},
    {"momentum": 0}, {"momentum": 0.0}, {"momentum": 1}, {"momentum": 1.5}, {"momentum": -0.1}, {"momentum": "0.1"}, {"momentum": True},
    {"momentum": float("nan")},
    {"ema_type": TYPES[1], "gamma": 0}, {"ema_type": TYPES[1], "gamma": -1.0}, {"ema_type": TYPES[1], "gamma": float("inf")},
    {"gamma": 100}, {"ema_type": TYPES[2], "gamma": 100},
    {"interval": 0}, {"interval": -2}, {"interval": 1.5}, {"interval": True},
    {"update_buffers": 1}, {"strict_load": "yes"},
    {"begin_iter": -1}, {"begin_iter": 0.5}, {"begin_epoch": -1}, {"begin_iter": 2, "begin_epoch": 1},
    {"decay": 0.999}, {"momentum": 0.1, "warmup": 5},
], ids=repr)
def test_bad_spellings_raise(dgtd, bad):
    with pytest.raises(ValueError):
        dgtd.runner.parse_ema(bad)
    if isinstance(bad, dict):
        class NoBuckets:
            buckets, working_dtype, world = [], None, 1
        with pytest.raises(ValueError):                     # before anything is built
            dgtd.runner.FlatAdamW(NoBuckets(), ema=bad)


def rule(kind, momentum, gamma, interval, begin_iter, iterations, enabled=True):
    """The table of include/dgtd.h restated: (coef, steps after, iters after) per iteration."""
    steps, out = 0, []
    for it in range(iterations):
        if not enabled or it < begin_iter:
            coef = 1.0
        else:
            if steps == 0:
                coef = 1.0
            elif steps % interval == 0:
                coef = (momentum, max(momentum, gamma / (gamma + steps)), 1.0 / (steps // interval + 1))[kind]
            else:
                coef = 0.0
            steps += 1
        out.append((coef, steps, it + 1))
    return out


@pytest.mark.parametrize("begin_iter", [0, 4])
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_schedule_follows_the_table(dgtd, kind, interval, begin_iter):
    cfg = {"ema_type": TYPES[kind], "momentum": 0.05, "interval": interval, "begin_iter": begin_iter}
    if kind == 1:
        cfg["gamma"] = 0.25
    ema = dgtd.runner.EmaTorch(None, cfg)
    want = rule(kind, 0.05, 0.25, interval, begin_iter, 12)
    got = []
    for _ in range(12):
        c = ema.schedule()
        got.append((c, ema.ema_steps, ema.ema_iters))
    print(kind, interval, begin_iter, got)
    assert got == want
    assert [s for _, s, _ in got][-1] == 12 - begin_iter
    updates = [c for c, _, _ in got[begin_iter:]]
    assert updates[0] == 1.0 and all((c == 0.0) == (i % interval != 0) for i, c in enumerate(updates))
    if kind == 1:           # annealing: gamma / (gamma + steps) until the momentum takes over
        assert any(c == 0.05 for c in updates) and any(0.05 < c < 1.0 for c in updates)
    off = dgtd.runner.EmaTorch(None, cfg)
    off.set_ema_enabled(False)
    assert [off.schedule() for _ in range(6)] == [1.0] * 6 and off.ema_steps == 0 and off.ema_iters == 6


# ---------------------------------------------------------------------------------------------------------------- the runner on CPU
YAML = """
train_cfg: {by_epoch: True, max_epochs: 2, val_interval: 1}
model: {type: ema_tiny}
optim_wrapper:
  optimizer: {type: AdamW, lr: 0.05, weight_decay: 0.1}
custom_hooks:
  - type: our_init
%s
"""
HOOK = "  - {type: EMAHook, ema_type: %s, momentum: 0.1, interval: 2, begin_iter: 1%s}\n"


class Tiny(torch.nn.Module):
    def __init__(self, compute_dtype=torch.float32):
        super().__init__()
        self.fc = torch.nn.Linear(6, 5)
        self.bn = torch.nn.BatchNorm1d(5)
        self.head = torch.nn.Linear(5, 6)

    def forward(self, raw, input, label, depth, mode="loss"):
        y = self.head(self.bn(self.fc(input + depth)))
        return {"loss": ((y - label) ** 2).mean()} if mode == "loss" else y


class Checksum:
    """A stand-in evaluator: records what the model's weights were when validation ran."""

    def __init__(self, model):
        self.model, self.results, self.seen = model, [], []

    def process(self, batch, out):
        self.seen.append({k: v.detach().clone() for k, v in self.model.state_dict().items()})

    def compute_metrics(self):
        return {"n": float(len(self.seen))}


def _batches(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [{"input": torch.randn(8, 6, generator=g), "label": torch.randn(8, 6, generator=g), "depth": 0.1 * torch.randn(8, 6, generator=g)}
            for _ in range(n)]


@pytest.fixture
def make_runner(dgtd, tmp_path):
    reg = dgtd.runner.config.MODEL_REGISTRY
    reg["ema_tiny"] = Tiny

    def make(hook=HOOK % (TYPES[0], ""), seed=0):
        torch.manual_seed(seed)
        return dgtd.runner.Runner(dgtd.runner.load_config(YAML % hook), device="cpu", compute_dtype=torch.float32,
                                  work_dir=str(tmp_path), log=lambda m: None)
    yield make
    reg.pop("ema_tiny", None)


def _params64(r):
    return {k: v.detach().double().clone() for k, v in r.model.named_parameters()}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_average_matches_fp64_loop_over_the_recorded_parameters(make_runner, kind):
    r = make_runner(HOOK % (TYPES[kind], ""))
    assert type(r.ema).__name__ == "EmaTorch" and r.ema_cfg["kind"] == kind
    r.model.train()
    e64, big, updates = _params64(r), 0.0, 0
    sched = rule(kind, 0.1, 100.0, 2, 1, 5)
    for it, b in enumerate(_batches(5)):
        r.train_step(b)
        p64 = _params64(r)
        c = sched[it][0]
        assert r.ema.coef == c and r.ema.ema_steps == sched[it][1]
        if c != 0.0:
            updates += 1
            e64 = {k: e64[k] + c * (p64[k] - e64[k]) for k in e64}
        big = max([big] + [float(v.abs().max()) for v in p64.values()] + [float(v.abs().max()) for v in e64.values()])
    got = r.ema.ema_tensors()
    assert set(got) == set(e64)                                  # update_buffers off: parameters only
    worst = max(float((got[k].double() - e64[k]).abs().max()) for k in e64)
    print(f"kind {kind}: {updates} updates, largest magnitude {big:.4f}, worst error {worst:.3e}, bound {updates * EPS * big:.3e}")
    assert updates >= 3 and worst <= updates * EPS * big
    assert any(not torch.equal(got[k], p) for k, p in r.model.named_parameters())          # an average, not a copy


def test_validate_sees_the_average_and_restores_the_weights(make_runner):
    r = make_runner()
    r.model.train()
    for b in _batches(5):
        r.train_step(b)
    ev = Checksum(r.model)
    r.evaluators = [ev]
    raw = {k: v.detach().clone() for k, v in r.model.state_dict().items()}
    avg = {k: v.detach().clone() for k, v in r.ema.ema_tensors().items()}
    assert r.validate(_batches(2, seed=9)) == {"n": 2.0}
    for seen in ev.seen:
        for k, v in seen.items():
            assert torch.equal(v, avg[k] if k in avg else raw[k]), k
    for k, v in r.model.state_dict().items():
        assert torch.equal(v, raw[k]), k                          # bit for bit
    for k, v in r.ema.ema_tensors().items():
        assert torch.equal(v, avg[k]), k
    assert r.model.training


def test_checkpoint_layout_and_round_trip(make_runner, tmp_path):
    r = make_runner()
    r.model.train()
    for b in _batches(5):
        r.train_step(b)
    raw = {k: v.detach().clone() for k, v in r.model.state_dict().items()}
    avg = {k: v.detach().clone() for k, v in r.ema.ema_tensors().items()}
    path = str(tmp_path / "ema.pth")
    r.save(path)
    for k, v in r.model.state_dict().items():
        assert torch.equal(v, raw[k]), k                          # saving exchanges nothing in the live model
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck["ema_state_dict"]) == {"module." + k for k in raw} | {"steps"}
    assert int(ck["ema_state_dict"]["steps"]) == r.ema.ema_steps == 4
    for k in raw:
        assert torch.equal(ck["state_dict"][k], avg[k] if k in avg else raw[k]), k             # the averaged model, as our_init.before_val loads it
        assert torch.equal(ck["ema_state_dict"]["module." + k], raw[k]), k
        assert ck["state_dict"][k].shape == raw[k].shape
    fresh = make_runner(seed=5)
    assert not torch.equal(fresh.model.fc.weight, raw["fc.weight"])
    fresh.resume(path)
    for k, v in fresh.model.state_dict().items():
        assert torch.equal(v, raw[k]), k
    got = fresh.ema.ema_tensors()
    assert set(got) == set(avg) and all(torch.equal(got[k], avg[k]) for k in avg)
    assert fresh.ema.ema_steps == 4 and fresh.ema.ema_iters == 5
    # and the run goes on identically
    nxt = _batches(1, seed=4)[0]
    r.train_step(nxt)
    fresh.model.train()
    fresh.train_step(nxt)
    assert all(torch.equal(a, b) for a, b in zip(r.ema.ema_tensors().values(), fresh.ema.ema_tensors().values()))


@pytest.mark.parametrize("strict", [False, True])
def test_resume_from_a_file_without_ema_state_dict(make_runner, tmp_path, strict):
    plain = make_runner("")                                       # no hook: the file of before
    assert plain.ema is None
    plain.model.train()
    plain.train_step(_batches(1)[0])
    path = str(tmp_path / "plain.pth")
    plain.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"state_dict", "meta", "optimizer"} and ck["meta"] == {"epoch": 0}
    r = make_runner(HOOK % (TYPES[0], ", strict_load: true" if strict else ""), seed=5)
    if strict:
        with pytest.raises(KeyError):
            r.resume(path)
        return
    r.resume(path)
    got = r.ema.ema_tensors()
    for k, p in r.model.named_parameters():
        assert torch.equal(p, ck["state_dict"][k]) and torch.equal(got[k], ck["state_dict"][k]), k
    assert r.ema.ema_steps == 0


def test_update_buffers_and_begin_epoch(make_runner):
    r = make_runner("  - {type: EMAHook, momentum: 0.5, update_buffers: true, begin_epoch: 1}\n")
    assert "bn.running_mean" in r.ema.ema_tensors() and "bn.num_batches_tracked" not in r.ema.ema_tensors()
    data = _batches(3)
    r.train(lambda epoch: data, epochs=1)
    assert r.ema.ema_steps == 0 and r.ema.ema_iters == 3          # epoch 0 < begin_epoch: a copy of the weights
    for k, v in r.ema.ema_tensors().items():
        assert torch.equal(v, r.model.state_dict()[k]), k
    r.train(lambda epoch: data, epochs=2)
    assert r.ema.ema_steps == 3
    assert not torch.equal(r.ema.ema_tensors()["bn.running_mean"], r.model.bn.running_mean)


def test_header_and_ctypes_table_carry_the_new_entries(dgtd):
    import ctypes
    import importlib.util
    spec = importlib.util.spec_from_file_location("_abi", os.path.join(ROOT, "tests", "test_abi.py"))
    abi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(abi)
    decl = abi.header_functions()
    lib = ctypes.CDLL(dgtd._lib.LIB_PATH)
    for name, n in {"dgtd_ema_schedule": 7, "dgtd_adamw_flat_ema": 22, "dgtd_ema_flat": 5, "dgtd_ema_swap": 6}.items():
        assert decl.get(name) == n and len(dgtd._lib.SIGNATURES[name][1]) == n, name
        assert hasattr(lib, name), name
    assert decl["dgtd_adamw_flat_clip"] == 20
