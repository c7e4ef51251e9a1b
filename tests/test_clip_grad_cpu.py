"""CPU: ``optim_wrapper.clip_grad`` (config/cod.yml:108-110, mmengine's OptimWrapper) - the spellings the runner accepts, the torch
path of the CPU optimizer, and the C ABI of the device path (header and ctypes table; no compute calls)."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"dgtd_grad_norm_partial": 7, "dgtd_grad_clip_finalize": 7, "dgtd_adamw_flat_clip": 20}


def header_functions():
    text = open(os.path.join(ROOT, "include", "dgtd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|int64_t|const char\*)\s+(dgtd_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        out[m.group(2)] = len([a for a in m.group(3).split(",") if a.strip() and a.strip() != "void"])
    return out


@pytest.fixture(scope="module")
def dgtd():
    import __graft_entry__ as ge
    ge.build()
    import dgtd as m
    return m


def test_accepted_spellings_parse(dgtd):
    parse = dgtd.runner.parse_clip_grad
    assert parse(None) is None
    assert parse({"max_norm": 35, "norm_type": 2}) == {"type": "norm", "max_norm": 35.0, "norm_type": 2.0}
    assert parse({"max_norm": 0.5}) == {"type": "norm", "max_norm": 0.5, "norm_type": 2.0}
    assert parse({"type": "norm", "max_norm": 1.0, "norm_type": "inf"}) == {"type": "norm", "max_norm": 1.0, "norm_type": math.inf}
    assert parse({"max_norm": 1.0, "norm_type": float("inf")})["norm_type"] == math.inf
    assert parse({"type": "value", "clip_value": 0.5}) == {"type": "value", "clip_value": 0.5}


@pytest.mark.parametrize("bad", [
    {}, "norm", {"type": "norm"}, {"type": "value"}, {"type": "value", "max_norm": 1.0}, {"type": "norm", "clip_value": 0.5},
    {"max_norm": 1.0, "clip_value": 0.5}, {"type": "value", "max_norm": 1.0, "clip_value": 0.5},
    {"max_norm": 1.0, "norm_type": 1}, {"max_norm": 1.0, "norm_type": 3.0}, {"max_norm": 1.0, "norm_type": "l2"},
    {"max_norm": 0.0}, {"max_norm": -1.0}, {"max_norm": float("nan")}, {"max_norm": float("inf")}, {"max_norm": "1"},
    {"type": "value", "clip_value": 0}, {"type": "value", "clip_value": -0.5}, {"type": "l2", "max_norm": 1.0},
    {"max_norm": 1.0, "error_if_nonfinite": True},
], ids=repr)
def test_bad_spellings_raise(dgtd, bad):
    with pytest.raises(ValueError):
        dgtd.runner.parse_clip_grad(bad)


def test_key_is_read_from_the_yaml(dgtd):
    """The runner reads ``optim_wrapper.clip_grad`` where the reference's file carries it; without the key nothing is clipped."""
    base = "optim_wrapper:\n  type: AmpOptimWrapper\n  optimizer: {type: AdamW, lr: 0.0005}\n"
    get = lambda text: dgtd.runner.parse_clip_grad(dgtd.runner.load_config(text)["optim_wrapper"].get("clip_grad"))
    assert get(base) is None
    assert get(base + "  clip_grad:\n    type: value\n    clip_value: 0.5\n") == {"type": "value", "clip_value": 0.5}
    assert get(base + "  clip_grad: {max_norm: 35, norm_type: 2}\n") == {"type": "norm", "max_norm": 35.0, "norm_type": 2.0}
    assert get(base + "  clip_grad: {max_norm: 1.5, norm_type: inf}\n")["norm_type"] == math.inf
    with pytest.raises(ValueError):
        get(base + "  clip_grad: {max_norm: 35, norm_type: 1}\n")


def _toy():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.LayerNorm(7))     # weight, bias, weight (+ one bias left without gradient)
    g = torch.Generator().manual_seed(1)
    for p in list(net.parameters())[:3]:
        p.grad = torch.randn(p.shape, generator=g) * 3.0
    return net


@pytest.mark.parametrize("clip", [{"max_norm": 2.0}, {"max_norm": 1e4, "norm_type": 2}, {"type": "norm", "max_norm": 0.7, "norm_type": "inf"},
                                  {"type": "value", "clip_value": 0.5}], ids=repr)
def test_cpu_helper_is_torchs_utilities(dgtd, clip):
    """Bit for bit the direct call: same parameters (those with a gradient), same arguments, same return value."""
    a, b = _toy(), _toy()
    got = dgtd.runner.clip_grad_torch(a.parameters(), clip)
    have = [p for p in b.parameters() if p.grad is not None]
    assert len(have) == 3
    if clip.get("type") == "value":
        torch.nn.utils.clip_grad_value_(have, clip["clip_value"])
        assert got is None
        assert max(float(p.grad.abs().max()) for p in have) == 0.5
    else:
        want = torch.nn.utils.clip_grad_norm_(have, clip["max_norm"], norm_type=float(clip.get("norm_type", 2)))
        assert torch.equal(got, want)
    for p, q in zip(a.parameters(), b.parameters()):
        assert (p.grad is None) == (q.grad is None)
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad)
    before = [None if p.grad is None else p.grad.clone() for p in a.parameters()]
    assert dgtd.runner.clip_grad_torch(a.parameters(), None) is None            # key absent: gradients untouched
    for p, q in zip(a.parameters(), before):
        assert p.grad is None or torch.equal(p.grad, q)


def test_header_and_ctypes_table_carry_the_new_entries(dgtd):
    decl = header_functions()
    for name, n in NEW_ENTRIES.items():
        assert decl.get(name) == n, (name, decl.get(name))
        assert name in dgtd._lib.SIGNATURES and len(dgtd._lib.SIGNATURES[name][1]) == n, name
    import ctypes
    lib = ctypes.CDLL(dgtd._lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), f"{name} declared in dgtd.h but not exported"
    # the entries that were there keep their signatures
    assert decl["dgtd_adamw_flat"] == 14 and decl["dgtd_adamw_flat_amp"] == 17 and decl["dgtd_adamw_flat_g16"] == 17 and decl["dgtd_found_inf"] == 4


def test_flat_adamw_validates_at_construction(dgtd):
    """The dict is checked before the optimizer looks at a bucket: a bad one never reaches a step."""
    class NoBuckets:
        buckets, working_dtype, world = [], None, 1
    with pytest.raises(ValueError):
        dgtd.runner.FlatAdamW(NoBuckets(), clip_grad={"max_norm": 1.0, "norm_type": 1})
    with pytest.raises(ValueError):
        dgtd.runner.FlatAdamW(NoBuckets(), clip_grad={"max_norm": 1.0, "clip_value": 1.0})
    assert dgtd.runner.FlatAdamW(NoBuckets()).grad_norm() is None
