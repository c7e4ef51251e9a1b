"""CPU: the exact-rounding helpers of tests/_numerics.py against a brute-force nearest-neighbour search on the 16-bit grids."""
import math

import pytest
import torch

import _numerics as nm

HALVES = [torch.bfloat16, torch.float16]


def _grid(dtype):
    """Every finite value of a 16-bit type, ascending, plus +-inf as the grid points beyond the largest finite value (the value one
    step past it, 2^(emax+1), has an even significand: midpoints there round to inf)."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype).to(torch.float64)
    v = v[torch.isfinite(v)]
    v = torch.unique(v)                                   # +0 and -0 collapse; ties at 0 are decided by sign separately
    return torch.cat([v.new_tensor([-math.inf]), v, v.new_tensor([math.inf])])


def _brute(x64, dtype):
    """Nearest grid value, ties to the even significand; beyond the largest finite value the neighbour is 2^(emax+1) -> inf."""
    grid = _grid(dtype)
    fi = torch.finfo(dtype)
    big = 2.0 ** (math.log2(fi.max) // 1 + 1)
    gnum = grid.clone()
    gnum[0], gnum[-1] = -big, big
    i = torch.searchsorted(gnum, x64).clamp(1, len(gnum) - 1)
    a, b = gnum[i - 1], gnum[i]
    da, db = (x64 - a).abs(), (b - x64).abs()
    ga, gb = grid[i - 1], grid[i]
    # the even neighbour: significand bit 0 of the 16-bit pattern (inf counts as even: it stands for 2^(emax+1))
    def even(g):
        bits = g.to(dtype).view(torch.int16).to(torch.int32)
        return (bits & 1) == 0
    pick_b = (db < da) | ((db == da) & even(gb))
    out = torch.where(pick_b, gb, ga)
    out = torch.where(x64 == b, gb, out)
    out = torch.where(x64 == a, ga, out)
    out = torch.where(torch.isinf(x64), x64, out)
    # zero keeps the sign of the input (a value that rounds to 0 from below is -0)
    out = torch.where(out == 0, torch.copysign(torch.zeros_like(out), x64), out)
    return out


def _same(a, b):
    """bitwise equality of 16-bit tensors (NaN payloads aside)"""
    an, bn = torch.isnan(a.float()), torch.isnan(b.float())
    return bool(((a.view(torch.int16) == b.view(torch.int16)) | (an & bn)).all())


def _constructed(dtype):
    """midpoints of every adjacent pair of finite values, +-1 fp64 ulp around them, extremes and overflow thresholds"""
    g = _grid(dtype)[1:-1]
    fi = torch.finfo(dtype)
    mid = (g[:-1] + g[1:]) / 2
    up, dn = torch.nextafter(mid, torch.tensor(math.inf, dtype=torch.float64)), torch.nextafter(mid, torch.tensor(-math.inf, dtype=torch.float64))
    mx = fi.max
    p = {torch.bfloat16: 8, torch.float16: 11}[dtype]
    thr = mx + 2.0 ** (math.floor(math.log2(mx)) - p)      # overflow threshold: 65520 for fp16, (2 - 2^-8) 2^127 for bf16
    tiny_sub = 2.0 ** (math.log2(fi.tiny) - (p - 1))
    special = torch.tensor([0.0, -0.0, tiny_sub, -tiny_sub, tiny_sub / 2, tiny_sub / 2 * (1 + 2 ** -40), tiny_sub * 0.75, tiny_sub * 1.5,
                            fi.tiny, fi.tiny * (1 - 2 ** -30), mx, -mx, thr, -thr, thr * (1 - 2 ** -50), thr * (1 + 2 ** -50), 1e300, -1e300,
                            math.inf, -math.inf, 1 + 2 ** -8 + 2 ** -40, 1 + 2 ** -11 + 2 ** -40], dtype=torch.float64)
    return torch.cat([mid, up, dn, special])


def test_overflow_thresholds():
    assert nm.round_to(torch.tensor([65519.99, 65520.0], dtype=torch.float64), torch.float16).tolist() == [65504.0, math.inf]
    t = (2 - 2 ** -8) * 2.0 ** 127
    r = nm.round_to(torch.tensor([t * (1 - 2 ** -30), t, -t], dtype=torch.float64), torch.bfloat16)
    assert r[0].item() == torch.finfo(torch.bfloat16).max and r[1].item() == math.inf and r[2].item() == -math.inf


@pytest.mark.parametrize("dtype", HALVES, ids=str)
def test_double_rounding_case(dtype):
    """the case torch's fp64 -> 16-bit cast gets wrong (it goes through fp32 and rounds twice)"""
    p = {torch.bfloat16: 8, torch.float16: 11}[dtype]
    x = torch.tensor([1 + 2.0 ** -p + 2.0 ** -40], dtype=torch.float64)
    assert nm.round_to(x, dtype).item() == 1 + 2.0 ** (1 - p)


@pytest.mark.parametrize("dtype", HALVES, ids=str)
def test_round_to_constructed_cases(dtype):
    x = _constructed(dtype)
    assert _same(nm.round_to(x, dtype), _brute(x, dtype).to(dtype))


@pytest.mark.parametrize("dtype", HALVES, ids=str)
def test_round_to_random_sample(dtype):
    g = torch.Generator().manual_seed(7)
    fi = torch.finfo(dtype)
    # log-uniform magnitudes over the whole range including the subnormals and past the overflow threshold, random signs
    e = torch.rand(400_000, generator=g, dtype=torch.float64) * (math.log2(fi.max) - math.log2(fi.tiny) + 14) + math.log2(fi.tiny) - 12
    x = torch.exp2(e) * torch.where(torch.rand(400_000, generator=g) < 0.5, -1.0, 1.0).double()
    assert _same(nm.round_to(x, dtype), _brute(x, dtype).to(dtype))


def test_round_to_nan_and_fp32():
    x = torch.tensor([math.nan, 1 + 2 ** -30, -0.0, 1e-310], dtype=torch.float64)
    for dt in HALVES:
        r = nm.round_to(x, dt)
        assert math.isnan(r[0].item()) and r[1].item() == 1.0 and r[2].item() == 0 and math.copysign(1, r[2].item()) < 0
        assert r[3].item() == 0
    r = nm.round_to(x, torch.float32)
    assert r.dtype == torch.float32 and math.isnan(r[0].item()) and r[1].item() == 1.0


def test_bracket_and_assert_bracketed():
    ref = torch.tensor([1.0, 1.0 + 2 ** -8, 100.0, math.inf, math.nan, 70000.0], dtype=torch.float64)
    err = torch.tensor([1e-6, 1e-6, 1.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    lo, hi = nm.bracket(ref, err, torch.bfloat16)
    # 1 + 2^-8 is a bf16 midpoint: +-err straddles it, both neighbours are legal
    assert lo.tolist()[:3] == [1.0, 1.0, 99.0] and hi.tolist()[:3] == [1.0, 1.0078125, 101.0]
    assert lo[3].item() == hi[3].item() == math.inf and math.isnan(lo[4].item())
    got = torch.tensor([1.0, 1.0078125, 100.0, math.inf, math.nan, 70144.0], dtype=torch.bfloat16)
    nm.assert_bracketed(got, lo, hi, "ok", ref=ref, err=err)
    with pytest.raises(AssertionError, match="1 of 6"):
        nm.assert_bracketed(torch.tensor([1.0, 1.0078125, 102.0, math.inf, math.nan, 70144.0], dtype=torch.bfloat16), lo, hi, "x", ref=ref, err=err)
    with pytest.raises(AssertionError, match="NaN mismatches"):
        nm.assert_bracketed(torch.tensor([1.0, 1.0, 100.0, math.inf, 0.0, 70144.0], dtype=torch.bfloat16), lo, hi, "x")
    with pytest.raises(AssertionError):
        nm.assert_bracketed(torch.tensor([math.nan, 1.0, 100.0, math.inf, math.nan, 70144.0], dtype=torch.bfloat16), lo, hi, "x")
    # fp16 overflow: the correctly rounded 70000 is inf, a saturated 65504 is outside
    lo, hi = nm.bracket(ref[5:], err[5:], torch.float16)
    assert lo.item() == hi.item() == math.inf
    with pytest.raises(AssertionError):
        nm.assert_bracketed(torch.tensor([65504.0], dtype=torch.float16), lo, hi, "sat")


def test_assert_sharp():
    ref = torch.linspace(1, 2, 1001, dtype=torch.float64)
    lo, hi = nm.bracket(ref, torch.full_like(ref, 1e-7), torch.bfloat16)
    assert nm.assert_sharp(lo, hi) > 0.99
    lo, hi = nm.bracket(ref, torch.full_like(ref, 2.0 ** -9), torch.bfloat16)   # one ulp wide: every bracket admits two values
    with pytest.raises(AssertionError, match="single value"):
        nm.assert_sharp(lo, hi)


def test_ratio_excludes_final_rounding():
    ref = torch.tensor([1.0 + 2 ** -10], dtype=torch.float64)
    assert nm.ratio(torch.tensor([1.0], dtype=torch.bfloat16), ref, torch.tensor([1e-7], dtype=torch.float64)) == 0.0
    assert nm.ratio(torch.tensor([1.0078125], dtype=torch.bfloat16), ref, torch.tensor([2.0 ** -9], dtype=torch.float64)) == pytest.approx(1.5)
