"""Exact-rounding helpers for rounding-level kernel tests (imported by the test files as ``_numerics``; not a conftest).

A kernel that evaluates an expression with an internal arithmetic error of at most ``err`` and rounds the result once to ``dtype``
may legally return any representable value in [round(ref - err), round(ref + err)] (rounding is monotone).  ``bracket`` computes that
interval from an fp64 reference, ``assert_bracketed`` checks a kernel output against it, and ``assert_sharp`` shows that the interval
is a single value almost everywhere, i.e. that the check would catch one extra rounding.
"""
from __future__ import annotations

import torch

_I32 = torch.int32


def round_to(x64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Correct round-to-nearest-even of fp64 values to ``dtype`` (bf16, fp16 or fp32): subnormals, overflow to +-inf, +-0, NaN.

    fp64 -> fp32 is one correct rounding.  For the 16-bit types the value first goes to fp32 with round-to-ODD (truncate, then set the
    last bit when anything was cut off): with 24 >= p + 2 bits that intermediate rounds to the same 16-bit value as the fp64 input, so
    the second (nearest-even) rounding is exact.  ``tensor.to(bfloat16)`` on fp64 rounds twice to nearest and is wrong at midpoints."""
    x64 = x64.to(torch.float64)
    y = x64.to(torch.float32)
    if dtype == torch.float32:
        return y
    assert dtype in (torch.bfloat16, torch.float16), dtype
    inexact = (y.to(torch.float64) != x64) & ~torch.isnan(x64)
    bits = y.view(_I32)
    # y rounded AWAY from zero (|y| > |x|): step one ulp back toward zero (sign-magnitude: magnitude - 1); inf -> the largest finite
    away = inexact & (y.to(torch.float64).abs() > x64.abs())
    bits = torch.where(away, bits - 1, bits)
    bits = torch.where(inexact, bits | 1, bits)                # sticky bit: round to odd
    return bits.view(torch.float32).to(dtype)


def ulp(x64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of the ``dtype`` grid at |x| (the subnormal spacing below the smallest normal), in fp64."""
    fi = torch.finfo(dtype)
    p = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}[dtype]
    a = x64.to(torch.float64).abs().clamp(min=fi.tiny)
    e = torch.floor(torch.log2(a))
    e = torch.where(torch.exp2(e) > a, e - 1, e)               # log2 rounding at exact powers of two
    e = torch.where(torch.exp2(e + 1) <= a, e + 1, e)
    return torch.exp2(e - (p - 1))


def bracket(ref64: torch.Tensor, err64: torch.Tensor, dtype: torch.dtype):
    """(lo, hi) = (round(ref - err), round(ref + err)) in ``dtype``: the outputs a kernel with internal error <= err may produce.
    Infinite references (an infinite operand) and NaN references are passed through exactly."""
    ref64, err64 = ref64.to(torch.float64), err64.to(torch.float64)
    lo, hi = round_to(ref64 - err64, dtype), round_to(ref64 + err64, dtype)
    inf = torch.isinf(ref64)
    r = round_to(ref64, dtype)
    return torch.where(inf, r, lo), torch.where(inf, r, hi)


def assert_bracketed(got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, name: str, ref=None, err=None) -> None:
    """lo <= got <= hi everywhere, NaN exactly where the reference (lo) is NaN.  ref / err (fp64, optional) enrich the message."""
    assert got.shape == lo.shape == hi.shape, (name, got.shape, lo.shape, hi.shape)
    g, l, h = got.to(torch.float64), lo.to(torch.float64), hi.to(torch.float64)
    gn, ln = torch.isnan(g), torch.isnan(l)
    bad_nan = gn != ln
    bad = bad_nan | (~ln & ~gn & ((g < l) | (g > h)))
    n = int(bad.sum())
    if n == 0:
        return
    r = ref.to(torch.float64) if ref is not None else (l + h) / 2
    dist = torch.where(bad, (g - r).abs(), torch.zeros_like(g))
    dist = torch.where(bad & torch.isnan(dist), torch.full_like(dist, float("inf")), dist)
    i = int(torch.argmax(dist.reshape(-1)))
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
    gv, rv = g.reshape(-1)[i].item(), r.reshape(-1)[i].item()
    u = ulp(r.reshape(-1)[i:i + 1], got.dtype if got.dtype != torch.float64 else torch.float32).item()
    ev = err.to(torch.float64).reshape(-1)[i].item() if err is not None else float("nan")
    raise AssertionError(f"{name}: {n} of {got.numel()} outputs outside the rounding bracket ({int(bad_nan.sum())} NaN mismatches); "
                         f"worst at {idx}: got {gv!r}, ref {rv!r} ({(gv - rv) / u:+.2f} ulp), allowed "
                         f"[{l.reshape(-1)[i].item()!r}, {h.reshape(-1)[i].item()!r}], err {ev!r}")


def assert_sharp(lo: torch.Tensor, hi: torch.Tensor, min_frac: float = 0.9, name: str = "") -> float:
    """At least ``min_frac`` of the (non-NaN) brackets admit exactly one value: the bound is not vacuous.  Returns the fraction."""
    keep = ~torch.isnan(lo.to(torch.float32))
    n = int(keep.sum())
    if n == 0:
        return 1.0
    frac = float(((lo == hi) & keep).sum()) / n
    assert frac >= min_frac, f"{name}: only {frac:.3f} of the brackets are a single value (need {min_frac}): the bound cannot see one rounding"
    return frac


def ratio(got: torch.Tensor, ref64: torch.Tensor, err64: torch.Tensor) -> float:
    """How much of the bound a kernel uses: max over the finite outputs with err > 0 of the deviation the final rounding does not
    explain, (|got - ref| - ulp(got) / 2)+ / err.  At most 1 for every output inside its bracket."""
    g, r, e = got.to(torch.float64), ref64.to(torch.float64), err64.to(torch.float64)
    m = torch.isfinite(g) & torch.isfinite(r) & (e > 0)
    if not bool(m.any()):
        return 0.0
    dev = ((g - r).abs() - ulp(g, got.dtype) / 2).clamp(min=0)
    return float((dev[m] / e[m]).max())
