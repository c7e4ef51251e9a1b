"""Shared pieces of the rounding-level kernel tests (imported as ``_kernel_check``; not a conftest): the error constants, the
NaN-guarded buffers and the bit-reproducibility helpers.  Nothing here touches the GPU at import time."""
from __future__ import annotations

import math

import torch

import _numerics as nm

DEV = "cuda"
F64 = torch.float64

# ---- error constants (each with its source; none is fitted to an observed error)
U32 = 2.0 ** -24            # unit roundoff of one fp32 rounding to nearest
# fp32 accumulation of a 16-bit MFMA reduction of length <= 4096 (16-bit products are exact in fp32): cdna_hip_programming.md
# § "FP32-input MFMA" measured 0.75-1.5e-7 * sum|a b| at K <= 1024 and 3.5e-7 at K = 4096 against fp64; 2^-21 = 4.8e-7 covers both
C_MFMA = 2.0 ** -21
MFMA_MAX_K = 4096


class Buf:
    """A tensor of `shape` at a 16-byte aligned, non-zero offset inside a NaN-filled buffer (pad elements on either side)."""

    def __init__(self, shape, dtype, init=None, pad=None):
        n = math.prod(shape)
        last = shape[-1] if shape else 1
        self.pad = pad if pad is not None else (3 * last if last % 8 == 0 and last <= 4096 else 24)
        assert self.pad % 8 == 0 and self.pad > 0
        self.flat = torch.full((n + 2 * self.pad,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.flat[self.pad:self.pad + n].view(shape)
        if init is not None:
            self.t.copy_(init)
        assert self.t.data_ptr() % 16 == 0

    @property
    def p(self):
        return self.t.data_ptr()

    def guards_intact(self, name):
        g = torch.cat([self.flat[:self.pad], self.flat[self.pad + self.t.numel():]])
        assert bool(torch.isnan(g.float()).all()), f"{name}: the kernel wrote outside its output"


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _same_bits(a, b, name):
    assert torch.equal(_bits(a), _bits(b)), f"{name}: a second launch on the same inputs gave different bits"


def _run_twice(fn, outs, name):
    """launch fn(out buffers) into two sets of NaN-filled buffers, require identical bits, return the first set"""
    first = [Buf(o[0], o[1]) for o in outs]
    fn(first)
    second = [Buf(o[0], o[1]) for o in outs]
    fn(second)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(first, second)):
        x.guards_intact(f"{name}[{i}]")
        _same_bits(x.t, y.t, f"{name}[{i}]")
    return [x.t for x in first]


def check_bracketed(got, ref, err, dtype, name, family, margins):
    """got in [round(ref - err), round(ref + err)], NaN exactly where ref is NaN; records the share of err used under `family`.
    (The bracket check of test_kernel_numerics_gpu._check without its sharpness step: a bound that contains a 16-bit rounding of an
    intermediate is a few output ulps wide and cannot be single-valued; what such a bound can see is shown by mutation instead.)"""
    lo, hi = nm.bracket(ref, err, dtype)
    nm.assert_bracketed(got, lo, hi, name, ref=ref, err=err)
    share = nm.ratio(got, ref, err)
    margins[family] = max(margins.get(family, 0.0), share)
    return share
