"""Test helper: numpy float64 restatement of dgtd_predict_maps (include/dgtd.h, csrc/predict_maps.hip) and the bound within which
the fp32 kernel must agree with it.

The map of one job, from a logit plane L [S, S] to H x W:

    scale = in / out;  src = max(scale * (dst + 0.5) - 0.5, 0);  i0 = floor(src);  i1 = i0 + (i0 < in - 1);  l = src - i0
    top = (1 - lx) * L[y0, x0] + lx * L[y0, x1];  bot = (1 - lx) * L[y1, x0] + lx * L[y1, x1];  r = (1 - ly) * top + ly * bot
    s = 1 / (1 + exp(-r));   v = 255 * s          (plain)
                             v = 255 * (s - min s) / (max s - min s + 1e-8)    (min-max, extrema over the job's own pixels)
    byte = floor(clamp(v + 0.5, 0, 255)),  NaN -> 0

``coords`` chooses how the TAPS (i0, i1, l) are computed.  ``np.float64`` is F.interpolate in float64 (tests/test_predict_maps_cpu.py
holds it to torch within 1e-12).  ``np.float32`` evaluates the same three lines in float32, operation by operation - IEEE arithmetic, so
these ARE the kernel's taps (the header defines them in fp32, and the file is compiled with contraction off) - which takes the
rounding of the coordinates out of the comparison: a tap weight that is off by d moves r by d * |L[i1] - L[i0]|, which for src near 64
and a neighbour difference of 10 is 1e-4 in r, twenty times the bound below, and says nothing about the kernel.  Everything
downstream of the taps is float64 in both variants.

The bound (``eps_plain`` / ``eps_minmax``), in units of one grey level, with u = 2^-24 (the relative error of one fp32 rounding) and
M = the largest finite |logit| of the input:
  * the blends: 1 - l rounds once, each of the two products and the sum of a blend round once; two horizontal blends feed one
    vertical blend, so along any path from a logit to r there are at most 8 roundings of quantities bounded by M (the weights are
    in [0, 1] and sum to 1 up to u):  |dr| <= 8 u M  ("a few ulps of the largest logit": 4 ulp for a power-of-two M);
  * the sigmoid has slope <= 1/4:  |ds| <= 2 u M from the blends, plus its own evaluation: expf within 1 ulp (2 u relative), the
    addition 1 + e and the division one rounding each, all relative to s <= 1:  |ds| <= 2 u M + 4 u =: es;
  * plain: v = 255 s, then 255 * s and + 0.5 round once each at magnitude <= 256:  eps = 255 es + 512 u.
    For M <= 16 that is 255 * 36 u + 512 u = 5.8e-4 < 1e-3;
  * min-max: s, min s and max s each carry es; numerator and denominator of (s - min) / (max - min + 1e-8) are each off by 2 es plus a
    rounding, and the quotient is at most 1, so |dv01| <= 4 es / R + 4 u with R = max s - min s (the tests keep R >= 0.5);
    eps = 255 (4 es / R + 4 u) + 512 u.

``accepts(byte, v, eps)``: the byte is the quantisation of some v' within eps of v.  Outside the tie band (v + 0.5 within eps of an
integer) that is one exact value, inside it one of two neighbours; never more than one level off."""
import numpy as np

U = 2.0 ** -24


def taps(in_size: int, out_size: int, coords=np.float64):
    """(i0, i1, lam) per output index; ``lam`` is returned as float64 whatever ``coords``."""
    f = coords
    scale = f(in_size) / f(out_size)
    dst = np.arange(out_size).astype(f)
    src = scale * (dst + f(0.5)) - f(0.5)
    src = np.maximum(src, f(0.0))
    assert src.dtype == f
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    lam = src - i0.astype(f)
    assert lam.dtype == f
    return i0, i1, lam.astype(np.float64)


def resize(plane, H: int, W: int, coords=np.float64) -> np.ndarray:
    """Bilinear resize of ``plane`` [S, S] (any float dtype; taken to float64 exactly) to [H, W], horizontal blends first."""
    L = np.asarray(plane, dtype=np.float64)
    y0, y1, ly = taps(L.shape[0], H, coords)
    x0, x1, lx = taps(L.shape[1], W, coords)
    with np.errstate(invalid="ignore"):
        top = (1.0 - lx)[None, :] * L[y0][:, x0] + lx[None, :] * L[y0][:, x1]
        bot = (1.0 - lx)[None, :] * L[y1][:, x0] + lx[None, :] * L[y1][:, x1]
        return (1.0 - ly)[:, None] * top + ly[:, None] * bot


def sigmoid(r: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-r))


def levels(plane, H: int, W: int, minmax: bool = False, coords=np.float32):
    """(v [H, W] float64 in grey levels before the rounding, R): R = max s - min s over the map (NaNs aside), None in plain mode."""
    s = sigmoid(resize(plane, H, W, coords))
    if not minmax:
        return 255.0 * s, None
    if np.isnan(s).all():
        return np.full_like(s, np.nan), 0.0
    mn, mx = np.nanmin(s), np.nanmax(s)
    return 255.0 * (s - mn) / (mx - mn + 1e-8), float(mx - mn)


def quantise(v: np.ndarray) -> np.ndarray:
    """floor(clamp(v + 0.5, 0, 255)) as uint8; NaN -> 0."""
    with np.errstate(invalid="ignore"):
        q = np.floor(np.clip(v + 0.5, 0.0, 255.0))
    return np.where(np.isnan(q), 0.0, q).astype(np.uint8)


def _es(max_abs_logit: float) -> float:
    return 2.0 * U * float(max_abs_logit) + 4.0 * U


def eps_plain(max_abs_logit: float) -> float:
    return 255.0 * _es(max_abs_logit) + 512.0 * U


def eps_minmax(max_abs_logit: float, R: float) -> float:
    assert R > 0.0
    return 255.0 * (4.0 * _es(max_abs_logit) / R + 4.0 * U) + 512.0 * U


def accepts(byte: np.ndarray, v: np.ndarray, eps: float) -> np.ndarray:
    """Elementwise: ``byte == floor(clamp(v' + 0.5, 0, 255))`` for some v' in [v - eps, v + eps]; a NaN v wants 0."""
    assert 0.0 <= eps < 0.5
    b = np.asarray(byte).astype(np.int64)
    lo, hi = quantise(v - eps).astype(np.int64), quantise(v + eps).astype(np.int64)
    return (lo <= b) & (b <= hi)


def tie_share(v: np.ndarray, eps: float) -> float:
    """Share of the pixels whose v + 0.5 lies within eps of an integer (where two bytes are acceptable)."""
    t = v[~np.isnan(v)] + 0.5
    return float(np.mean(np.abs(t - np.round(t)) <= eps)) if t.size else 0.0


def max_abs(plane) -> float:
    a = np.abs(np.asarray(plane, dtype=np.float64))
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


# the target sizes of the GPU test, per source size S: tiny maps, the identity, a non-integer up-sample with both edge clamps, a
# down-sample whose taps skip source pixels, widths that are no multiple of 4 or 16 (head and tail of the stores), many blocks
def target_sizes(S: int):
    return [(1, 1), (1, 7), (S, S), (33, 47), (17, 9), (5, 67), (3, 1), (300, 500)]


def logits(B: int, S: int, seed: int = 0) -> np.ndarray:
    """N(0, 4^2) clipped to |x| <= 16, float32 [B, S, S]."""
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(0.0, 4.0, (B, S, S)), -16.0, 16.0).astype(np.float32)
