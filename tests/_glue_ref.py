"""fp64 references, error models, kernel-arithmetic emulations and launch-geometry mirrors of the Hitnet decoder glue
(csrc/hitnet_glue.hip: shared-slope PReLU, the CA channel gate, bilinear resize; csrc/sam.hip).  Device-agnostic torch, test helper only
(imported as ``_glue_ref``; not a conftest).  What the error models can see is shown by mutation in test_glue_numerics_cpu.py.

Layout: feature maps are token matrices [B, HW, C] (bilinear: [B, H, W, C]) in the I/O type T (bf16, fp16 or fp32); weights, stats and
weight gradients are fp32.  Every reference is fp64 on the exact stored operands; where a kernel stores an intermediate (pooled sums,
hidden units, gates) the next stage's reference starts from the STORED value, so each stage is held to its own arithmetic.  Every bound
is a constant times the same expression on absolute values.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

import _numerics as nm
from _attn_ref import EXP_LIB, RCP, outside  # noqa: F401 (RCP: see DIV; outside: shared with the tests)
from _kernel_check import U32

F64 = torch.float64
F32 = torch.float32
HALVES = (torch.bfloat16, torch.float16)

# ---- error constants (each with its source; none is fitted to an observed error)
# `a / b` in device code: clang's documented default for HIP is -fhip-fp32-correctly-rounded-divide-sqrt ("single precision divide and
# sqrt used in the program source are correctly rounded"), the build passes no fast-math flag, and the generated code of both files is
# the v_div_scale / v_rcp / v_fma / v_div_fixup sequence: one rounding.  (RCP = 2 U32 would be the allowance for a bare v_rcp_f32.)
DIV = U32
# a gate below 2^-126 may be flushed or lost when expf overflows (1 / (1 + inf) = 0): absolute, as FLUSH32 in _attn_ref
FLUSH32 = 2.0 ** -126
# bilinear: roundings on one tap's path from the pixel to the output.  forward: (1 - l) once per axis, the inner product and add, the
# outer product and add = 6.  backward: (1 - l) and the add of the two tap parts per axis (4), wy * wx, wgt * g = 6, plus the chain.
BIL_FWD_TAP = 6
BIL_BWD_TAP = 6


def vec(dtype):
    """elements per 16-byte chunk (Vec16<T>::N)"""
    return 4 if dtype == F32 else 8


def cdiv(a, b):
    return -(-a // b)


def gamma(n):
    """n roundings in a chain: n u / (1 - n u)"""
    return n * U32 / (1.0 - n * U32)


def fl32(x):
    return x.to(F32).to(F64)


def rt(x, dtype):
    return nm.round_to(x, dtype).to(F64)


def store(x, dtype):
    """what a kernel stores when it rounds an fp32 result to T: fp64 -> fp32 -> T"""
    return rt(fl32(x), dtype)


def _finite(err, ref):
    """an infinite or NaN reference carries no error term (bracket() passes it through exactly)"""
    return torch.where(torch.isfinite(ref), err, torch.zeros_like(err))


def relu(x):
    return torch.where(x < 0, torch.zeros_like(x), x)          # keeps NaN, as F.relu does


def sigmoid_terms(a, da):
    """1 / (1 + expf(-a)) for a pre-activation known to +-da: (value, bound).  First order in the exponent: the relative error of
    e = expf(-a) is da + EXP_LIB and d gate / gate = -(1 - gate) d e / e; then the add and the division."""
    gate, comp = torch.sigmoid(a), torch.sigmoid(-a)
    return gate, _finite(gate * comp * (da + EXP_LIB) + gate * (U32 + DIV), a) + FLUSH32


def sharpness(ref, err, at):
    """(share of single-valued brackets among the elements that are not ties, share of ties) at the resolution of dtype `at`.  A tie
    is an element whose fp64 reference is a midpoint of the `at` grid (dyadic resize ratios average 16-bit values and produce them):
    either neighbour is a correct rounding of a result that is off by one fp32 rounding, so no bound can be sharp there.  A reference
    within 2^-12 ulp of a midpoint counts as one: the fp32 rounding of a scale such as 2/3 moves a true tie by about 2^-24 of the
    value, and a generic element falls into that zone with probability 2^-11."""
    ok = torch.isfinite(ref) & torch.isfinite(err)
    r, u = rt(ref, at), nm.ulp(ref, at)
    tie = ok & (((ref - r).abs() - u / 2).abs() <= u * 2.0 ** -12)
    lo, hi = nm.bracket(ref, err, at)
    keep = ok & ~tie
    n = int(keep.sum())
    return (float(((lo == hi) & keep).sum()) / n if n else 1.0), float(tie.sum()) / max(1, int(ok.sum()))


# ============================================================================================== PReLU
PRELU_SLOPES = (0.25, float(torch.tensor(0.3, dtype=F32)), -0.5, 0.0)


def prelu_plan(n, dtype):
    """(forward grid, forward trips per thread, backward grid, backward trips per thread) of dgtd_prelu_fwd / _bwd"""
    chunks = n // vec(dtype)
    gf = min(cdiv(chunks, 256), 2048)
    gb = min(gf, 512)
    return gf, cdiv(chunks, gf * 256), gb, cdiv(chunks, gb * 256)


# n / V -> plan, read off ew_grid and the two launches by hand
PRELU_CASES = {
    1: (1, 1, 1, 1),                                   # one chunk, 255 idle threads
    256 * 3 + 77: (4, 1, 4, 1),                        # several workgroups, ragged last one
    512 * 256 + 77: (513, 1, 512, 2),                  # the backward's grid-stride loop with a ragged second trip
    2048 * 256 + 5: (2048, 2, 512, 5),                 # the forward's grid-stride loop
}


def prelu_inputs(n, dtype, seed=0, specials=False):
    g_ = torch.Generator(device="cpu").manual_seed(100 + seed)
    x = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_) + 0.5              # non-zero mean: da = sum_{x <= 0} g x does not cancel
    # the last chunk (the ragged tail of the grid-stride loops) carries weight: da's chain bound grows like n (about 2^-15 sum |g x|
    # at 512 workgroups), so a lost chunk shows at every n only if its terms grow like n too: 8 * (2 + n 2^-16) per element
    V = 4 if dtype == torch.float32 else 8
    if n > V:
        x[-V:], g[-V:] = -8.0, 2.0 + n * 2.0 ** -16
    if specials:
        assert n >= 64
        x[3], x[9], x[17], x[20], x[33], x[41] = 0.0, -0.0, 2.0 ** -24, -3 * 2.0 ** -24, float("inf"), float("-inf")
        x[50] = float("nan")
    return x.to(dtype), g.to(dtype)


def prelu_ref(x, g, slope, da0, dtype):
    """y = x > 0 ? x : slope x and dx likewise on g: the fp64 product of an fp32 slope and a <= 24-bit value is exact.  The kernel
    rounds it to fp32 and then to T, or, for fp16 under -ffp-contract=fast, once (the compiler folds the conversion into a mixed-
    precision multiply, v_fma_mixlo_f16): the bound admits both, U32 |slope x| for the 16-bit types and 0 for fp32.
    da = da0 + sum_{not x > 0} g x with its chain bound: V adds per trip and thread, 6 butterfly levels, 3 adds of the four waves, one
    atomic per workgroup (in any order); fp32 inputs also round the product (or fuse it)."""
    x64, g64, s = x.to(F64), g.to(F64), float(slope)
    pos = x64 > 0
    u = 0.0 if dtype == F32 else U32
    zero = torch.zeros_like(x64)
    y, dx = torch.where(pos, x64, s * x64), torch.where(pos, g64, s * g64)
    t = torch.where(pos, zero, g64 * x64)
    _, _, gb, trips = prelu_plan(x.numel(), dtype)
    chain = vec(dtype) * trips + 6 + 3 + gb + (1 if dtype == F32 else 0)
    return SimpleNamespace(y=y, y_err=_finite(torch.where(pos, zero, u * y.abs()), y), dx=dx, dx_err=_finite(torch.where(pos, zero, u * dx.abs()), dx),
                           da=da0 + t.sum(), da_err=gamma(chain) * (abs(da0) + t.abs().sum()))


PRELU_MUTATIONS = ("slope_bf16", "da_last_chunk")


def prelu_emulate(x, g, slope, da0, dtype, mutate=None):
    assert mutate is None or mutate in PRELU_MUTATIONS, mutate
    x64, g64, s = x.to(F64), g.to(F64), float(slope)
    if mutate == "slope_bf16":
        s = float(torch.tensor(s, dtype=F32).to(torch.bfloat16))
    pos = x64 > 0
    t = torch.where(pos, torch.zeros_like(x64), g64 * x64)
    if mutate == "da_last_chunk":
        t = t[:-vec(dtype)]
    return SimpleNamespace(y=torch.where(pos, x64, store(s * x64, dtype)), dx=torch.where(pos, g64, store(s * g64, dtype)),
                           da=fl32(da0 + t.sum()))


# ============================================================================================== pooled sums (CA gate and SAM)
def pool_geometry(HW, C, dtype):
    """pooled_sum_kernel / sam_pool_kernel: CV chunks per row, rpp rows per pass, gx slices (<= 64), rows one thread sums, and the
    longest chain of fp32 additions: the per-thread rows, the rpp row slots met in LDS, the two running sums over the slices + 1"""
    CV = C // vec(dtype)
    rpp = 256 // CV
    gx = max(1, min(cdiv(HW, max(1, 256 // C) * 8), 64))
    rows = cdiv(HW, gx * rpp)
    return SimpleNamespace(CV=CV, rpp=rpp, gx=gx, rows=rows, chain=rows + rpp + cdiv(gx, 2) + 1)


def apply_grid(HW, C, dtype):
    return max(1, min(cdiv(HW * (C // vec(dtype)), 512), 128))


def _slice_of_row(HW, geo):
    r = torch.arange(HW)
    return (r // geo.rpp) % geo.gx


def _pooled_emulated(v64, geo, drop_tail):
    """sum over HW of [.., HW, C] as the kernels slice it; drop_tail: the odd-count tail slice of the two-running-sum walk is skipped"""
    if not (drop_tail and geo.gx % 2 == 1):
        return fl32(v64.sum(-2))
    keep = (_slice_of_row(v64.shape[-2], geo) != geo.gx - 1).to(v64.device)
    return fl32((v64 * keep[:, None]).sum(-2))


# ============================================================================================== CA gate
def ca_plan(B, HW, C, R, dtype):
    """(CV, rpp, gx, apply grid, backward path) of dgtd_ca_gate_fwd / _bwd"""
    geo = pool_geometry(HW, C, dtype)
    return geo.CV, geo.rpp, geo.gx, apply_grid(HW, C, dtype), ("fused" if B <= 32 else "two-kernel")


def ca_stats_floats(B, C, R):
    return 2 * B * C + B * R + 64 * B * C


def ca_scratch_floats(B, C, R):
    return B * C + 64 * B * C + B * 2 * R * C


# (B, HW, C, R) per type family -> plan, read off hitnet_glue.hip by hand.  rows: also run dgtd_ca_gate_bwd_rows.
CA_CASES_16 = {
    (1, 1, 8, 1): (1, 256, 1, 1, "fused"),               # CV = 1, one row, R = 1
    (2, 7, 24, 6): (3, 85, 1, 1, "fused"),               # CV = 3: thread 255 idle; fewer rows than row slots
    (2, 63, 32, 8): (4, 64, 1, 1, "fused"),              # one slice, one row short of the row slots
    (2, 130, 32, 32): (4, 64, 3, 2, "fused"),            # 3 slices: the odd tail of the two running sums; R = 32
    (2, 100, 64, 16): (8, 32, 4, 2, "fused"),            # 4 slices (HW = 100 / 32 rows)
    (1, 45, 96, 24): (12, 21, 3, 2, "fused"),            # CV = 12, rpp = 21 (4 idle threads), 3 slices, the last with 3 rows
    (2, 20, 128, 32): (16, 16, 2, 1, "fused"),           # 2 slices
    (1, 4096, 32, 8): (4, 64, 64, 32, "fused"),          # 64 x 64: exactly the 64-slice cap
    (1, 1100, 128, 1): (16, 16, 64, 35, "fused"),        # cap exceeded: 69 slices wanted, two rows per thread
    (1, 16400, 32, 8): (4, 64, 64, 128, "fused"),        # HW * CV = 65600 > 65536: the apply grid cap of 128
    (32, 9, 32, 8): (4, 64, 1, 1, "fused"),              # the fused backward's cap and its largest LDS
    (33, 9, 32, 8): (4, 64, 1, 1, "two-kernel"),         # ca_gate_mlp_bwd_kernel + ca_apply_bwd_kernel
    (40, 9, 32, 8): (4, 64, 1, 1, "two-kernel"),         # rows mode beyond the cap
}
CA_CASES_32 = {
    (2, 63, 4, 1): (1, 256, 1, 1, "fused"),
    (2, 130, 100, 25): (25, 10, 9, 7, "fused"),          # CV = 25: rpp = 10, 6 idle threads; 9 slices (odd tail)
    (1, 1100, 128, 32): (32, 8, 64, 69, "fused"),        # rpp = 8; 64-slice cap with 3 rows per thread
    (33, 9, 128, 32): (32, 8, 1, 1, "two-kernel"),        # two rows per thread
}
CA_ROWS = {(2, 130, 32, 32), (40, 9, 32, 8), (2, 130, 100, 25)}


def ca_cases(dtype):
    return CA_CASES_32 if dtype == F32 else CA_CASES_16


def _first_layer(R, C, g_):
    """[R, C] first-layer weights: rows alternate in sign on top of noise, so that with positive channel means every sample has dead
    and live hidden units (R = 1: live), while about one weight in eight has the other sign (both signs within a row)"""
    sign = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(R)])[:, None]
    return ((torch.randn(R, C, generator=g_) * 0.3 + 0.35 * sign) / math.sqrt(C)).contiguous()


def _second_layer(C, R, g_):
    """[C, R] second-layer weights, mostly positive: the gradients dz (of one sign here, g and res have positive means) then add up
    in dh = W2^T dz instead of cancelling, and a bound on absolute values stays near the value it bounds"""
    return ((torch.randn(C, R, generator=g_) * 0.3 + 0.35) / math.sqrt(R)).contiguous()


def ca_inputs(B, HW, C, R, dtype, seed=0, saturate=False):
    """res, x, g in T; w1 [R, C], w2 [C, R] fp32.  The gates stay in about (0.1, 0.9), so that no output is a difference of much
    larger terms; saturate: w2 rescaled so that the gate pre-activations span exactly +-100."""
    g_ = torch.Generator(device="cpu").manual_seed(200 + seed + 7 * C + HW)
    res = torch.randn(B, HW, C, generator=g_) + 1.0
    x = torch.randn(B, HW, C, generator=g_)
    g = torch.randn(B, HW, C, generator=g_) + 0.25
    w1 = _first_layer(R, C, g_)
    w2 = _second_layer(C, R, g_)
    res = res.to(dtype)
    if saturate:
        w2 = w2 * torch.tensor([1.0 if c % 2 == 0 else -1.0 for c in range(C)])[:, None]
        a = relu((res.to(F64).mean(1)) @ w1.to(F64).T) @ w2.to(F64).T
        w2 = (w2 * (100.0 / float(a.abs().max()))).contiguous()
    return res, x.to(dtype), g.to(dtype), w1, w2


def _mlp_hidden(pooled, W, HW, C):
    """relu(W (pooled / HW)) from the stored pooled sums: one division (DIV) and a sequential dot of length C (gamma(C) admits the
    fused and the two-rounding form).  The pre-activation bracket goes through the ReLU: [relu(lo), relu(hi)]."""
    m = pooled / HW
    a, S = m @ W.T, m.abs() @ W.abs().T
    ea = _finite((DIV + gamma(C)) * S, a)
    lo, hi = relu(a - ea), relu(a + ea)
    return torch.where(torch.isfinite(a), (lo + hi) / 2, relu(a)), _finite((hi - lo) / 2, a)


def _mlp_gate(hidden, W, R):
    """sigmoid(W hidden) from the stored hidden units: a dot of length R, then the sigmoid"""
    a, S = hidden @ W.T, hidden.abs() @ W.abs().T
    return sigmoid_terms(a, _finite(gamma(R) * S, a))


def ca_fwd_terms(res, x, w1, w2, dtype, st):
    """name -> (ref, err, stored type) of pooled, hidden, gate, out; st: the stored pooled [B, C], hidden [B, R], gate [B, C]"""
    B, HW, C = res.shape
    R = w1.shape[0]
    geo = pool_geometry(HW, C, dtype)
    r64, x64, W1, W2 = res.to(F64), x.to(F64), w1.to(F64), w2.to(F64)
    T = {"pooled": (r64.sum(1), gamma(geo.chain) * r64.abs().sum(1), F32)}
    T["hidden"] = _mlp_hidden(st.pooled.to(F64), W1, HW, C) + (F32,)
    T["gate"] = _mlp_gate(st.hidden.to(F64), W2, R) + (F32,)
    p = r64 * st.gate.to(F64)[:, None, :]
    out = p + x64
    T["out"] = (out, _finite(U32 * (p.abs() * (1 + U32) + out.abs()), out), dtype)       # fma, or the product rounded first
    return T


def ca_bwd_terms(g, res, w1, w2, dtype, st, rows=False):
    """name -> (ref, err, stored type) of dres and dw1 [R, C], dw2 [C, R] (rows: dw_rows [B, 2 R C]) from the stored pooled, hidden and
    gate, through dz -> dh -> dmean on absolute values"""
    B, HW, C = res.shape
    R = w1.shape[0]
    geo = pool_geometry(HW, C, dtype)
    g64, r64, W1, W2 = g.to(F64), res.to(F64), w1.to(F64), w2.to(F64)
    gt, hid, mean = st.gate.to(F64), st.hidden.to(F64), st.pooled.to(F64) / HW
    gr = g64 * r64
    dgs, e_dgs = gr.sum(1), gamma(geo.chain + (1 if dtype == F32 else 0)) * gr.abs().sum(1)
    sg = gt * (1 - gt)
    dz = dgs * sg
    e_dz = e_dgs * sg.abs() + 3 * U32 * dz.abs() + FLUSH32            # a product of a saturated gate may underflow
    mask = hid > 0
    s, e_s = dz @ W2, e_dz @ W2.abs() + gamma(C) * (dz.abs() @ W2.abs())
    zero = torch.zeros_like(s)
    dh, e_dh = torch.where(mask, s, zero), torch.where(mask, e_s, zero)
    t, e_t = dh @ W1, e_dh @ W1.abs() + gamma(R) * (dh.abs() @ W1.abs())
    dm = t / HW
    e_dm = e_t / HW + DIV * dm.abs()
    p = g64 * gt[:, None, :]
    dres = p + dm[:, None, :]
    T = {"dres": (dres, e_dm[:, None, :] + U32 * (p.abs() * (1 + U32) + dres.abs()), dtype)}
    if rows:
        r1, r2 = dh[:, :, None] * mean[:, None, :], dz[:, :, None] * hid[:, None, :]                # [B, R, C], [B, C, R]
        e1 = e_dh[:, :, None] * mean.abs()[:, None, :] + (DIV + U32) * r1.abs()
        e2 = e_dz[:, :, None] * hid.abs()[:, None, :] + U32 * r2.abs()
        T["rows"] = (torch.cat([r1.reshape(B, -1), r2.reshape(B, -1)], 1), torch.cat([e1.reshape(B, -1), e2.reshape(B, -1)], 1), F32)
    else:       # the batch walk: B additions of products that are fused or rounded first (two-kernel path: rounded into dwp)
        T["dw1"] = (dh.T @ mean, e_dh.T @ mean.abs() + (DIV + gamma(B + 1)) * (dh.abs().T @ mean.abs()), F32)
        T["dw2"] = (dz.T @ hid, e_dz.T @ hid.abs() + gamma(B + 1) * (dz.abs().T @ hid.abs()), F32)
    return T


CA_MUTATIONS = ("tail_slice", "wrong_count", "gate16", "dmean_no_hw", "dw_missing_sample", "fmax_relu")


def ca_applicable(mut, case, dtype, nan_input=False):
    B, HW, C, R = case
    geo = pool_geometry(HW, C, dtype)
    return {"tail_slice": geo.gx % 2 == 1 and (geo.gx - 1) * geo.rpp < HW, "gate16": dtype in HALVES, "dmean_no_hw": HW > 1,
            "fmax_relu": nan_input}.get(mut, True)


def ca_emulate(res, x, g, w1, w2, dtype, mutate=None, rows=False):
    """fp64 emulation of the documented arithmetic: every stored value rounded to fp32 (out, dres to T through fp32), everything
    else exact.  Returns the stored stats and every output.
      tail_slice         the tail slice of an odd slice count is skipped (pooled and sum g res)
      wrong_count        the mean is pooled / (HW + 1)
      gate16             the gate is rounded to T before the apply pass
      dmean_no_hw        dmean without its 1 / HW
      dw_missing_sample  the batch sum of dw1 / dw2 stops before the last sample (rows mode: the last row is left out = zero)
      fmax_relu          fmaxf-style hidden ReLU: a NaN pre-activation becomes 0"""
    assert mutate is None or mutate in CA_MUTATIONS, mutate
    B, HW, C = res.shape
    geo = pool_geometry(HW, C, dtype)
    r64, x64, g64, W1, W2 = res.to(F64), x.to(F64), g.to(F64), w1.to(F64), w2.to(F64)
    cnt = HW + 1 if mutate == "wrong_count" else HW
    pooled = _pooled_emulated(r64, geo, mutate == "tail_slice")
    a = (pooled / cnt) @ W1.T
    hidden = fl32(torch.clamp(torch.nan_to_num(a, nan=0.0, posinf=float("inf"), neginf=float("-inf")), min=0) if mutate == "fmax_relu"
                  else relu(a))
    gate = fl32(torch.sigmoid(hidden @ W2.T))
    ga = rt(gate, dtype) if mutate == "gate16" else gate
    out = store(r64 * ga[:, None, :] + x64, dtype)
    # backward, from the stored stats
    mean = pooled / cnt
    dz = _pooled_emulated(g64 * r64, geo, mutate == "tail_slice") * gate * (1 - gate)
    s = dz @ W2
    dh = torch.where(hidden > 0, s, torch.zeros_like(s))
    dm = dh @ W1 if mutate == "dmean_no_hw" else (dh @ W1) / HW
    dres = store(g64 * gate[:, None, :] + dm[:, None, :], dtype)
    E = SimpleNamespace(pooled=pooled, hidden=hidden, gate=gate, out=out, dres=dres)
    if rows:
        E.rows = fl32(torch.cat([(dh[:, :, None] * mean[:, None, :]).reshape(B, -1), (dz[:, :, None] * hidden[:, None, :]).reshape(B, -1)], 1))
        if mutate == "dw_missing_sample":
            E.rows[B - 1] = 0.0
    else:
        n = B - 1 if mutate == "dw_missing_sample" else B
        E.dw1, E.dw2 = fl32(dh[:n].T @ mean[:n]), fl32(dz[:n].T @ hidden[:n])
    return E


# ============================================================================================== SAM
def sam_supported(B, HW, C, R, dtype):
    """mirror of sam_ok (sam.hip)"""
    V = vec(dtype)
    return (0 < B <= 65535 and HW > 0 and V <= C <= 128 and C % V == 0 and 256 % (C // V) == 0 and 0 < R <= 32
            and 3 * R * C + R <= 1024)


def sam_stats_floats(B, C, R):
    return 4 * B * C + 4 * B * R + 2 * B + 2 * 64 * B * C


def sam_scratch_floats(B, C):
    return 2 * 64 * B * C


def sam_plan(B, HW, C, R, dtype):
    geo = pool_geometry(HW, C, dtype)
    return geo.CV, geo.rpp, geo.gx, apply_grid(HW, C, dtype)


SAM_CASES_16 = {
    (2, 256, 32, 2): (4, 64, 4, 2),                      # the model's shape
    (1, 63, 32, 2): (4, 64, 1, 1),
    (3, 240, 64, 4): (8, 32, 8, 4),
    (2, 81, 128, 2): (16, 16, 6, 3),
    (5, 130, 32, 2): (4, 64, 3, 2),                      # the batch walk (sample 0 last); 3 slices: odd tail
}
SAM_CASES_32 = {
    (2, 63, 4, 2): (1, 256, 1, 1),
    (5, 130, 32, 2): (8, 32, 3, 3),                      # the slice count follows C, not CV: cdiv(130, 64) = 3
}


def sam_cases(dtype):
    return SAM_CASES_32 if dtype == F32 else SAM_CASES_16


def sam_inputs(B, HW, C, R, dtype, seed=0):
    g_ = torch.Generator(device="cpu").manual_seed(300 + seed + 7 * C + HW)
    xh = torch.randn(B, HW, C, generator=g_) + 1.0
    xl = torch.randn(B, HW, C, generator=g_) - 0.75
    g = torch.randn(B, HW, C, generator=g_) + 0.25
    w1, v1 = _first_layer(R, C, g_), _first_layer(R, C, g_)
    w2, v2 = _second_layer(C, R, g_), _second_layer(1, R, g_)[0].contiguous()
    return xh.to(dtype), xl.to(dtype), g.to(dtype), w1, w2, v1, v2


def sam_unpack(stats, B, C, R):
    """views of the stats buffer (sam.hip `what the backward keeps`): pooled [2,B,C], gc [2,B,C], hc [2,B,R], hw [2,B,R], gw [2,B]"""
    o, S = 0, SimpleNamespace()
    for name, shape in (("pooled", (2, B, C)), ("gc", (2, B, C)), ("hc", (2, B, R)), ("hw", (2, B, R)), ("gw", (2, B))):
        n = math.prod(shape)
        setattr(S, name, stats[o:o + n].view(shape))
        o += n
    return S


def sam_fwd_terms(xh, xl, w1, w2, v1, v2, dtype, st):
    B, HW, C = xh.shape
    R = w1.shape[0]
    geo = pool_geometry(HW, C, dtype)
    X = torch.stack([xh.to(F64), xl.to(F64)])                                                 # [2, B, HW, C]
    W1, W2, V1, V2 = w1.to(F64), w2.to(F64), v1.to(F64), v2.to(F64)
    T = {"pooled": (X.sum(2), gamma(geo.chain) * X.abs().sum(2), F32)}
    pooled = st.pooled.to(F64)
    T["hc"] = _mlp_hidden(pooled, W1, HW, C) + (F32,)
    T["hw"] = _mlp_hidden(pooled, V1, HW, C) + (F32,)
    T["gc"] = _mlp_gate(st.hc.to(F64), W2, R) + (F32,)
    gw, e_gw = _mlp_gate(st.hw.to(F64), V2[None, :], R)
    T["gw"] = (gw[..., 0], e_gw[..., 0], F32)
    G = fl32(st.gc.to(F64) * st.gw.to(F64)[..., None])                                        # G = gc * gw, one fp32 rounding (exact here)
    p = X * G[:, :, None, :]
    out = p[0] + p[1]
    T["out"] = (out, _finite(U32 * ((p[0].abs() + p[1].abs()) * (1 + U32) + out.abs()), out), dtype)
    return T


def sam_bwd_terms(g, xh, xl, w1, w2, v1, v2, dtype, st):
    """dxh, dxl and dw = { dW1 [R,C] | dW2 [C,R] | dV1 [R,C] | dV2 [R] } from the stored stats"""
    B, HW, C = xh.shape
    R = w1.shape[0]
    geo = pool_geometry(HW, C, dtype)
    g64 = g.to(F64)
    X = torch.stack([xh.to(F64), xl.to(F64)])
    W1, W2, V1, V2 = w1.to(F64), w2.to(F64), v1.to(F64), v2.to(F64)
    gc, gw, hc, hw, m = st.gc.to(F64), st.gw.to(F64)[..., None], st.hc.to(F64), st.hw.to(F64), st.pooled.to(F64) / HW
    gx_ = g64[None] * X
    dG, e_dG = gx_.sum(2), gamma(geo.chain + (1 if dtype == F32 else 0)) * gx_.abs().sum(2)   # [2, B, C]
    f = gw * gc * (1 - gc)
    dzc = dG * f
    e_dzc = e_dG * f.abs() + 4 * U32 * dzc.abs() + FLUSH32
    tw = dG * gc
    e_tw = e_dG * gc.abs() + U32 * tw.abs()
    sw = gw * (1 - gw)
    dzw = tw.sum(-1, keepdim=True) * sw                                                       # [2, B, 1]
    e_dzw = (e_tw.sum(-1, keepdim=True) + gamma(C) * tw.abs().sum(-1, keepdim=True)) * sw.abs() + 3 * U32 * dzw.abs()
    s, e_s = dzc @ W2, e_dzc @ W2.abs() + gamma(C) * (dzc.abs() @ W2.abs())                   # [2, B, R]
    zero = torch.zeros_like(s)
    dhc, e_dhc = torch.where(hc > 0, s, zero), torch.where(hc > 0, e_s, zero)
    sv = V2 * dzw
    dhw, e_dhw = torch.where(hw > 0, sv, zero), torch.where(hw > 0, V2.abs() * e_dzw + U32 * sv.abs(), zero)
    t = dhc @ W1 + dhw @ V1
    e_t = e_dhc @ W1.abs() + e_dhw @ V1.abs() + gamma(2 * R) * (dhc.abs() @ W1.abs() + dhw.abs() @ V1.abs())
    dm = t / HW
    e_dm = e_t / HW + DIV * dm.abs()
    G = fl32(gc * gw)
    p = g64[None] * G[:, :, None, :]
    dx = p + dm[:, :, None, :]
    e_dx = e_dm[:, :, None, :] + U32 * (p.abs() * (1 + U32) + dx.abs())
    # weight gradients: per sample the two inputs' products and their add, then one add into the running sum (sample B-1 .. 0)
    cw = gamma(B + 2)
    bt = lambda a, b: torch.einsum("zbi,zbj->ij", a, b)
    parts = [(bt(dhc, m), bt(e_dhc, m.abs()) + (DIV + cw) * bt(dhc.abs(), m.abs())),
             (bt(dzc, hc), bt(e_dzc, hc.abs()) + cw * bt(dzc.abs(), hc.abs())),
             (bt(dhw, m), bt(e_dhw, m.abs()) + (DIV + cw) * bt(dhw.abs(), m.abs())),
             (bt(dzw, hw), bt(e_dzw, hw.abs()) + cw * bt(dzw.abs(), hw.abs()))]
    dw = torch.cat([p_[0].reshape(-1) for p_ in parts])
    e_dw = torch.cat([p_[1].reshape(-1) for p_ in parts])
    return {"dxh": (dx[0], e_dx[0], dtype), "dxl": (dx[1], e_dx[1], dtype), "dw": (dw, e_dw, F32)}


SAM_MUTATIONS = ("tail_slice", "wrong_count", "gate16", "dmean_no_hw", "dw_missing_sample", "wrong_mask", "fmax_relu")


def sam_applicable(mut, case, dtype, nan_input=False):
    B, HW, C, R = case
    return {"tail_slice": pool_geometry(HW, C, dtype).gx % 2 == 1, "gate16": dtype in HALVES, "dmean_no_hw": HW > 1,
            "fmax_relu": nan_input}.get(mut, True)


def sam_emulate(xh, xl, g, w1, w2, v1, v2, dtype, mutate=None):
    """as ca_emulate; wrong_mask: the ReLU masks of x_h's gradients are taken from x_l's hidden units and the other way round;
    dw_missing_sample: sample 0, which is summed last, is left out"""
    assert mutate is None or mutate in SAM_MUTATIONS, mutate
    B, HW, C = xh.shape
    geo = pool_geometry(HW, C, dtype)
    g64 = g.to(F64)
    X = torch.stack([xh.to(F64), xl.to(F64)])
    W1, W2, V1, V2 = w1.to(F64), w2.to(F64), v1.to(F64), v2.to(F64)
    cnt = HW + 1 if mutate == "wrong_count" else HW
    pooled = _pooled_emulated(X, geo, mutate == "tail_slice")
    m = pooled / cnt
    act = (lambda a: torch.clamp(torch.nan_to_num(a, nan=0.0, posinf=float("inf"), neginf=float("-inf")), min=0)) \
        if mutate == "fmax_relu" else relu
    hc, hw = fl32(act(m @ W1.T)), fl32(act(m @ V1.T))
    gc, gw = fl32(torch.sigmoid(hc @ W2.T)), fl32(torch.sigmoid(hw @ V2))                     # [2,B,C], [2,B]
    G = fl32(gc * gw[..., None])
    Ga = rt(G, dtype) if mutate == "gate16" else G
    out = store((X * Ga[:, :, None, :]).sum(0), dtype)
    dG = _pooled_emulated(g64[None] * X, geo, mutate == "tail_slice")
    gw1 = gw[..., None]
    dzc = dG * gw1 * gc * (1 - gc)
    dzw = (dG * gc).sum(-1, keepdim=True) * gw1 * (1 - gw1)
    mc, mw = (hc.flip(0), hw.flip(0)) if mutate == "wrong_mask" else (hc, hw)
    s = dzc @ W2
    zero = torch.zeros_like(s)
    dhc, dhw = torch.where(mc > 0, s, zero), torch.where(mw > 0, V2 * dzw, zero)
    dm = dhc @ W1 + dhw @ V1
    if mutate != "dmean_no_hw":
        dm = dm / HW
    dx = store(g64[None] * G[:, :, None, :] + dm[:, :, None, :], dtype)
    k = slice(1, None) if mutate == "dw_missing_sample" else slice(None)
    bt = lambda a, b: torch.einsum("zbi,zbj->ij", a[:, k], b[:, k]).reshape(-1)
    dw = fl32(torch.cat([bt(dhc, m), bt(dzc, hc), bt(dhw, m), bt(dzw, hw)]))
    return SimpleNamespace(pooled=pooled, hc=hc, hw=hw, gc=gc, gw=gw, out=out, dxh=dx[0], dxl=dx[1], dw=dw)


# ============================================================================================== bilinear
def bil_scale(n_in, n_out, align):
    """make_axis: one IEEE fp32 division on the host"""
    if align:
        return (torch.tensor(float(n_in - 1), dtype=F32) / torch.tensor(float(n_out - 1), dtype=F32)) if n_out > 1 else torch.tensor(0.0)
    return torch.tensor(float(n_in), dtype=F32) / torch.tensor(float(n_out), dtype=F32)


def bil_lpi(Hi, Ho, align):
    """lanes per item of dgtd_bilinear_bwd: by the vertical up-sampling factor 1 / scale (fp32)"""
    sc = bil_scale(Hi, Ho, align)
    up = float(torch.tensor(1.0, dtype=F32) / sc) if float(sc) > 0 else float(Ho)
    return 16 if up >= 6.0 else (8 if up >= 3.0 else (2 if up >= 1.5 else 1))


def bil_plan(B, Hi, Wi, Ho, Wo, C, align, dtype):
    """(forward grid, forward trips, LPI, backward grid, backward trips)"""
    CV = C // vec(dtype)
    nf, nb, lpi = B * Ho * Wo * CV, B * Hi * Wi * CV, bil_lpi(Hi, Ho, align)
    gf, gb = min(cdiv(nf, 256), 2048), min(cdiv(nb * lpi, 256), 2048)
    return gf, cdiv(nf, gf * 256), lpi, gb, cdiv(cdiv(nb, 256 // lpi), gb)


def _axis64(n_in, n_out, align, shift=0.0, dev="cpu"):
    """fp64 source index (from the fp32 scale), its uncertainty delta_s in the kernel's fp32, and the taps of index s + shift"""
    sc = float(bil_scale(n_in, n_out, align))
    o = torch.arange(n_out, dtype=F64, device=dev)
    if align:
        s = sc * o
        ds = U32 * s.abs()                                   # one rounding of scale * o
    else:
        s = sc * (o + 0.5) - 0.5
        ds = U32 * (2 * s.abs() + 0.5)                        # the product, then the subtraction (one rounding if fused)
        s = s.clamp(min=0.0)
    return s, ds


def _taps_matrix(s, n_in):
    """dense [n_out, n_in] weights of index s: i0 = min(floor(s), n_in - 1), i1 = min(i0 + 1, n_in - 1), l = s - i0"""
    i0 = s.floor().clamp(max=n_in - 1).long()
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l = s - i0.to(F64)
    W = torch.zeros(s.numel(), n_in, dtype=F64, device=s.device)
    W.scatter_add_(1, i0[:, None], (1 - l)[:, None])
    W.scatter_add_(1, i1[:, None], l[:, None])
    return W


def _slope_matrix(s, n_in):
    """d W / d s in the cell of index s: -1 at floor(s), +1 at floor(s) + 1; zero outside [0, n_in - 1) (both clamps are flat)"""
    k = s.floor().long()
    inside = ((k >= 0) & (k < n_in - 1)).to(F64)
    kc = k.clamp(0, max(n_in - 2, 0))
    D = torch.zeros(s.numel(), n_in, dtype=F64, device=s.device)
    if n_in > 1:
        D.scatter_add_(1, kc[:, None], -inside[:, None])
        D.scatter_add_(1, kc[:, None] + 1, inside[:, None])
    return D


def bil_axis(n_in, n_out, align, dev="cpu"):
    """W [n_out, n_in] fp64 weights; E >= |delta W|: delta_s times the larger of the slopes of the cells within delta_s of the index;
    T0 / T1: taps certainly read with a non-zero weight / possibly read (for where a NaN goes)"""
    s, ds = _axis64(n_in, n_out, align, dev=dev)
    W = _taps_matrix(s, n_in)
    Dl, Dh = _slope_matrix(s - ds, n_in), _slope_matrix(s + ds, n_in)
    E = ds[:, None] * torch.maximum(Dl.abs(), Dh.abs())
    sure = W > 2 * E + 1e-300
    # possibly touched: a tap of either neighbouring index, also at weight zero (the forward reads i1 at l = 0, as F.interpolate does)
    may = torch.zeros_like(sure)
    for sh in (s - ds, s, s + ds):
        sh = sh.clamp(min=0.0)
        i0 = sh.floor().clamp(max=n_in - 1).long()
        may.scatter_(1, i0[:, None], True)
        may.scatter_(1, (i0 + 1).clamp(max=n_in - 1)[:, None], True)
    return SimpleNamespace(W=W, E=E, sure=sure, may=may | sure, s=s, ds=ds)


def bil_fwd_terms(x, Ho, Wo, align, dtype):
    """y = Wh x Ww^T per channel.  Index term: the interpolant is continuous and piecewise linear in each index, so the kernel's fp32
    index moves it by at most delta_s times the LOCAL slope (E holds delta_s on the +-1 pattern of the cell); arithmetic term:
    BIL_FWD_TAP roundings on sum |w v|."""
    B, Hi, Wi, C = x.shape
    ah, aw = bil_axis(Hi, Ho, align, x.device), bil_axis(Wi, Wo, align, x.device)
    x64 = x.to(F64)
    ein = lambda A, v, Bm: torch.einsum("oh,bhwc,pw->bopc", A, v, Bm)
    ref = ein(ah.W, x64, aw.W)
    sl_h = torch.maximum(ein(_slope_matrix(ah.s - ah.ds, Hi), x64, aw.W).abs(), ein(_slope_matrix(ah.s + ah.ds, Hi), x64, aw.W).abs())
    sl_w = torch.maximum(ein(ah.W, x64, _slope_matrix(aw.s - aw.ds, Wi)).abs(), ein(ah.W, x64, _slope_matrix(aw.s + aw.ds, Wi)).abs())
    err = ah.ds[None, :, None, None] * sl_h + aw.ds[None, None, :, None] * sl_w + gamma(BIL_FWD_TAP) * ein(ah.W, x64.abs(), aw.W)
    return ref, _finite(err, ref)


def bil_bwd_chain(Hi, Wi, Ho, Wo, align, dev="cpu"):
    """[Hi, Wi] longest chain of additions into one input pixel: the non-zero taps one lane sums (the rows that touch an input row are
    consecutive, so a lane of LPI takes at most ceil(rows / LPI) of them) plus log2(LPI) shuffle steps"""
    lpi = bil_lpi(Hi, Ho, align)
    nh = (bil_axis(Hi, Ho, align, dev).may).sum(0)
    nw = (bil_axis(Wi, Wo, align, dev).may).sum(0)
    return (-(-nh // lpi))[:, None] * nw[None, :] + int(math.log2(lpi))


def bil_bwd_terms(dy, Hi, Wi, align, dtype):
    """dx = Wh^T dy Ww; index term on sum |delta w| |dy| (first order), arithmetic term (BIL_BWD_TAP + chain) U32 sum |w| |dy|"""
    B, Ho, Wo, C = dy.shape
    ah, aw = bil_axis(Hi, Ho, align, dy.device), bil_axis(Wi, Wo, align, dy.device)
    g64 = dy.to(F64)
    ein = lambda A, v, Bm: torch.einsum("oh,bopc,pw->bhwc", A, v, Bm)
    ref, ga = ein(ah.W, g64, aw.W), g64.abs()
    chain = bil_bwd_chain(Hi, Wi, Ho, Wo, align, dy.device).to(F64)
    err = ein(ah.E, ga, aw.W) + ein(ah.W, ga, aw.E) + ein(ah.E, ga, aw.E) \
        + gamma(1) * (BIL_BWD_TAP + chain)[None, :, :, None] * ein(ah.W, ga, aw.W)
    return ref, _finite(err, ref)


# (Hi, Wi, Ho, Wo) -> (LPI align_corners, LPI otherwise), by hand from dgtd_bilinear_bwd: up = 1 / scale of the H axis
BIL_CASES = {
    (2, 2, 16, 16): (16, 16),          # 1/15 -> 15; 2/16 -> 8
    (2, 2, 12, 12): (16, 16),          # 1/11 -> 11; fl32(1/6) -> exactly 6.0: the threshold
    (2, 2, 6, 6): (8, 8),              # 1/5 -> 5; fl32(1/3) -> exactly 3.0
    (2, 2, 3, 3): (2, 2),              # 1/2 -> 2; fl32(2/3) -> exactly 1.5
    (4, 4, 16, 16): (8, 8),            # 3/15 -> 5; 4/16 -> 4
    (8, 8, 16, 16): (2, 2),            # 7/15 -> 2.14; 0.5 -> 2
    (16, 16, 16, 16): (1, 1),          # identity
    (32, 32, 16, 16): (1, 1),
    (7, 9, 19, 13): (8, 2),            # 6/18 -> 3.0; 7/19 -> 2.71
    (3, 5, 40, 33): (16, 16),          # 2/39 -> 19.5; 3/40 -> 13.3: fewer candidate rows than lanes for some pixels
    (1, 5, 16, 7): (16, 16),           # Hi = 1: scale 0 -> up = Ho; 1/16 -> 16
    (5, 1, 7, 16): (2, 1),             # 4/6 -> 1.5; 5/7 -> 1.4
    (16, 16, 1, 1): (1, 1),            # n_out = 1: scale 0 / scale 16
    (4, 16, 32, 8): (16, 16),          # H up x8 (3/31 -> 10.3; 0.125 -> 8), W down x0.5
}
# grid-stride cases (B, Hi, Wi, Ho, Wo, C): forward with B Ho Wo CV just above 524288; backward at LPI 1 and LPI 2
BIL_BIG = {
    "fwd": (2, 16, 16, 512, 513, 8),
    "bwd-lpi1": (1, 264, 264, 132, 132, 64),
    "bwd-lpi2": (1, 184, 184, 368, 368, 64),
}


def bil_inputs(B, H, W, C, dtype, seed=0):
    g_ = torch.Generator(device="cpu").manual_seed(400 + seed + 13 * H + W)
    return (torch.randn(B, H, W, C, generator=g_) + 0.5).to(dtype)


BIL_MUTATIONS = ("drop_last_row", "drop_last_col", "no_neg_clamp", "swap_align", "lambda16", "drop_shuffle")


def _axis_emulated(n_in, n_out, align, dtype, mutate):
    """the kernel's fp32 taps() for every output index (product rounded, then the subtraction): dense fp32-exact weights in fp64"""
    sc = bil_scale(n_in, n_out, align)
    o = torch.arange(n_out, dtype=F32)
    if align:
        s = sc * o
    else:
        s = sc * (o + 0.5) - 0.5
        if mutate != "no_neg_clamp":
            s = torch.where(s < 0, torch.zeros_like(s), s)
    i0 = s.to(torch.int64).clamp(max=n_in - 1)              # (int)s truncates toward zero
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l = s - i0.to(F32)
    if mutate == "lambda16":
        l = l.to(dtype).to(F32)
    W = torch.zeros(n_out, n_in, dtype=F64)
    W.scatter_add_(1, i0[:, None], (1 - l).to(F64)[:, None])
    W.scatter_add_(1, i1[:, None], l.to(F64)[:, None])
    return W


def _candidates(n_in, n_out, align):
    """[n_out, n_in] mask, lo [n_in]: the backward's candidate range of every input index, restated in fp32"""
    sc = bil_scale(n_in, n_out, align)
    inv = (torch.tensor(1.0, dtype=F32) / sc) if float(sc) > 0 else torch.tensor(float(n_out), dtype=F32)
    i = torch.arange(n_in, dtype=F32)
    lo = (torch.floor((i - 1.0) * inv).to(torch.int64) - 2).clamp(min=0)
    hi = (torch.ceil((i + 1.5) * inv).to(torch.int64) + 1).clamp(max=n_out - 1)
    o = torch.arange(n_out)[:, None]
    return (o >= lo[None, :]) & (o <= hi[None, :]), lo, hi


def bil_emulate_fwd(x, Ho, Wo, align, dtype, mutate=None):
    assert mutate in (None, "no_neg_clamp", "swap_align", "lambda16"), mutate
    B, Hi, Wi, C = x.shape
    al = (not align) if mutate == "swap_align" else align
    Wh, Ww = _axis_emulated(Hi, Ho, al, dtype, mutate), _axis_emulated(Wi, Wo, al, dtype, mutate)
    return store(torch.einsum("oh,bhwc,pw->bopc", Wh, x.to(F64), Ww), dtype)


def bil_emulate_bwd(dy, Hi, Wi, align, dtype, mutate=None):
    """drop_last_row / _col: the candidate window ends one early; drop_shuffle: the partials that arrive through the first xor step
    (lanes sub >= LPI / 2) are lost"""
    assert mutate is None or mutate in BIL_MUTATIONS, mutate
    B, Ho, Wo, C = dy.shape
    al = (not align) if mutate == "swap_align" else align
    Wh, Ww = _axis_emulated(Hi, Ho, al, dtype, mutate), _axis_emulated(Wi, Wo, al, dtype, mutate)
    mh, lo, hi = _candidates(Hi, Ho, align)
    mw, _, hiw = _candidates(Wi, Wo, align)
    o = torch.arange(Ho)[:, None]
    if mutate == "drop_last_row":
        mh = mh & (o < hi[None, :])
    if mutate == "drop_last_col":
        mw = mw & (torch.arange(Wo)[:, None] < hiw[None, :])
    if mutate == "drop_shuffle":
        lpi = bil_lpi(Hi, Ho, align)
        mh = mh & (((o - lo[None, :]) % lpi) < max(lpi // 2, 1))
    return store(torch.einsum("oh,bopc,pw->bhwc", Wh * mh, dy.to(F64), Ww * mw), dtype)


def bil_applicable(mut, case, align, dtype):
    """a mutation applies where it changes a weight the kernel uses: the emulated axis matrices differ, or a dropped candidate row /
    column / lane group carries a non-zero weight"""
    Hi, Wi, Ho, Wo = case
    if mut in ("no_neg_clamp", "swap_align", "lambda16"):
        if mut == "lambda16" and dtype not in HALVES:
            return False
        al = (not align) if mut == "swap_align" else align
        return any(not torch.equal(_axis_emulated(i, o, align, dtype, None), _axis_emulated(i, o, al, dtype, mut))
                   for i, o in ((Hi, Ho), (Wi, Wo)))
    n_in, n_out = (Wi, Wo) if mut == "drop_last_col" else (Hi, Ho)
    W = _axis_emulated(n_in, n_out, align, dtype, None)
    _, lo, hi = _candidates(n_in, n_out, align)
    o = torch.arange(n_out)[:, None]
    if mut == "drop_shuffle":
        lpi = bil_lpi(Hi, Ho, align)
        return lpi > 1 and bool((W * ((o >= lo[None, :]) & (((o - lo[None, :]) % lpi) >= lpi // 2))).any())
    return bool((W * (o == hi[None, :])).any())
