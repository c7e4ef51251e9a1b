"""GPU: the 16-bit GEMM (csrc/gemm.hip), the dense 3x3 convolution (csrc/conv3x3.hip) and every GELU site against fp64 references
at rounding-level bounds (tests/_numerics.py).

Every reference is computed in fp64 from the exact 16-bit operands the kernel reads; where a kernel rounds a stored intermediate on
purpose, the reference starts from the kernel's stored intermediate.  A kernel output must lie in [round(ref - err), round(ref + err)]
with err = c * sum|terms| (the same expression evaluated on absolute values), and at least 90 % of those brackets must be a single
value, so that one extra rounding anywhere fails.  Outputs are pre-filled with NaN (an element that is never written fails), all
operands are 16-byte aligned views at a non-zero offset inside a larger NaN-filled buffer (the guard regions must stay NaN), and a
second launch must reproduce the first bit for bit.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import _numerics as nm
from _kernel_check import C_MFMA, DEV, F64, MFMA_MAX_K, U32, Buf, _bits, _run_twice, _same_bits  # noqa: F401 (shared with the attention tests)

pytestmark = pytest.mark.gpu

HALVES = [torch.bfloat16, torch.float16]

# ---- error constants (each with its source; none is fitted to an observed error); U32, C_MFMA and MFMA_MAX_K live in _kernel_check
# |error| of Phi in gelu_phi (csrc/common.h): A&S 7.1.26 (1.5e-7 on erfc, 7.5e-8 on Phi) plus its fp32 evaluation
PHI_ABS = 5e-7

MARGINS = {}                # test family -> largest (|got - ref| - ulp/2) / err seen (reported at the end of the module)


@pytest.fixture(scope="module", autouse=True)
def lib():
    import dgtd
    L = dgtd._lib
    L.load()
    yield L
    if MARGINS:
        print("\nlargest share of the error bound used, per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(MARGINS.items())))


def _code(dt):
    import dgtd
    return dgtd._lib.dtype_code(torch.empty(1, dtype=dt))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    import dgtd
    dgtd._lib.call(name, *args)


def _check(got, ref, err, dtype, name, family, sharp_at=None, sharp_where=None):
    """bracket check + sharpness.  sharp_at: the dtype at which sharpness is demanded when it differs from the output's own (fp32
    sums with a chain bound are never single-valued at fp32 resolution; at 16-bit resolution they must be).  sharp_where: the
    elements on which it is demanded (GELU: where its absolute bound is below the output's rounding, see _check_gelu)."""
    lo, hi = nm.bracket(ref, err, dtype)
    nm.assert_bracketed(got, lo, hi, name, ref=ref, err=err)
    if sharp_at is not None:
        lo, hi = nm.bracket(ref, err, sharp_at)
        name += " (at 16-bit resolution)"
    if sharp_where is not None:
        lo, hi = lo[sharp_where], hi[sharp_where]
    nm.assert_sharp(lo, hi, name=name)
    MARGINS[family] = max(MARGINS.get(family, 0.0), nm.ratio(got, ref, err))


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, mean=0.0, std=1.0):
    return torch.randn(shape, generator=_gen(seed), device=DEV, dtype=torch.float32) * std + mean


# ---------------------------------------------------------------------------------------------- GELU references (fp64)
def _phi64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def _pdf64(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_ref(x64):
    """x Phi(x) and its bound: |x| PHI_ABS (common.h) + one fp32 rounding of the product"""
    ref = x64 * _phi64(x64)
    return ref, PHI_ABS * x64.abs() + U32 * ref.abs()


def gelu_grad_ref(x64):
    """Phi(x) + x phi(x) = fmaf(x, pdf, Phi) and its bound: PHI_ABS, plus for the Gaussian term the relative error of exp(-x^2/2) in
    fp32 (the argument -x^2/2 log2 e is formed with three roundings: (3/2) x^2 U32, v_exp_f32 and the pdf product: 2 U32 more) and the
    rounding of the fma.  Stated on |Phi| + |x phi| so that the cancellation around the root near x = -0.75 is allowed for."""
    xp = x64 * _pdf64(x64)
    ref = _phi64(x64) + xp
    err = PHI_ABS + (1.5 * x64 * x64 + 2.0) * U32 * xp.abs() + U32 * (_phi64(x64) + xp.abs())
    return ref, err


# ---------------------------------------------------------------------------------------------- GEMM (csrc/gemm.hip)
BM = 128


def gemm_variant(M, N, K):
    """(BN, NSTAGE) the default dispatch of gemm.hip launch() picks"""
    wide = N % 128 == 0 and (M // BM) * (N // 128) >= 192
    tiles = (M // BM) * (N // (128 if wide else 64))
    return (128 if wide else 64), (3 if wide and tiles <= 256 else 2)


def colsum_chain(BN):
    """longest chain of fp32 additions in the GELU_BWD column partials: NPASS per-thread adds + RPP adds of the per-row partials"""
    CPR = BN // 8
    RPP = 256 // CPR
    return BM // RPP + RPP


GEMM_CASES = [  # M, N, K, expected (BN, NSTAGE), what it exercises
    (128, 64, 64, (64, 2)),          # one tile, one k-step
    (1152, 192, 128, (64, 2)),       # 27 tiles: not a multiple of 8 (XCD remap)
    (2048, 320, 1280, (64, 2)),      # N % 128 != 0, 20 k-steps
    (8192, 512, 64, (128, 3)),       # 3-stage, nk = 1
    (8192, 512, 128, (128, 3)),      # 3-stage, nk = 2
    (3200, 1152, 192, (128, 3)),     # 225 tiles (not a multiple of 8), nk = 3
    (8192, 2048, 512, (128, 2)),     # the benchmarked shape
    (4224, 1152, 256, (128, 2)),     # 297 tiles
]


def _gemm_operands(M, N, K, dt, seed, scale_a=1.0, scale_b=1.0):
    """asymmetric operands: A with a positive mean, B rows with means of either sign (columns of D of both signs, little
    cancellation, so that the bound is sharp); bias small"""
    a = (_randn((M, K), seed, mean=0.5) * scale_a).to(dt)
    mu = (torch.rand((N, 1), generator=_gen(seed + 1), device=DEV) - 0.5)
    b = ((_randn((N, K), seed + 2) + mu) / math.sqrt(K) * scale_b).to(dt)
    bias = (0.1 * _randn((N,), seed + 3)).to(dt)
    return a, b, bias


def _fl32(t64):
    """the fp32 rounding of an exact fp64 value (an fp32 operation of the kernel whose operands are exact), back in fp64"""
    return nm.round_to(t64, torch.float32).to(F64)


def _mm64(a, b):
    """fp64 a @ b^T and |a| @ |b|^T"""
    a64, b64 = a.to(F64), b.to(F64)
    return a64 @ b64.t(), a64.abs() @ b64.abs().t()


def _gemm_all_entries(M, N, K, dt, a, b, bias, tag, rows_per_sample=None, family="gemm"):
    code, st = _code(dt), _st()
    A, Bm, Bias = Buf((M, K), dt, a), Buf((N, K), dt, b), Buf((N,), dt, bias)
    acc, S = _mm64(A.t, Bm.t)
    bias64 = Bias.t.to(F64)
    ref, err = acc + bias64, C_MFMA * (S + bias64.abs())

    # gemm_bias, with and without bias
    (d,) = _run_twice(lambda o: _call("dgtd_gemm_bias", A.p, Bm.p, Bias.p, o[0].p, M, N, K, code, st), [((M, N), dt)], f"{tag} gemm_bias")
    _check(d, ref, err, dt, f"{tag} gemm_bias", family)
    (d0,) = _run_twice(lambda o: _call("dgtd_gemm_bias", A.p, Bm.p, None, o[0].p, M, N, K, code, st), [((M, N), dt)], f"{tag} gemm_nobias")
    _check(d0, acc, C_MFMA * S, dt, f"{tag} gemm_bias(no bias)", family)

    # gemm_bias_gelu: pre = round(acc + bias); h = round(gelu(STORED pre))
    pre, h = _run_twice(lambda o: _call("dgtd_gemm_bias_gelu", A.p, Bm.p, Bias.p, o[0].p, o[1].p, M, N, K, code, st),
                        [((M, N), dt), ((M, N), dt)], f"{tag} gemm_gelu")
    _check(pre, ref, err, dt, f"{tag} gemm_gelu.pre", family)
    gr, ge = gelu_ref(pre.to(F64))
    _check(h, gr, ge, dt, f"{tag} gemm_gelu.h", "gelu-epilogue", sharp_where=pre.float() >= -3)
    (h2,) = _run_twice(lambda o: _call("dgtd_gemm_bias_gelu", A.p, Bm.p, Bias.p, None, o[0].p, M, N, K, code, st), [((M, N), dt)],
                       f"{tag} gemm_gelu(no pre)")
    _same_bits(h2, h, f"{tag} gemm_gelu without the stored pre-activation")

    # gemm_bias_residual with s / gamma and the stored y: out = round(fmaf(fl32(s gamma), STORED y, x))
    nsamp = M // rows_per_sample if rows_per_sample else 2
    rps = rows_per_sample or M // 2
    X = Buf((M, N), dt, _randn((M, N), 11).to(dt))
    s = Buf((nsamp,), torch.float32, torch.linspace(0.0, 1.5, nsamp, device=DEV))     # s = 0 for sample 0: DropPath drop
    gamma = Buf((N,), torch.float32, 0.5 + 0.1 * _randn((N,), 12))
    y, out = _run_twice(lambda o: _call("dgtd_gemm_bias_residual", A.p, Bm.p, Bias.p, X.p, s.p, gamma.p, o[0].p, o[1].p, M, N, K, rps, code, st),
                        [((M, N), dt), ((M, N), dt)], f"{tag} gemm_residual")
    _check(y, ref, err, dt, f"{tag} gemm_residual.y", family)
    sg = (s.t.repeat_interleave(rps)[:, None] * gamma.t[None, :]).to(F64)      # fp32 product, as the kernel forms it
    t1, x64 = sg * y.to(F64), X.t.to(F64)
    _check(out, t1 + x64, U32 * (t1.abs() + x64.abs()), dt, f"{tag} gemm_residual.out", "residual-epilogue")
    # without s / gamma / y: out = round(fl32(y + x)), y the same rounding the call above stored.  fmaf(1, y, x) is one IEEE fp32
    # rounding of the exact sum, which the reference reproduces (err 0); the sum of two 16-bit values often lies exactly on a midpoint
    # of the 16-bit grid, where only this double rounding decides
    (out1,) = _run_twice(lambda o: _call("dgtd_gemm_bias_residual", A.p, Bm.p, Bias.p, X.p, None, None, None, o[0].p, M, N, K, 1, code, st),
                         [((M, N), dt)], f"{tag} gemm_residual(plain)")
    y64 = y.to(F64)
    _check(out1, _fl32(y64 + x64), torch.zeros_like(y64), dt, f"{tag} gemm_residual(plain)", "residual-epilogue")

    # gemm_gelu_bwd: dpre = round(acc * gelu'(pre)) (+ column partials of the STORED dpre per 128-row tile)
    P = Buf((M, N), dt, (6.0 * torch.rand((M, N), generator=_gen(13), device=DEV) - 3.5).to(dt))
    ws_bytes = _lib_fn("dgtd_gemm_gelu_bwd_workspace")(M, N)
    nb = C.c_int(0)
    dp, cs = _run_twice(lambda o: _call("dgtd_gemm_gelu_bwd", A.p, Bm.p, P.p, o[0].p, o[1].p, C.byref(nb), M, N, K, code, st),
                        [((M, N), dt), ((ws_bytes // 4 // N, N), torch.float32)], f"{tag} gemm_gelu_bwd")
    assert nb.value == M // BM
    gg, gge = gelu_grad_ref(P.t.to(F64))
    rd = acc * gg
    _check(dp, rd, C_MFMA * S * gg.abs() + (acc.abs() + C_MFMA * S) * gge + U32 * rd.abs(), dt, f"{tag} gemm_gelu_bwd.dpre", "gelu-bwd-epilogue")
    dp64 = dp.to(F64).view(M // BM, BM, N)
    BN, _ = gemm_variant(M, N, K)
    _check(cs, dp64.sum(1), colsum_chain(BN) * U32 * dp64.abs().sum(1), torch.float32, f"{tag} gemm_gelu_bwd.colsum", "colsum",
           sharp_at=torch.bfloat16)
    for t in (A, Bm, Bias, X, s, gamma, P):
        t.guards_intact(f"{tag} inputs")


def _lib_fn(name):
    import dgtd
    return getattr(dgtd._lib.load(), name)


@pytest.mark.parametrize("M,N,K,variant", GEMM_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in GEMM_CASES])
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_gemm_entries_vs_fp64(M, N, K, variant, dt):
    """every entry of the GEMM (bias / no bias, GELU with and without the stored pre, residual with and without s, gamma and y,
    GELU backward with its column partials) at every tile width / pipeline depth the dispatch can reach"""
    assert gemm_variant(M, N, K) == variant
    a, b, bias = _gemm_operands(M, N, K, dt, seed=M + N + K)
    _gemm_all_entries(M, N, K, dt, a, b, bias, f"{dt} {M}x{N}x{K}")


@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_gemm_residual_tiles_straddle_samples(dt):
    """1920 rows = 6 samples of 320: every 128-row tile but one straddles two samples with different DropPath scales"""
    M, N, K = 1920, 256, 128
    a, b, bias = _gemm_operands(M, N, K, dt, seed=5)
    _gemm_all_entries(M, N, K, dt, a, b, bias, f"{dt} straddle", rows_per_sample=320)


def test_gemm_fp16_overflow_is_inf():
    """fp16 outputs beyond 65520 are +-inf (the correctly rounded value), never a saturated 65504"""
    dt, M, N, K = torch.float16, 256, 128, 64
    a, b, _ = _gemm_operands(M, N, K, dt, seed=21)
    s = math.sqrt(65520.0 / _mm64(a, b)[0].abs().median().item())
    a, b, bias = _gemm_operands(M, N, K, dt, seed=21, scale_a=s, scale_b=s)
    acc, _ = _mm64(a, b)
    big = (acc.abs() > 65520).float().mean().item()
    assert 0.05 < big < 0.95, big                       # both overflowing and finite outputs
    _gemm_all_entries(M, N, K, dt, a, b, bias, "fp16 overflow", family="gemm-fp16-range")


def test_gemm_fp16_subnormal_outputs_not_flushed():
    dt, M, N, K = torch.float16, 256, 128, 64
    a, b, bias = _gemm_operands(M, N, K, dt, seed=22, scale_a=2.0 ** -7, scale_b=2.0 ** -7)
    bias.zero_()
    acc, _ = _mm64(a, b)
    sub = ((acc.abs() < 6.1e-5) & (acc != 0)).float().mean().item()
    assert sub > 0.2, sub
    _gemm_all_entries(M, N, K, dt, a, b, bias, "fp16 subnormal", family="gemm-fp16-range")


@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_gemm_nan_row_propagates(dt):
    """a NaN in one row of A makes that output row NaN in every epilogue (and the column partial of its tile)"""
    M, N, K = 256, 128, 128
    a, b, bias = _gemm_operands(M, N, K, dt, seed=23)
    a[77, 5] = float("nan")
    _gemm_all_entries(M, N, K, dt, a, b, bias, f"{dt} nan-row")


# ---------------------------------------------------------------------------------------------- dense 3x3 convolution (csrc/conv3x3.hip)
def _cdiv(a, b):
    return -(-a // b)


def conv_fwd_instance(Z, B, H, W, Ci, Co):
    """(CI, NT, MT, TWX, nsplit) of the conv3x3_fwd_kernel the default dispatch (fwd_geom / dispatch_fwd_geom) launches"""
    twx = 32 if W >= 32 else 16
    rw = 32 // twx
    mt_cap = 4 if Ci <= 32 else (2 if Ci <= 64 else 1)
    mt, m = 1, mt_cap
    while m > 1:
        if Z * B * _cdiv(H, 4 * m * rw) * _cdiv(W, twx) >= 1024:
            mt = m
            break
        m >>= 1
    nt = _cdiv(Co, 32)
    if nt > 1 and Z * B * _cdiv(H, 4 * rw) * _cdiv(W, twx) < 512:
        return (Ci, 1, 1, twx, nt)
    if twx == 16:
        return (Ci, nt, 1, 16, 1)
    if Ci <= 32 and mt == 4:
        return (Ci, nt, 4, 32, 1)
    if Ci <= 64 and mt >= 2:
        return (Ci, nt, 2, 32, 1)
    return (Ci, nt, 1, 32, 1)


def conv_ref(x64, w64, b64=None):
    """y[b,h,w,co] = sum_{ky,kx,ci} xpad[b,h+ky,w+kx,ci] w[co,ky,kx,ci] (+ bias) as 9 shifted fp64 matmuls, and sum|terms|"""
    Bn, H, W, Ci = x64.shape
    xp = F.pad(x64, (0, 0, 1, 1, 1, 1))
    ref = torch.zeros(Bn, H, W, w64.shape[0], dtype=F64, device=DEV)
    S = torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky:ky + H, kx:kx + W, :]
            wk = w64[:, ky, kx, :]
            ref += xs @ wk.t()
            S += xs.abs() @ wk.abs().t()
    if b64 is not None:
        ref += b64
        S += b64.abs()
    return ref, S


def _conv_operands(Z, B, H, W, Ci, Co, dt, seed, shared=False):
    x = _randn((1 if shared else Z, B, H, W, Ci), seed, mean=0.5).to(dt)
    mu = torch.rand((Z, Co, 1, 1, 1), generator=_gen(seed + 1), device=DEV) - 0.5
    w = ((_randn((Z, Co, 3, 3, Ci), seed + 2) + mu) / math.sqrt(9 * Ci)).to(dt)
    b = (0.1 * _randn((Z, Co), seed + 3)).to(dt)
    return x, w, b


def _relu_keep_nan(t):
    return torch.where(t < 0, torch.zeros_like(t), t)


def _conv_case(dt, Z, B, H, W, Ci, Co, *, shared=False, act=0, bias=True, add=False, entry="ex", seed=1, x=None, w=None, tag="",
               family="conv-fwd"):
    """one dgtd_conv3x3_fwd(_ex) configuration against the fp64 reference; returns (y, reference pieces)"""
    code, st = _code(dt), _st()
    x0, w0, b0 = _conv_operands(Z, B, H, W, Ci, Co, dt, seed, shared)
    if x is not None:
        x0 = x
    if w is not None:
        w0 = w
    X, Wt, Bi = Buf(x0.shape, dt, x0), Buf(w0.shape, dt, w0), Buf(b0.shape, dt, b0)
    Add = Buf((Z, B, H, W, Co), dt, _randn((Z, B, H, W, Co), seed + 4).to(dt)) if add else None
    Ref = Buf((Z, B, H, W, Co), dt, _randn((Z, B, H, W, Co), seed + 5).to(dt)) if act == 3 else None
    slope = Buf((1,), torch.float32, torch.tensor([0.25], device=DEV)) if act >= 2 else None
    name = f"{tag}{dt} conv Z{Z} B{B} {H}x{W} {Ci}->{Co} act{act}{' bias' if bias else ''}{' add' if add else ''}{' shared' if shared else ''}"
    outs = [((Z, B, H, W, Co), dt), ((Z, B, H, W, Co), dt), ((1,), torch.float32)]

    def run(o):
        if act == 3:
            o[2].t.zero_()
        if entry == "plain":
            assert act in (0, 1) and not add
            _call("dgtd_conv3x3_fwd", X.p, None, Wt.p, Bi.p if bias else None, o[0].p, Z, B, H, W, Ci, Co, act, int(shared), code, st)
        else:
            _call("dgtd_conv3x3_fwd_ex", X.p, None, Wt.p, Bi.p if bias else None, o[0].p, o[1].p if act == 2 else None,
                  Add.p if add else None, Ref.p if act == 3 else None, slope.p if slope else None, o[2].p if act == 3 else None,
                  Z, B, H, W, Ci, Co, act, int(shared), code, st)
    if act == 3:   # the slope gradient is an fp32 atomic sum over workgroups: its bits may differ between launches
        first = [Buf(*o) for o in outs]
        run(first)
        second = [Buf(*o) for o in outs]
        run(second)
        torch.cuda.synchronize()
        _same_bits(first[0].t, second[0].t, name)
        y, y2, sgr = first[0].t, None, [first[2].t, second[2].t]
        first[0].guards_intact(name)
    else:
        y, y2, _ = _run_twice(run, outs, name)
    x64 = X.t.to(F64)
    refs, Ss = [], []
    for z in range(Z):
        r, S = conv_ref(x64[0 if shared else z], Wt.t[z].to(F64), Bi.t[z].to(F64) if bias else None)
        refs.append(r)
        Ss.append(S)
    ref, S = torch.stack(refs), torch.stack(Ss)
    err = C_MFMA * S
    if act == 0 or act == 1:
        r1 = _relu_keep_nan(ref) if act == 1 else ref
        if add:
            a64 = Add.t.to(F64)
            r1, err = r1 + a64, err + U32 * (r1.abs() + a64.abs())
        lo, hi = nm.bracket(r1, err, dt)
        if act == 1 and not add:     # ReLU is monotone: it commutes with the bracket
            lo, hi = nm.bracket(ref, err, dt)
            lo, hi = _relu_keep_nan(lo), _relu_keep_nan(hi)
        nm.assert_bracketed(y, lo, hi, name, ref=r1, err=err)
        nm.assert_sharp(lo, hi, name=name)
        MARGINS[family] = max(MARGINS.get(family, 0.0), nm.ratio(y, r1, err))
    elif act == 2:
        _check(y2, ref, err, dt, name + " y2", family)
        # PReLU of the STORED pre-activation; slope 0.25 makes slope * p exact, and the add is one fp32 rounding (contracted into an
        # fma or not, the same value), reproduced exactly: err 0
        p = y2.to(F64)
        yr = torch.where(p > 0, p, 0.25 * p)
        if add:
            yr = _fl32(yr + Add.t.to(F64))
        _check(y, yr, torch.zeros_like(yr), dt, name + " y", "prelu-epilogue")
    return dict(y=y, y2=y2, ref=ref, S=S, X=X, W=Wt, B=Bi, Add=Add, Ref=Ref, sgrad=sgr if act == 3 else None, name=name)


CONV_CH = [24, 32, 64, 96]


@pytest.mark.parametrize("Co", CONV_CH)
@pytest.mark.parametrize("Ci", CONV_CH)
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_fwd_all_channel_pairs(dt, Ci, Co):
    """all 16 (Ci, Co) pairs: ReLU + bias through dgtd_conv3x3_fwd, no bias / no activation through _fwd_ex (5 rows: ragged against
    every tile height; 48 columns: a partial 32-wide tile)"""
    _conv_case(dt, 2, 2, 5, 48, Ci, Co, act=1, bias=True, entry="plain")
    _conv_case(dt, 2, 2, 5, 48, Ci, Co, act=0, bias=False, seed=2)


# geometries that reach each branch of fwd_geom / dispatch_fwd_geom (the instance depends on Ci and Co as well)
CONV_GEOMS = {
    "split16": (1, 2, 5, 16),        # few workgroups: NT > 1 split over blockIdx.z, 16-wide tiles
    "split32": (1, 2, 33, 48),       # split, 32-wide tiles, a partial last tile
    "t16": (8, 8, 64, 16),           # 16-wide tiles without the split
    "mt1": (4, 8, 33, 80),           # 32-wide, MT = 1, partial last tile
    "mt2": (2, 8, 128, 128),         # MT = 2 (Ci <= 64)
    "mt4": (16, 8, 17, 128),         # MT = 4 (Ci <= 32; MT = 2 for Ci = 64), H = 17 ragged against 16-row tiles
}


@pytest.mark.parametrize("Co", [32, 64, 96])
@pytest.mark.parametrize("Ci", CONV_CH)
@pytest.mark.parametrize("geom", list(CONV_GEOMS))
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_fwd_dispatch_branches(dt, geom, Ci, Co):
    Z, B, H, W = CONV_GEOMS[geom]
    inst = conv_fwd_instance(Z, B, H, W, Ci, Co)
    if geom == "mt4" and Ci <= 32:
        assert inst[2] == 4
    if geom == "mt2" and Ci <= 64:
        assert inst[2] == 2
    if geom.startswith("split") and Co > 32:
        assert inst[4] > 1
    _conv_case(dt, Z, B, H, W, Ci, Co, act=0, bias=True, shared=(geom == "mt4"), tag=f"{inst} ")


@pytest.mark.parametrize("H", [1, 5, 17, 33])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_fwd_heights(dt, H, shared):
    _conv_case(dt, 3, 2, H, 32, 24, 24, act=1, shared=shared)
    _conv_case(dt, 3, 2, H, 16, 64, 96, act=0, shared=shared, seed=3)


@pytest.mark.parametrize("act,bias,add", [(0, True, True), (1, False, True), (2, True, False), (2, False, True), (3, False, False),
                                          (3, True, True)])
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_fwd_epilogues(dt, act, bias, add):
    Z, B, H, W, Ci, Co = 2, 2, 17, 48, 64, 32
    if act != 3:
        _conv_case(dt, Z, B, H, W, Ci, Co, act=act, bias=bias, add=add)
        return
    # PReLU backward: v = round(conv + bias) is not stored by this call; the same kernel with act 0 stores exactly that rounding
    v = _conv_case(dt, Z, B, H, W, Ci, Co, act=0, bias=bias)["y"].to(F64)
    c = _conv_case(dt, Z, B, H, W, Ci, Co, act=3, bias=bias, add=add)
    r = c["Ref"].t.to(F64)
    neg = ~(r > 0)
    yr = torch.where(neg, 0.25 * v, v)            # exact (slope 0.25); the add below is one fp32 rounding, reproduced exactly
    if add:
        yr = _fl32(yr + c["Add"].t.to(F64))
    _check(c["y"], yr, torch.zeros_like(yr), dt, c["name"] + " y", "prelu-bwd-epilogue")
    # slope gradient: sum of fp32 products v r over r <= 0: per-thread chain (MT NT 16 terms), a 64-lane butterfly (6), the 4 waves
    # (3), then one atomic add per workgroup in any order (grid size)
    ci, nt, mt, twx, nsplit = conv_fwd_instance(Z, B, H, W, Ci, Co)
    th = 4 * mt * (32 // twx)
    wgs = _cdiv(W, twx) * _cdiv(H, th) * B * Z * nsplit
    chain = 1 + mt * nt * 16 + 6 + 3 + wgs
    t = torch.where(neg, v * r, torch.zeros_like(v))
    sref, serr = t.sum().reshape(1), (chain * U32 * t.abs().sum()).reshape(1)
    for k, sg in enumerate(c["sgrad"]):
        _check(sg, sref, serr, torch.float32, c["name"] + f" sgrad[{k}]", "prelu-slope-grad", sharp_at=torch.bfloat16)


@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_flip_and_masked_input_gradient(dt):
    """the input gradient: dgtd_conv3x3_flip is exactly the permute + flip, and the forward kernel on dy with that kernel and the
    forward output as the ReLU mask equals the fp64 convolution of dy * (y > 0)"""
    code, st = _code(dt), _st()
    Z, B, H, W, Ci, Co = 2, 2, 17, 48, 32, 96
    fwd = _conv_case(dt, Z, B, H, W, Ci, Co, act=1)
    w = fwd["W"]
    (wt,) = _run_twice(lambda o: _call("dgtd_conv3x3_flip", w.p, o[0].p, Z, Co, Ci, st), [((Z, Ci, 3, 3, Co), dt)], "flip")
    _same_bits(wt, w.t.flip(2, 3).permute(0, 4, 2, 3, 1).contiguous(), "conv3x3_flip vs permute + flip")
    dy = Buf((Z, B, H, W, Co), dt, _randn((Z, B, H, W, Co), 31, mean=0.3).to(dt))
    mask = Buf((Z, B, H, W, Co), dt, fwd["y"])
    WT = Buf(wt.shape, dt, wt)
    (dx,) = _run_twice(lambda o: _call("dgtd_conv3x3_fwd", dy.p, mask.p, WT.p, None, o[0].p, Z, B, H, W, Co, Ci, 0, 0, code, st),
                       [((Z, B, H, W, Ci), dt)], "masked input gradient")
    m = (mask.t.float() > 0).to(F64)
    assert 0.2 < m.mean().item() < 0.9
    refs, Ss = zip(*[conv_ref(dy.t[z].to(F64) * m[z], WT.t[z].to(F64)) for z in range(Z)])
    _check(dx, torch.stack(refs), C_MFMA * torch.stack(Ss), dt, "masked input gradient", "conv-dgrad")


def _wgrad_ref(xs64, dys64):
    """dw[co,ky,kx,ci] = sum_{b,h,w} dy[b,h,w,co] xpad[b,h+ky,w+kx,ci], db = sum dy (fp64), with sum|terms|"""
    Bn, H, W, Ci = xs64.shape
    Co = dys64.shape[-1]
    xp = F.pad(xs64, (0, 0, 1, 1, 1, 1))
    d2 = dys64.reshape(-1, Co)
    dw = torch.zeros(Co, 3, 3, Ci, dtype=F64, device=DEV)
    S = torch.zeros_like(dw)
    for ky in range(3):
        for kx in range(3):
            x2 = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Ci)
            dw[:, ky, kx, :] = d2.t() @ x2
            S[:, ky, kx, :] = d2.abs().t() @ x2.abs()
    return dw, S, d2.sum(0), d2.abs().sum(0)


def _channel_means(Co, seed):
    """per-channel means of dy of either sign and magnitude 0.5 .. 1: sum dy x has little cancellation, so the bound is sharp"""
    u = torch.rand((Co,), generator=_gen(seed), device=DEV)
    return torch.where(u < 0.5, -1.0, 1.0) * (0.5 + u)


def wgrad_geometry(B, H, W, Ci):
    tw, th = (32 if W >= 32 else 16), (4 if Ci >= 64 else 8)
    return th, tw, B * _cdiv(H, th) * _cdiv(W, tw)


def _wgrad_check(dt, dw, db, xs64, dys64, P, per, B, H, W, Ci, name):
    """dw: a per-partial MFMA chain (<= MFMA_MAX_K pixels: C_MFMA) then the fixed-order fp32 reduce over the per * P partial rows
    (conv3x3_wgrad_reduce_kernel: pairs, quads, 8-groups into two running sums, a tail, one final add: depth <= Ptot + 3).
    db: per thread every 8th pixel of each of its tiles, 8 slices, then the Ptot partials, all sequential fp32 adds."""
    th, tw, ntiles = wgrad_geometry(B, H, W, Ci)
    tiles_per_partial = _cdiv(ntiles, P)
    assert tiles_per_partial * th * tw <= MFMA_MAX_K
    Ptot = per * P
    ref, S, dbr, dbs = 0, 0, 0, 0
    for xs, dys in zip(xs64, dys64):
        r = _wgrad_ref(xs, dys)
        ref, S, dbr, dbs = ref + r[0], S + r[1], dbr + r[2], dbs + r[3]
    _check(dw, ref, (C_MFMA + (Ptot + 3) * U32) * S, dt, name + " dw", "conv-wgrad")
    _check(db, dbr, (th * tw // 8 * tiles_per_partial + 8 + Ptot) * U32 * dbs, dt, name + " db", "conv-wgrad-bias")


def _wgrad_splits(Lfn, Z, B, H, W, Ci, Co):
    ws = Lfn("dgtd_conv3x3_wgrad_workspace")(Z, B, H, W, Ci, Co)
    per = Z * _cdiv(Co, 32) * 32 * (9 * _cdiv(Ci, 32) * 32 + 1) * 4
    assert ws % per == 0
    return ws // per, ws


@pytest.mark.parametrize("Ci,Co", [(24, 96), (32, 64), (64, 24), (96, 32)])
@pytest.mark.parametrize("W", [16, 48])
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_wgrad(dt, Ci, Co, W):
    """dw and db for all four CI kernels in both tile widths, ragged H and W, masked dy, P > 1 partial rows"""
    code, st = _code(dt), _st()
    Z, B, H = 2, 2, 17
    x = Buf((Z, B, H, W, Ci), dt, _randn((Z, B, H, W, Ci), 41, mean=0.5).to(dt))
    mu = _channel_means(Co, 42)
    dy = Buf((Z, B, H, W, Co), dt, (_randn((Z, B, H, W, Co), 43) + mu).to(dt))
    mask = Buf((Z, B, H, W, Co), dt, _randn((Z, B, H, W, Co), 44, mean=0.7).to(dt))
    P, wsb = _wgrad_splits(_lib_fn, Z, B, H, W, Ci, Co)
    assert P > 1
    ws = torch.empty(wsb // 4, device=DEV, dtype=torch.float32)
    name = f"{dt} wgrad {Ci}->{Co} W{W} P{P}"
    dw, db = _run_twice(lambda o: _call("dgtd_conv3x3_wgrad", x.p, dy.p, mask.p, o[0].p, o[1].p, ws.data_ptr(), Z, B, H, W, Ci, Co, 0, code, st),
                        [((Z, Co, 3, 3, Ci), dt), ((Z, Co), dt)], name)
    m = (mask.t.float() > 0).to(F64)
    for z in range(Z):
        _wgrad_check(dt, dw[z], db[z], [x.t[z].to(F64)], [dy.t[z].to(F64) * m[z]], P, 1, B, H, W, Ci, f"{name} z{z}")


@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_wgrad_batched_shared_slots(dt):
    """the deferred phase: 6 entries feeding 2 weights (3 each), masks on some entries only; dw[slot] = the sum over its entries"""
    code, st = _code(dt), _st()
    n, nslots, B, H, W, Ci, Co = 6, 2, 2, 17, 48, 24, 24
    slot = [0, 1, 1, 0, 0, 1]
    xs = [Buf((B, H, W, Ci), dt, _randn((B, H, W, Ci), 50 + i, mean=0.5).to(dt)) for i in range(n)]
    mu = _channel_means(Co, 60)
    dys = [Buf((B, H, W, Co), dt, (_randn((B, H, W, Co), 61 + i) + mu).to(dt)) for i in range(n)]
    masks = [Buf((B, H, W, Co), dt, _randn((B, H, W, Co), 70 + i, mean=0.7).to(dt)) if i % 2 else None for i in range(n)]
    wsb = _lib_fn("dgtd_conv3x3_wgrad_batched_workspace")(n, B, H, W, Ci, Co)
    P, _ = _wgrad_splits(_lib_fn, n, B, H, W, Ci, Co)
    assert P > 1
    ws = torch.empty(wsb // 4, device=DEV, dtype=torch.float32)
    Pn = C.c_void_p * n

    def run(o):
        dwp = (C.c_void_p * nslots)(*[o[k].p for k in range(nslots)])
        dbp = (C.c_void_p * nslots)(*[o[nslots + k].p for k in range(nslots)])
        _call("dgtd_conv3x3_wgrad_batched", Pn(*[t.p for t in xs]), Pn(*[t.p for t in dys]), Pn(*[m.p if m else None for m in masks]),
              (C.c_int * n)(*slot), n, dwp, dbp, nslots, ws.data_ptr(), B, H, W, Ci, Co, code, st)
    outs = [((Co, 3, 3, Ci), dt)] * nslots + [((Co,), dt)] * nslots
    res = _run_twice(run, outs, f"{dt} wgrad_batched")
    for k in range(nslots):
        idx = [i for i in range(n) if slot[i] == k]
        dy64 = [dys[i].t.to(F64) * ((masks[i].t.float() > 0).to(F64) if masks[i] else 1.0) for i in idx]
        _wgrad_check(dt, res[k], res[nslots + k], [xs[i].t.to(F64) for i in idx], dy64, P, len(idx), B, H, W, Ci, f"{dt} wgrad_batched slot{k}")


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_conv3x3_nan_pixel_spreads_to_its_neighbourhood(dt, act):
    """a NaN input pixel makes every output channel of its 3x3 neighbourhood NaN whatever the activation (F.relu / PReLU of NaN is
    NaN), and nothing else"""
    Z, B, H, W, Ci, Co = 1, 2, 9, 32, 32, 64
    x, _, _ = _conv_operands(Z, B, H, W, Ci, Co, dt, 81)
    x[0, 1, 4, 7, 3] = float("nan")
    c = _conv_case(dt, Z, B, H, W, Ci, Co, act=act, x=x, seed=81)
    want = torch.zeros(Z, B, H, W, Co, dtype=torch.bool, device=DEV)
    want[0, 1, 3:6, 6:9, :] = True
    assert torch.equal(torch.isnan(c["y"].float()), want)


def test_conv3x3_fp16_overflow_is_inf():
    dt, Z, B, H, W, Ci, Co = torch.float16, 1, 2, 9, 32, 64, 32
    x, w, _ = _conv_operands(Z, B, H, W, Ci, Co, dt, 91)
    s = math.sqrt(2 * 65520.0 / conv_ref(x[0].to(F64), w[0].to(F64))[0].abs().median().item())
    x, w = (x.float() * s).to(dt), (w.float() * s).to(dt)
    c = _conv_case(dt, Z, B, H, W, Ci, Co, act=0, x=x, w=w, seed=91, family="conv-fp16-range")
    assert 0.05 < torch.isinf(c["y"].float()).float().mean().item() < 0.95


# ---------------------------------------------------------------------------------------------- GELU, exhaustively
def _all_values(dt):
    """every finite value of a 16-bit type, then +inf, -inf, NaN"""
    v = torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(dt)
    v = v[torch.isfinite(v.float())]
    return torch.cat([v, torch.tensor([float("inf"), -float("inf"), float("nan")], device=DEV).to(dt)])


def _check_gelu(got, x, dt, name, grad):
    """finite inputs against the fp64 bound; +-inf / NaN against F.gelu in fp32 on the device.  Sharpness is demanded where the
    absolute bound is below the output's own rounding: x >= -3 (Phi(-3) = 1.3e-3; below that PHI_ABS |x| grows past half an ulp of
    x Phi(x) -- common.h states the bound is absolute)."""
    xf = x.to(F64)
    fin = torch.isfinite(xf)
    ref, err = (gelu_grad_ref if grad else gelu_ref)(xf[fin])
    lo, hi = nm.bracket(ref, err, got.dtype)
    nm.assert_bracketed(got[fin], lo, hi, name, ref=ref, err=err)
    core = xf[fin] >= -3
    nm.assert_sharp(lo[core], hi[core], name=name)
    MARGINS["gelu-grad" if grad else "gelu"] = max(MARGINS.get("gelu-grad" if grad else "gelu", 0.0), nm.ratio(got[fin], ref, err))
    xs = x[~fin].float().clone().requires_grad_(True)
    t = F.gelu(xs)
    if grad:
        t.backward(torch.ones_like(t))
        t = xs.grad
    k = got[~fin].float()
    for xv, kv, tv in zip(xs.tolist(), k.tolist(), t.detach().tolist()):
        if math.isnan(tv) and math.isnan(kv) or kv == tv:
            continue
        # x = +inf: the kernel returns inf * Phi(inf) = inf, the limit of x Phi(x); F.gelu's fp32 form may give NaN there.  Either is
        # non-finite, which is all the loss scaler and the training step look at.
        assert not grad and xv == math.inf and kv == math.inf, f"{name}: gelu{'_grad' if grad else ''}({xv}) = {kv}, F.gelu gives {tv}"


@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_gelu_exhaustive_gemm_epilogues(dt):
    """dgtd_gemm_bias_gelu with B = I (pre = A exactly) and dgtd_gemm_gelu_bwd with an upstream factor of exactly 1"""
    code, st = _code(dt), _st()
    v = _all_values(dt)
    K = N = 64
    M = _cdiv(v.numel(), N * BM) * BM
    # the non-finite values get rows of their own: inf * 0 in the other columns of their row is NaN, which the fp64 reference repeats
    nfin = 3
    a = torch.zeros(M, K, dtype=dt, device=DEV)
    fin = v[:-nfin]
    a.view(-1)[:fin.numel()] = fin
    for i in range(nfin):
        a[M - 1 - i, i] = v[-nfin + i]
    A, I = Buf((M, K), dt, a), Buf((N, K), dt, torch.eye(N, K, dtype=dt, device=DEV))
    pre, h = _run_twice(lambda o: _call("dgtd_gemm_bias_gelu", A.p, I.p, None, o[0].p, o[1].p, M, N, K, code, st),
                        [((M, N), dt), ((M, N), dt)], f"{dt} exhaustive gemm_gelu")
    acc, _ = _mm64(A.t, I.t)
    nm.assert_bracketed(pre, *nm.bracket(acc, torch.zeros_like(acc), dt), "pre = A")
    sel = torch.cat([torch.arange(fin.numel(), device=DEV)] + [torch.tensor([(M - 1 - i) * N + i], device=DEV) for i in range(nfin)])
    x = a.view(-1)[sel]
    _check_gelu(h.reshape(-1)[sel], x, dt, f"{dt} gemm_bias_gelu", grad=False)
    # gelu_bwd: dy = e_0 rows, w_t[:, 0] = 1 -> the accumulator is exactly 1 everywhere; pre = the values
    dy = torch.zeros(M, K, dtype=dt, device=DEV)
    dy[:, 0] = 1
    wt = torch.zeros(N, K, dtype=dt, device=DEV)
    wt[:, 0] = 1
    DY, WT = Buf((M, K), dt, dy), Buf((N, K), dt, wt)
    P = Buf((M, N), dt, torch.zeros(M, N, dtype=dt, device=DEV))
    P.t.view(-1)[:v.numel()] = v
    ws_bytes = _lib_fn("dgtd_gemm_gelu_bwd_workspace")(M, N)
    nb = C.c_int(0)
    dp, _ = _run_twice(lambda o: _call("dgtd_gemm_gelu_bwd", DY.p, WT.p, P.p, o[0].p, o[1].p, C.byref(nb), M, N, K, code, st),
                       [((M, N), dt), ((ws_bytes // 4 // N, N), torch.float32)], f"{dt} exhaustive gemm_gelu_bwd")
    _check_gelu(dp.reshape(-1)[:v.numel()], v, dt, f"{dt} gemm_gelu_bwd", grad=True)


@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_gelu_exhaustive_gelu_bias_bwd(dt):
    code, st = _code(dt), _st()
    v = _all_values(dt)
    Cc = 128
    rows = _cdiv(v.numel(), Cc)
    pre = torch.zeros(rows, Cc, dtype=dt, device=DEV)
    pre.view(-1)[:v.numel()] = v
    G, Pr = Buf((rows, Cc), dt, torch.ones(rows, Cc, dtype=dt, device=DEV)), Buf((rows, Cc), dt, pre)
    ws = torch.empty(_lib_fn("dgtd_colsum2_workspace")(Cc) // 4 + 1, device=DEV, dtype=torch.float32)
    dp, _ = _run_twice(lambda o: _call("dgtd_gelu_bias_bwd", G.p, Pr.p, o[0].p, o[1].p, _code(torch.float32), ws.data_ptr(), rows, Cc, code, st),
                       [((rows, Cc), dt), ((Cc,), torch.float32)], f"{dt} gelu_bias_bwd")
    _check_gelu(dp.reshape(-1)[:v.numel()], v, dt, f"{dt} gelu_bias_bwd", grad=True)


def _dwconv_gelu(dt, vals, K, C_, mode, name):
    """dgtd_dwconv_fwd with the centre tap 1, every other tap 0, no bias, on the finite values followed by one image that holds the
    three non-finite ones (inf * 0 turns their neighbours into NaN, so they are kept away from the rest).  Returns the outputs at
    the positions of `vals`."""
    code, st = _code(dt), _st()
    H, W = 16, 32
    per_img = H * W * C_
    nf = 3
    fin = vals[:-nf]
    Bn = _cdiv(fin.numel(), per_img) + 1
    x = torch.zeros(Bn, H, W, C_, dtype=dt, device=DEV)
    x.view(-1)[:fin.numel()] = fin
    for i in range(nf):
        x[Bn - 1, H // 2, W // 2, i] = vals[-nf + i]
    wt = torch.zeros(K * K, C_, dtype=torch.float32, device=DEV)
    wt[(K * K) // 2] = 1
    X, WT = Buf(x.shape, dt, x), Buf(wt.shape, torch.float32, wt)
    aux = Buf(x.shape, dt, torch.ones_like(x))
    (y,) = _run_twice(lambda o: _call("dgtd_dwconv_fwd", X.p, WT.p, None, aux.p, o[0].p, Bn, H, W, C_, K, mode, code, st),
                      [(x.shape, dt)], name)
    return torch.cat([y.reshape(-1)[:fin.numel()], y[Bn - 1, H // 2, W // 2, :nf]])


@pytest.mark.parametrize("K,C_", [(3, 64), (7, 128)], ids=["sliding3x3", "tiled7x7"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dt", HALVES, ids=str)
def test_gelu_exhaustive_dwconv(dt, mode, K, C_):
    v = _all_values(dt)
    y = _dwconv_gelu(dt, v, K, C_, mode, f"{dt} dwconv k{K} mode{mode}")
    _check_gelu(y, v, dt, f"{dt} dwconv k{K} mode{mode}", grad=mode == 2)


@pytest.mark.parametrize("K,C_", [(3, 64), (7, 128)], ids=["sliding3x3", "tiled7x7"])
@pytest.mark.parametrize("mode", [1, 2])
def test_gelu_fp32_dwconv_every_exponent(mode, K, C_):
    """fp32: 2^20 values over every exponent (subnormals included) of both signs.  A fp32 bracket with the absolute bound is a few
    ulps wide everywhere, so sharpness is demanded at fp16 resolution (an error of a 16-bit rounding would be caught)."""
    n = 1 << 20
    g = _gen(99)
    e = torch.randint(-149, 128, (n,), generator=g, device=DEV).to(F64)
    m = 1 + torch.rand(n, generator=g, device=DEV, dtype=F64)
    s = torch.where(torch.rand(n, generator=g, device=DEV) < 0.5, -1.0, 1.0).to(F64)
    x = (s * m * torch.exp2(e)).clamp(-3e38, 3e38).to(torch.float32)
    v = torch.cat([x, torch.tensor([float("inf"), -float("inf"), float("nan")], device=DEV)])
    y = _dwconv_gelu(torch.float32, v, K, C_, mode, f"fp32 dwconv k{K} mode{mode}")
    xf = v.to(F64)
    fin = torch.isfinite(xf)
    ref, err = (gelu_grad_ref if mode == 2 else gelu_ref)(xf[fin])
    lo, hi = nm.bracket(ref, err, torch.float32)
    nm.assert_bracketed(y[fin], lo, hi, f"fp32 dwconv k{K} mode{mode}", ref=ref, err=err)
    core = xf[fin] >= -3
    nm.assert_sharp(*[t[core] for t in nm.bracket(ref, err, torch.float16)], name=f"fp32 dwconv k{K} mode{mode} (at fp16 resolution)")
    fam = "gelu-grad-fp32" if mode == 2 else "gelu-fp32"
    MARGINS[fam] = max(MARGINS.get(fam, 0.0), nm.ratio(y[fin], ref, err))
    # +inf, -inf, NaN: gelu gives inf (x Phi(x) -> inf), NaN (-inf * 0), NaN; gelu' gives NaN for all three (x pdf = +-inf * 0), as F.gelu's
    # backward does
    got = y[~fin].tolist()
    want = [float("nan")] * 3 if mode == 2 else [float("inf"), float("nan"), float("nan")]
    for k, w in zip(got, want):
        assert (math.isnan(k) and math.isnan(w)) or k == w, (got, want)
