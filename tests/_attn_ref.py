"""fp64 reference, error model, kernel-arithmetic emulation and dispatch mirror of the spatial-reduction attention kernels
(csrc/attn_fwd.hip, csrc/attn_bwd.hip).  Device-agnostic torch, test helper only (imported as ``_attn_ref``; not a conftest).

Storage layout: q, out, dout, dq [B, N, heads*64]; kv, dkv [B, Nkv, 2*heads*64] (K then V); lse, delta [B, heads, N].
Everything below works per head in fp64: Q, dO, O, dQ [B, heads, N, 64]; K, V, dK, dV [B, heads, Nkv, 64]; S, P, dS [B, heads, N, Nkv].
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

import _numerics as nm
from _kernel_check import C_MFMA, MFMA_MAX_K, U32

F64 = torch.float64
HALVES = (torch.bfloat16, torch.float16)

# ---- error constants (each with its source; none is fitted to an observed error)
# unit roundoff (half an ulp, relative) of the 16-bit I/O types, 2^-p for p significand bits (bf16: 8, fp16: 11): P and dS are rounded
# to the I/O type before the second MFMA (attn_fwd.hip `pb[j] = (bf16_t)sc[kt][8 * s2 + j]`, attn_bwd.hip `pf[j] = ...; df[j] = ...`)
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
# half the subnormal spacing of the I/O type: the ABSOLUTE rounding error of a P or dS below the smallest normal (fp16: 2^-25 for
# values below 6.1e-5, which most of a softmax row is); bf16 has the fp32 exponent range, its term is 2^-134
SUB16 = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 0.0}
# v_exp_f32 (__builtin_amdgcn_exp2f, 16-bit kernels): 1 ulp per the CDNA ISA guide's accuracy table = 2 unit roundoffs; a result below
# 2^-126 is flushed to zero (FLUSH32, absolute)
EXP_HW = 2 * U32
FLUSH32 = 2.0 ** -126
# exp2f and logf of the device library (fp32 kernels, and logf in every forward): the OpenCL C numerical-compliance table the library is
# written to allows 3 ulp for both = 6 unit roundoffs
EXP_LIB = 6 * U32
LOG_LIB = 6 * U32
# 1.f / l_tot: correctly rounded or v_rcp_f32 (1 ulp), whichever the compiler picks: 2 unit roundoffs
RCP = 2 * U32
# delta = rowsum(dO * O): 16-bit: 32 products and 32 additions per lane (or 32 fmas) and the cross-half add (attn_bwd.hip, the `dl +=`
# loop of sra_bwd_dq_bf16 and its __shfl_xor); fp32: attn_delta_kernel, 4 terms per lane and 4 group_sum levels - fewer
DELTA_CHAIN = 2 * 32 + 1


# ---------------------------------------------------------------------------------------------- layout
def to_heads(x, heads):
    """[B, n, heads*64] -> fp64 [B, heads, n, 64]"""
    B, n, C = x.shape
    assert C == heads * 64
    return x.to(F64).view(B, n, heads, 64).transpose(1, 2)


def kv_to_heads(kv, heads):
    """[B, Nkv, 2*heads*64] -> (K, V) fp64 [B, heads, Nkv, 64]"""
    C = heads * 64
    return to_heads(kv[..., :C], heads), to_heads(kv[..., C:], heads)


def _T(x):
    return x.transpose(-1, -2)


def make_inputs(B, N, Nkv, heads, dtype, family="standard", seed=0, device="cpu"):
    """(q, kv, dout) in `dtype`, drawn on the CPU (the same values on every device).
    standard: q, k ~ N(0,1); v and dO have a non-zero mean so that outputs do not cancel; the LAST query row carries a 16x larger dO
              (a query row lost from dK / dV must show at every N, and its relative weight falls as 1/sqrt(N) otherwise).
    sharp:    q * 4: peaked rows, alpha << 1 between register units, rows with P ~ 1.
    spiked:   one key of the last 32-key tile dominates query row 7 (or the last row of a shorter q): k = 4 q."""
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + 7 * N + Nkv)
    C = heads * 64
    q = torch.randn(B, N, C, generator=g)
    kv = torch.randn(B, Nkv, 2 * C, generator=g)
    kv[..., C:] += 0.5
    dout = torch.randn(B, N, C, generator=g) + 0.5
    dout[:, -1] *= 16.0
    if family == "sharp":
        q *= 4.0
    elif family == "spiked":
        row, key = min(7, N - 1), Nkv - 1 - min(3, Nkv - 1)
        kv[0, key, :C] = q[0, row] * 4.0
    else:
        assert family == "standard", family
    return q.to(dtype).to(device), kv.to(dtype).to(device), dout.to(dtype).to(device)


# ---------------------------------------------------------------------------------------------- fp64 reference
def reference(q, kv, dout, heads, scale, out_stored=None):
    """fp64 attention forward and backward from the exact stored operands.  Where the kernel reads a stored, rounded intermediate
    the reference starts from it: delta = rowsum(dO * out_stored) uses the `out` the forward kernel wrote (O itself when None).
    P comes from the fp64 lse."""
    Q, (K, V), G = to_heads(q, heads), kv_to_heads(kv, heads), to_heads(dout, heads)
    S = scale * (Q @ _T(K))
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O = P @ V
    Os = O if out_stored is None else to_heads(out_stored, heads)
    delta = (G * Os).sum(-1)
    dP = G @ _T(V)
    dS = scale * P * (dP - delta[..., None])
    return SimpleNamespace(S=S, P=P, lse=lse, O=O, delta=delta, dS=dS, dQ=dS @ K, dK=_T(dS) @ Q, dV=_T(P) @ G, Os=Os, dP=dP)


# ---------------------------------------------------------------------------------------------- dispatch mirror
def _cdiv(a, b):
    return -(-a // b)


def plan(B, N, Nkv, heads, dtype):
    """What dgtd_sra_attn_fwd / _bwd launch for this shape (DGTD_DKDV_WGS unset).  16-bit types:
         (qtw, KCH, nchunks, units, kgroups, nq, qch, nqc)   units = register units the forward runs in each LDS chunk
       fp32: (qtw, KCH, nchunks, qch, nslices)"""
    groups, bh = _cdiv(N, 128), B * heads
    qtw = 1
    while qtw < 8 and groups * bh // (qtw * 2) >= 512:            # pick_qtw, and its twin in dgtd_sra_attn_bwd
        qtw *= 2
    qtiles = _cdiv(N, 32)
    if dtype == torch.float32:
        KCH = 64 if Nkv <= 64 else 128
        qch = 1
        while qch < 32 and _cdiv(qtiles, qch * 2) * bh >= 512:
            qch *= 2
        return (qtw, KCH, _cdiv(Nkv, KCH), qch, _cdiv(Nkv, 256))
    KCH, KREG = (64, 64) if Nkv <= 64 else (256, 128)
    nchunks = _cdiv(Nkv, KCH)
    units = tuple(_cdiv(min(KCH, Nkv - c * KCH), KREG) for c in range(nchunks))
    kgroups = _cdiv(Nkv, 128)
    cols = bh * kgroups
    nq = min(qtiles, max(1, _cdiv(512 if cols <= 32 else 256, cols)))
    while nq > 1 and nq * B * Nkv * 2 * heads * 64 * 4 > 1024 * 65536:    # the slabs must fit the workspace
        nq -= 1
    qch = _cdiv(qtiles, nq)
    return (qtw, KCH, nchunks, units, kgroups, nq, qch, _cdiv(qtiles, qch))


def _chains(B, N, Nkv, heads, dtype):
    """lengths the error model needs: (register units of the forward, scores per lane and unit, extra fp32 additions into dq,
    into dkv, longest MFMA accumulation)"""
    pl = plan(B, N, Nkv, heads, dtype)
    if dtype == torch.float32:
        qtw, KCH, nchunks, qch, nslices = pl
        nwaves = _cdiv(min(Nkv, 256), 32)
        # dq: LDS atomics of the waves of a slice, then one read-add-store per further slice; dkv: one global atomic per workgroup
        return nchunks, KCH // 2, nwaves * nslices + nslices, _cdiv(_cdiv(N, 32), qch), max(Nkv, qch * 32)
    qtw, KCH, nchunks, units, kgroups, nq, qch, nqc = pl
    KREG = 64 if KCH == 64 else 128
    return sum(units), KREG // 2, 0, nqc - 1, max(Nkv, qch * 32)          # dkv: the slab reduce adds nqc partial sums


# ---------------------------------------------------------------------------------------------- error model
def bounds(q, kv, dout, heads, scale, dtype, r, launch=None):
    """One fp64 error tensor per output of the kernels for reference `r` (in the head layout): out, lse, delta, dq, dk, dv.
    Every term is c * (the same expression on absolute values).  Relative errors of p are first-order (they are < 1e-4).
    launch: the (B, N, Nkv, heads) whose dispatch sets the chain lengths, when the operands are a (batch, head) slice of it."""
    B, N, Nkv = launch[:3] if launch else (q.shape[0], q.shape[1], kv.shape[1])
    half = dtype in HALVES
    u16, sub16 = U16[dtype], SUB16[dtype]
    nun, nlane, n_dq, n_dkv, chain = _chains(B, N, Nkv, launch[3] if launch else heads, dtype)
    assert chain <= MFMA_MAX_K, chain                  # C_MFMA is stated for accumulations of at most this length
    Qa, (Ka, Va), Ga = to_heads(q, heads).abs(), tuple(t.abs() for t in kv_to_heads(kv, heads)), to_heads(dout, heads).abs()
    P = r.P
    # ---- scores.  A = scale |Q||K|^T bounds |S|.  The exp2 argument is fma(acc, sl2, -m) (16-bit) or acc * sl2 - m (fp32) with
    # sl2 = fl32(scale * LOG2E); in natural-log units its error is
    #   C_MFMA A           the MFMA accumulation of the 64 products (C_MFMA; fp32: the exact-fp32 MFMA is an fmaf chain, same guide §)
    #   2 U32 A            sl2: the rounding of the product and of the LOG2E constant
    #   U32 A              fp32 kernels only: acc * sl2 is rounded before the subtraction (attn_fwd.hip `float v = sc[kt][i] * scale_log2e`)
    #   U32 (A + Amax)     the rounding of the result, |s - m| <= A + Amax with Amax = max_k A
    # The running max m itself carries no error: it is one float that scales numerator and denominator alike, and alpha multiplies o
    # and l alike.  (This is also why "scale > 0 commutes with max" in the 16-bit forward needs scale > 0 and nothing else.)
    A = scale * (Qa @ _T(Ka))
    Amax = A.amax(-1, keepdim=True)
    n_arg = 3 if half else 4
    exp_rel = EXP_HW if half else EXP_LIB
    rel_pf = (C_MFMA + n_arg * U32) * A + U32 * Amax + exp_rel                      # relative error of one forward p
    # ---- l: a sequential per-lane sum of nlane p's per unit, `l_run * alpha + ls` per unit (2 roundings), one cross-half add; all
    # terms positive, so the relative error of l is the P-weighted mean of rel_pf plus the chain
    n_l = nun * (nlane + 2) + 1
    rel_l = (P * rel_pf).sum(-1) + n_l * U32                                          # [B, h, N]
    Pmax = P.amax(-1)                                                                 # = 1 / l: an absolute error e of p is e Pmax of P
    # ---- out = (sum_k round16(p) V) * (1 / l): u16 (and the subnormal / flush terms) on every p, the MFMA accumulation over the keys,
    # one `o *= alpha` rounding per unit, the reciprocal and the final product
    PV = P @ Va
    err_out = (P * (u16 + rel_pf)) @ Va + ((sub16 + FLUSH32) * Pmax)[..., None] * Va.sum(-2, keepdim=True) \
        + PV * (C_MFMA + nun * U32 + RCP + U32 + rel_l[..., None])
    # ---- lse = m * LN2 + logf(l): here alpha does matter (l alone is rescaled): per unit boundary exp2 of a difference of two maxima
    # (each <= Amax: U32 2 Amax for the subtraction) and its own accuracy; m * LN2: the constant and the product (or the fma);
    # logf: LOG_LIB on log l = lse - max S, l's relative error as an absolute one; the final addition
    Amx = Amax[..., 0]
    logl = r.lse - r.S.amax(-1)
    err_lse = rel_l + (nun - 1) * (exp_rel + U32 + 2 * U32 * Amx) + 2 * U32 * Amx + LOG_LIB * logl + U32 * (Amx + logl)
    # ---- delta: an fp32 chain over the stored out
    err_delta = DELTA_CHAIN * U32 * (Ga * r.Os.abs()).sum(-1)
    # ---- backward p = exp2(fma(acc, sl2, -lse2)), lse2 = fl32(lse_stored * LOG2E): the score terms as above with |s - lse| <= A + |lse|
    # for the result rounding, the error of the stored lse, and the two roundings in lse2 (constant, product)
    lse_a = r.lse.abs()[..., None]
    rel_pb = (C_MFMA + n_arg * U32) * A + 3 * U32 * lse_a + err_lse[..., None] + exp_rel
    # ---- dS = p * (dP - delta) * scale: the error of p, the MFMA error of dP = dO V^T, the error of delta, the subtraction and the two
    # products (3 U32); then the rounding to the I/O type
    dPa = Ga @ _T(Va)
    dla = r.delta.abs()[..., None]
    err_dS = scale * P * ((rel_pb + 3 * U32) * (dPa + dla) + C_MFMA * dPa + err_delta[..., None])
    dSa = r.dS.abs()
    E_dS = u16 * (dSa + err_dS) + sub16 + err_dS
    err_P = P * rel_pb
    E_P = u16 * (P + err_P) + sub16 + FLUSH32 + err_P
    # ---- dQ = dS K, dK = dS^T Q, dV = P^T dO: the propagated operand error, the MFMA accumulation, and the fp32 additions outside the
    # MFMA (fp32 dq: LDS atomics of the waves and the read-add-store across key slices; dkv: the slab reduce's nqc partial sums, or
    # the fp32 kernel's one global atomic per workgroup)
    err_dq = E_dS @ Ka + (C_MFMA + n_dq * U32) * (dSa @ Ka)
    err_dk = _T(E_dS) @ Qa + (C_MFMA + n_dkv * U32) * (_T(dSa) @ Qa)
    err_dv = _T(E_P) @ Ga + (C_MFMA + n_dkv * U32) * (_T(P) @ Ga)
    return dict(out=err_out, lse=err_lse, delta=err_delta, dq=err_dq, dk=err_dk, dv=err_dv)


OUTPUTS = ("out", "lse", "delta", "dq", "dk", "dv")


def ref_of(r):
    return dict(out=r.O, lse=r.lse, delta=r.delta, dq=r.dQ, dk=r.dK, dv=r.dV)


def out_dtype(name, dtype):
    """the type the kernel rounds each output to: out and dq in the I/O type, lse, delta and dkv in fp32"""
    return dtype if name in ("out", "dq") else torch.float32


def heads_of(got, heads):
    """kernel outputs in the storage layout (out, lse, delta, dq, dkv) -> the head layout of ref_of()"""
    dk, dv = kv_to_heads(got["dkv"], heads)
    return dict(out=to_heads(got["out"], heads), lse=got["lse"].to(F64), delta=got["delta"].to(F64), dq=to_heads(got["dq"], heads),
                dk=dk, dv=dv)


def outside(got, ref, err, dtype):
    """number of elements of `got` (head layout, values of the output's type) outside [round(ref - err), round(ref + err)], NaN
    mismatches included"""
    lo, hi = nm.bracket(ref, err, dtype)
    g, lo, hi = got.to(F64), lo.to(F64), hi.to(F64)
    gn, ln = torch.isnan(g), torch.isnan(lo)
    return int(((gn != ln) | (~gn & ~ln & ((g < lo) | (g > hi)))).sum())


# ---------------------------------------------------------------------------------------------- emulation of the kernels' arithmetic
MUTATIONS = ("m1", "m2", "m3", "m4", "m5", "m6")


def applicable(mut, Nkv, dtype):
    return {"m1": Nkv % 32 != 0, "m2": dtype == torch.float16, "m3": Nkv > 128}.get(mut, True)


def emulate(q, kv, dout, heads, scale, dtype, mutate=None):
    """fp64 emulation of the arithmetic the 16-bit kernels document: P rounded to the I/O type before P V, O stored in the I/O type, lse
    stored in fp32, the backward's P recomputed from the stored lse, delta from the stored O, P and dS rounded to the I/O type before the
    three gradient products, dq stored in the I/O type and dkv in fp32.  Everything else is exact.  Returns the storage layout
    (out, lse, delta, dq, dkv) with the values of the stored types, in fp64.

    mutate (a bug of the kind the bounds must see):
      m1  the zero-filled padding keys of a ragged 32-key tile take part in the forward softmax with score 0
      m2  P and dS go through bf16 in the fp16 kernel
      m3  O is not rescaled by alpha at the register-unit boundary at key 128
      m4  delta is summed over the 32 channels of lane half 0 only (the missing cross-half shuffle)
      m5  the last query row is missing from dK / dV
      m6  the last key is missing from dQ"""
    assert mutate is None or mutate in MUTATIONS, mutate
    B, N, C = q.shape
    Nkv = kv.shape[1]
    rt = lambda x, dt: nm.round_to(x, dt).to(F64)
    r16 = (lambda x: rt(x, torch.bfloat16)) if mutate == "m2" else (lambda x: rt(x, dtype))
    Q, (K, V), G = to_heads(q, heads), kv_to_heads(kv, heads), to_heads(dout, heads)
    S = scale * (Q @ _T(K))
    # ---- forward
    Sf, Vf = S, V
    if mutate == "m1":
        npad = -Nkv % 32
        Sf = torch.cat([S, S.new_zeros(*S.shape[:-1], npad)], -1)
        Vf = torch.cat([V, V.new_zeros(*V.shape[:-2], npad, 64)], -2)
    m = Sf.amax(-1, keepdim=True)
    p = torch.exp(Sf - m)
    l = p.sum(-1, keepdim=True)
    if mutate == "m3":
        # unit A = keys [0, 128) was exponentiated against its own max mA and never rescaled to the final m
        mA = Sf[..., :128].amax(-1, keepdim=True)
        p = torch.cat([torch.exp(Sf[..., :128] - mA), p[..., 128:]], -1)
    out = rt((r16(p) @ Vf) / l, dtype)
    lse = rt(m[..., 0] + torch.log(l[..., 0]), torch.float32)
    # ---- backward
    P = torch.exp(S - lse[..., None])
    GO = G * out
    if mutate == "m4":
        half0 = (torch.arange(64, device=q.device) // 8) % 2 == 0        # lane half h holds channels 16 s + 8 h .. + 7
        GO = GO * half0
    delta = rt(GO.sum(-1), torch.float32)
    dS16 = r16(scale * P * (G @ _T(V) - delta[..., None]))
    P16 = r16(P)
    dq = rt(dS16[..., :Nkv - 1] @ K[..., :Nkv - 1, :] if mutate == "m6" else dS16 @ K, dtype)
    if mutate == "m5":
        dS16, P16, Q, G = dS16[..., :N - 1, :], P16[..., :N - 1, :], Q[..., :N - 1, :], G[..., :N - 1, :]
    dk, dv = rt(_T(dS16) @ Q, torch.float32), rt(_T(P16) @ G, torch.float32)
    un = lambda x: x.transpose(1, 2).reshape(B, -1, C)
    return dict(out=un(out), lse=lse, delta=delta, dq=un(dq), dkv=torch.cat([un(dk), un(dv)], -1))


# ---------------------------------------------------------------------------------------------- the cases of both attention numerics tests
# (B, N, Nkv, heads) -> (plan of the 16-bit types, plan of fp32), as read off csrc/attn_fwd.hip / attn_bwd.hip by hand
CASES = {
    (1, 32, 32, 1): ((1, 64, 1, (1,), 1, 1, 1, 1), (1, 64, 1, 1, 1)),          # one tile of everything
    (2, 100, 37, 2): ((1, 64, 1, (1,), 1, 4, 1, 4), (1, 64, 1, 1, 1)),         # ragged N and ragged Nkv inside KCH = 64
    (1, 130, 64, 1): ((1, 64, 1, (1,), 1, 5, 1, 5), (1, 64, 1, 1, 1)),         # Nkv = 64 exactly: no mask; 2 queries in a 2nd 128-row group
    (1, 96, 65, 2): ((1, 256, 1, (1,), 1, 3, 1, 3), (1, 128, 1, 1, 1)),        # first shape on KCH 256 / KREG 128; ragged tile with one key
    (1, 64, 129, 1): ((1, 256, 1, (2,), 2, 2, 1, 2), (1, 128, 2, 1, 1)),       # 2nd register unit with one key; kgroups 2, three idle waves
    (1, 64, 512, 1): ((1, 256, 2, (2, 2), 4, 2, 1, 2), (1, 128, 4, 1, 2)),     # two full LDS chunks; fp32: four chunks, two backward slices
    (2, 160, 300, 2): ((1, 256, 2, (2, 1), 3, 5, 1, 5), (1, 128, 3, 1, 2)),    # two chunks, ragged; fp32: dq accumulated across two slices
    (1, 1000, 70, 1): ((1, 256, 1, (1,), 1, 32, 1, 32), (1, 128, 1, 1, 1)),    # nq = 32 partial slabs of one tile each, then the reduce
    (8, 200, 200, 8): ((1, 256, 1, (2,), 2, 2, 4, 2), (1, 128, 2, 1, 1)),      # nq 2, qch 4: the 2nd query chunk is short (3 of 7 tiles)
    (16, 1000, 37, 8): ((2, 64, 1, (1,), 1, 2, 16, 2), (2, 64, 1, 8, 1)),      # qtw 2, staged K/V reused across t; ragged last group; fp32 qch 8
    (16, 1000, 300, 8): ((2, 256, 2, (2, 1), 3, 1, 32, 1), (2, 128, 3, 8, 2)),  # qtw 2 restaging; dK/dV plain-store branch sweeping 32 tiles
    (16, 4090, 37, 8): ((8, 64, 1, (1,), 1, 2, 64, 2), (8, 64, 1, 32, 1)),     # qtw 8; dK/dV chunks of 64 tiles
}
SHARP_CASES = [c for c in CASES if c[2] > 128]            # the five cases with more than one register unit or LDS chunk


def expected_plan(case, dtype):
    return CASES[case][1 if dtype == torch.float32 else 0]
