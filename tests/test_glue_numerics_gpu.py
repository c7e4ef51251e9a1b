"""GPU: the Hitnet decoder glue (csrc/hitnet_glue.hip: PReLU, CA gate, bilinear resize; csrc/sam.hip) in bf16, fp16 and fp32 against
the fp64 references and error models of tests/_glue_ref.py (what those models can see is shown by mutation in
test_glue_numerics_cpu.py).

Every entry is called through the C ABI.  All tensors are 16-byte aligned views at a non-zero offset inside NaN-filled buffers whose
guard regions must stay NaN; outputs, stats and scratch are pre-filled with NaN, and stats / scratch have exactly the documented (CA
gate) or reported (SAM) size.  Stages are checked one by one, each from the STORED output of the stage before.  Every output must lie in
[round(ref - err), round(ref + err)] with NaN exactly where the reference has it, at least 90 % of the brackets that are not exact ties
must be a single value (16-bit outputs at their own resolution, fp32 outputs and stats at bf16 resolution), the launch geometry must
be the one the case was chosen for, and a second launch must give identical bits for everything except the PReLU slope gradient
(atomics), whose two launches are both held to the bracket.

Two departures from "90 % single-valued at the output's own resolution", both from the number formats and both printed:
  * the two grid-stride backward resize shapes in fp16 are held to bf16 resolution: at source index 263 the kernel's fp32 index
    (delta_s = U32 (2 s + 0.5) = 3.1e-5 per axis, on taps that sum to the output) is by itself an eighth of an fp16 ulp, so no
    reference can be single-valued for 90 % of such outputs (the CPU file measures 0.81 on the reference alone);
  * the saturating CA case (gates of exactly 0 or 1) has weight gradients of exactly 0 +- the underflow term: brackets only.
Sharpness is demanded of tensors with at least 64 elements (a share of a handful of values says nothing)."""
import time

import pytest
import torch

import _glue_ref as gr
import _numerics as nm
from _kernel_check import DEV, Buf, _same_bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
F32, F64 = torch.float32, torch.float64
SHORT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}

MARGINS = {}                # family -> largest share of its error bound used
SHARP = {}                  # family -> (smallest sharp share, largest tie share)
TIMES = {}                  # test id -> wall seconds


@pytest.fixture(scope="module", autouse=True)
def L():
    import dgtd
    lib = dgtd._lib
    lib.load()
    yield lib
    if MARGINS:
        print("\nglue: largest share of each error bound used, per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(MARGINS.items())))
        print("glue: smallest share of single-valued brackets / largest share of ties, per family: "
              + ", ".join(f"{k} {a:.3f}/{b:.3f}" for k, (a, b) in sorted(SHARP.items())))
        per = {}
        for k, v in TIMES.items():
            per.setdefault(k.split("[")[0], []).append(v)
        print("glue: wall seconds per case (cases, slowest, total), per test: "
              + ", ".join(f"{k} ({len(v)}, {max(v):.2f}, {sum(v):.2f})" for k, v in per.items()))


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                 # a device error: nothing more is launched on this GPU
        pytest.exit(f"device error after {request.node.name}, stopping the module: {e}", returncode=3)
    TIMES[request.node.name] = time.time() - t0


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(got, terms, name, family, sharp=True, at=None):
    ref, err, od = terms
    assert got.dtype == od, (name, got.dtype, od)
    lo, hi = nm.bracket(ref, err, od)
    nm.assert_bracketed(got.reshape(ref.shape), lo, hi, name, ref=ref, err=err)
    MARGINS[family] = max(MARGINS.get(family, 0.0), nm.ratio(got.reshape(ref.shape), ref, err))
    if sharp and ref.numel() >= 64:
        at = at or (od if od != F32 else torch.bfloat16)
        frac, ties = gr.sharpness(ref, err, at)
        a, b = SHARP.get(family, (1.0, 0.0))
        SHARP[family] = (min(a, frac), max(b, ties))
        assert frac >= 0.9, f"{name}: only {frac:.3f} of the brackets are a single value at {at}"
        assert ties < 0.25, f"{name}: {ties:.3f} of the references are exact ties"


def _bufs(tensors, dtypes=None):
    return [Buf(t.shape, t.dtype, t.to(DEV)) for t in tensors]


def _guards(bufs, name):
    for i, b in enumerate(bufs):
        b.guards_intact(f"{name}[{i}]")


def _all_nan(b):
    return bool(torch.isnan(b.t.float()).all())


# ============================================================================================== PReLU
def _prelu_launch(L, X, G, A, n, dtype, da0):
    y, dx, da = Buf((n,), dtype), Buf((n,), dtype), Buf((1,), F32)
    da.t.fill_(da0)
    code = L.dtype_code(X.t)
    L.call("dgtd_prelu_fwd", X.p, A.p, y.p, n, code, _st())
    L.call("dgtd_prelu_bwd", X.p, G.p, A.p, dx.p, da.p, n, code, _st())
    return y, dx, da


def _prelu_case(L, x, g, dtype, slope, tag, da0=0.75):
    n = x.numel()
    X, G = _bufs([x, g])
    A = Buf((1,), F32, torch.tensor([slope], dtype=F32))
    runs = [_prelu_launch(L, X, G, A, n, dtype, da0) for _ in range(2)]
    torch.cuda.synchronize()
    for r in runs:
        _guards(r, tag)
    _guards([X, G, A], tag + " inputs")
    _same_bits(runs[0][0].t, runs[1][0].t, tag + " y")
    _same_bits(runs[0][1].t, runs[1][1].t, tag + " dx")
    r = gr.prelu_ref(X.t, G.t, slope, da0, dtype)
    _check(runs[0][0].t, (r.y, r.y_err, dtype), tag + " y", "prelu y")
    _check(runs[0][1].t, (r.dx, r.dx_err, dtype), tag + " dx", "prelu dx")
    for k in (0, 1):                                          # atomics: both launches against the bracket
        _check(runs[k][2].t, (r.da.reshape(1), r.da_err.reshape(1), F32), tag + f" da (launch {k})", "prelu da", sharp=False)
    if n >= 64 and bool(torch.isfinite(r.da)):
        frac, _ = gr.sharpness(r.da.reshape(1), r.da_err.reshape(1), torch.bfloat16)
        assert frac == 1.0, f"{tag}: the slope gradient's bracket is not a single bf16 value"
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("nv", list(gr.PRELU_CASES))
def test_prelu_vs_fp64(L, nv, dtype):
    n = nv * gr.vec(dtype)
    assert gr.prelu_plan(n, dtype) == gr.PRELU_CASES[nv]
    x, g = gr.prelu_inputs(n, dtype, seed=nv % 97)
    for slope in gr.PRELU_SLOPES:
        _prelu_case(L, x, g, dtype, slope, f"prelu {SHORT[dtype]} n={n} slope={slope}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("slope", gr.PRELU_SLOPES)
def test_prelu_zeros_subnormals_inf_and_nan_follow_fp64(L, slope, dtype):
    """+0, -0, fp16 subnormals, +-inf and one NaN: y is NaN there, dx = slope * g as torch gives, da is NaN"""
    n = (256 * 3 + 77) * gr.vec(dtype)
    x, g = gr.prelu_inputs(n, dtype, specials=True)
    r = _prelu_case(L, x, g, dtype, slope, f"prelu specials {SHORT[dtype]} slope={slope}", da0=0.0)
    assert bool(torch.isnan(r.y[50])) and bool(torch.isnan(r.da)) and bool(torch.isfinite(r.dx[50]))


# ============================================================================================== CA gate
def _other_sign(row, c):
    """a channel whose weight in `row` has the other sign than channel c's"""
    return int(((row > 0) != (row[c] > 0)).nonzero()[0])


def _ca_launch(L, bufs, case, dtype, rows):
    B, HW, C, R = case
    RES, X, G, W1, W2 = bufs
    code = L.dtype_code(RES.t)
    out, dres = Buf((B, HW, C), dtype), Buf((B, HW, C), dtype)
    stats, scratch = Buf((gr.ca_stats_floats(B, C, R),), F32), Buf((gr.ca_scratch_floats(B, C, R),), F32)
    L.call("dgtd_ca_gate_fwd", RES.p, X.p, W1.p, W2.p, out.p, stats.p, B, HW, C, R, code, _st())
    if rows:
        dw = [Buf((B, 2 * R * C), F32)]
        L.call("dgtd_ca_gate_bwd_rows", G.p, RES.p, W1.p, W2.p, stats.p, dres.p, dw[0].p, scratch.p, B, HW, C, R, code, _st())
    else:
        dw = [Buf((R, C), F32), Buf((C, R), F32)]
        L.call("dgtd_ca_gate_bwd", G.p, RES.p, W1.p, W2.p, stats.p, dres.p, dw[0].p, dw[1].p, scratch.p, B, HW, C, R, code, _st())
    return [out, dres, stats, scratch] + dw


def _ca_case(L, inp, case, dtype, rows, tag, sharp=True):
    B, HW, C, R = case
    bufs = _bufs(inp)
    runs = [_ca_launch(L, bufs, case, dtype, rows) for _ in range(2)]
    torch.cuda.synchronize()
    for r in runs:
        _guards(r, tag)
    _guards(bufs, tag + " inputs")
    for a, b in zip(*runs):
        _same_bits(a.t, b.t, tag)
    out, dres, stats, scratch = (b.t for b in runs[0][:4])
    st = gr.SimpleNamespace(pooled=stats[:B * C].view(B, C), gate=stats[B * C:2 * B * C].view(B, C),
                            hidden=stats[2 * B * C:2 * B * C + B * R].view(B, R))
    gx = gr.pool_geometry(HW, C, dtype).gx
    for part in (stats[2 * B * C + B * R:].view(64, B * C), scratch[B * C:B * C + 64 * B * C].view(64, B * C)):
        assert bool(torch.isnan(part[gx:]).all()), f"{tag}: a slice partial beyond the {gx} slices was written"
    res, x, g, w1, w2 = (b.t for b in bufs)
    T = gr.ca_fwd_terms(res, x, w1, w2, dtype, st)
    T.update(gr.ca_bwd_terms(g, res, w1, w2, dtype, st, rows=rows))
    got = dict(pooled=st.pooled, hidden=st.hidden, gate=st.gate, out=out, dres=dres)
    if rows:
        got["rows"] = runs[0][4].t
    else:
        got["dw1"], got["dw2"] = runs[0][4].t, runs[0][5].t
    for k in T:
        _check(got[k], T[k], f"{tag} {k}", "ca " + k, sharp=sharp)
    return got, T, st


CA_PARAMS = [(c, dt) for dt in DTYPES for c in gr.ca_cases(dt)]
SAM_PARAMS = [(c, dt) for dt in DTYPES for c in gr.sam_cases(dt)]


@pytest.mark.parametrize("case,dtype", CA_PARAMS, ids=[f"{c}-{SHORT[dt]}" for c, dt in CA_PARAMS])
def test_ca_gate_vs_fp64(L, case, dtype):
    assert gr.ca_plan(*case, dtype) == gr.ca_cases(dtype)[case], "the dispatch no longer takes this case where it was meant to go"
    inp = gr.ca_inputs(*case, dtype)
    tag = f"ca {SHORT[dtype]} {case}"
    got, T, st = _ca_case(L, inp, case, dtype, False, tag)
    assert bool(((st.hidden > 0).any(1) & ((st.hidden == 0).any(1) | (case[3] == 1))).all()), f"{tag}: dead and live hidden units"
    if case in gr.CA_ROWS:
        got_r, _, _ = _ca_case(L, inp, case, dtype, True, tag + " rows")
        _same_bits(got["dres"], got_r["dres"], tag + ": dres of _bwd_rows against _bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ca_gate_saturated_gates_are_0_or_1_and_never_nan(L, dtype):
    case = (2, 130, 32, 32) if dtype != F32 else (2, 130, 100, 25)
    inp = gr.ca_inputs(*case, dtype, saturate=True)
    got, T, st = _ca_case(L, inp, case, dtype, False, f"ca saturating {SHORT[dtype]}", sharp=False)
    a = st.hidden.to(F64) @ inp[4].to(DEV).to(F64).T
    assert float(a.abs().max()) > 95 and float(a.min()) < -50 and float(a.max()) > 50
    assert not bool(torch.isnan(st.gate).any()) and bool((st.gate[a < -90] < 1e-37).all()) and bool((st.gate[a > 50] == 1).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_ca_gate_nan_goes_where_fp64_puts_it(L, bad, dtype):
    """one NaN element of res makes that sample's whole out and dres NaN, and dw2 and a column of dw1 NaN; the other sample stays in
    its brackets (assert_bracketed checks both directions).  +inf: two infinite channel means of one pixel, which the rows of w1 that
    weigh them with opposite signs turn into NaN; a single one would reach the hidden units as +-inf only."""
    case = (2, 130, 32, 32) if dtype != F32 else (2, 130, 100, 25)
    res, x, g, w1, w2 = gr.ca_inputs(*case, dtype)
    res[1, 17, 5] = bad
    if bad == float("inf"):
        res[1, 17, _other_sign(w1[0], 5)] = bad
    got, T, st = _ca_case(L, (res, x, g, w1, w2), case, dtype, False, f"ca {bad} {SHORT[dtype]}", sharp=False)
    assert bool(torch.isnan(st.hidden[1]).any()) and bool(torch.isfinite(st.hidden[0]).all())
    assert bool(torch.isnan(got["out"][1]).all()) and bool(torch.isfinite(got["out"][0]).all())
    assert bool(torch.isnan(got["dres"][1]).all()) and bool(torch.isfinite(got["dres"][0]).all())
    assert bool(torch.isnan(got["dw2"]).all()) and bool(torch.isnan(got["dw1"][:, 5]).all())


# ============================================================================================== SAM
def _sam_launch(L, bufs, case, dtype):
    B, HW, C, R = case
    XH, XL, G, W1, W2, V1, V2 = bufs
    code = L.dtype_code(XH.t)
    lib = L.load()
    ns, nscr = lib.dgtd_sam_stats_floats(B, C, R), lib.dgtd_sam_scratch_floats(B, C)
    assert (ns, nscr) == (gr.sam_stats_floats(B, C, R), gr.sam_scratch_floats(B, C))
    out, dxh, dxl = (Buf((B, HW, C), dtype) for _ in range(3))
    stats, scratch, dw = Buf((ns,), F32), Buf((nscr,), F32), Buf((3 * R * C + R,), F32)
    L.call("dgtd_sam_fwd", XH.p, XL.p, W1.p, W2.p, V1.p, V2.p, out.p, stats.p, B, HW, C, R, code, _st())
    L.call("dgtd_sam_bwd", G.p, XH.p, XL.p, W1.p, W2.p, V1.p, V2.p, stats.p, dxh.p, dxl.p, dw.p, scratch.p, B, HW, C, R, code, _st())
    return [out, dxh, dxl, dw, stats, scratch]


def _sam_case(L, inp, case, dtype, tag, sharp=True):
    B, HW, C, R = case
    bufs = _bufs(inp)
    runs = [_sam_launch(L, bufs, case, dtype) for _ in range(2)]
    torch.cuda.synchronize()
    for r in runs:
        _guards(r, tag)
    _guards(bufs, tag + " inputs")
    for a, b in zip(*runs):
        _same_bits(a.t, b.t, tag)
    out, dxh, dxl, dw, stats, scratch = (b.t for b in runs[0])
    st = gr.sam_unpack(stats, B, C, R)
    gx = gr.pool_geometry(HW, C, dtype).gx
    kept = 4 * B * C + 4 * B * R + 2 * B
    for part in (stats[kept:], scratch):
        assert bool(torch.isnan(part[2 * gx * B * C:]).all()), f"{tag}: a slice partial beyond the {gx} slices was written"
    xh, xl, g, w1, w2, v1, v2 = (b.t for b in bufs)
    T = gr.sam_fwd_terms(xh, xl, w1, w2, v1, v2, dtype, st)
    T.update(gr.sam_bwd_terms(g, xh, xl, w1, w2, v1, v2, dtype, st))
    got = dict(pooled=st.pooled, hc=st.hc, hw=st.hw, gc=st.gc, gw=st.gw, out=out, dxh=dxh, dxl=dxl, dw=dw)
    for k in T:
        _check(got[k], T[k], f"{tag} {k}", "sam " + k, sharp=sharp)
    return got, st


@pytest.mark.parametrize("case,dtype", SAM_PARAMS, ids=[f"{c}-{SHORT[dt]}" for c, dt in SAM_PARAMS])
def test_sam_vs_fp64(L, case, dtype):
    assert gr.sam_plan(*case, dtype) == gr.sam_cases(dtype)[case]
    got, st = _sam_case(L, gr.sam_inputs(*case, dtype), case, dtype, f"sam {SHORT[dtype]} {case}")
    for h in (st.hc, st.hw):
        assert bool(((h > 0).any(-1) & (h == 0).any(-1)).all()), "dead and live hidden units in every sample and input"


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_sam_nan_goes_where_fp64_puts_it(L, bad, dtype):
    case = (2, 256, 32, 2)
    inp = list(gr.sam_inputs(*case, dtype))
    inp[0][1, 17, 5] = bad
    if bad == float("inf"):                                      # two infinite channel means that row 0 of W1 weighs with opposite signs
        inp[0][1, 17, _other_sign(inp[3][0], 5)] = bad
    got, st = _sam_case(L, inp, case, dtype, f"sam {bad} {SHORT[dtype]}", sharp=False)
    assert bool(torch.isnan(got["out"][1]).all()) and bool(torch.isfinite(got["out"][0]).all())
    assert bool(torch.isnan(got["dxh"][1]).all()) and bool(torch.isfinite(got["dxh"][0]).all())
    R, C = case[3], case[2]
    assert bool(torch.isnan(st.hc[0, 1, 0])) and bool(torch.isfinite(st.hc[1]).all()) and bool(torch.isnan(got["dw"][R * C:2 * R * C]).all())


SAM_C = (4, 8, 12, 16, 20, 24, 32, 40, 48, 64, 68, 96, 100, 124, 128, 132, 136)
SAM_R = (1, 2, 3, 5, 10, 11, 16, 20, 21, 31, 32, 33)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_sam_supported_agrees_with_what_sam_fwd_accepts(L, dtype):
    """a grid of (C, R): chunk counts that do not divide 256 (C / V = 3, 5, 12, 17, 31, ...), C beyond 128, R beyond 32, and
    3 R C + R on both sides of 1024 (980 / 1029 at C = 16, 970 / 1067 at C = 32, 770 / 1155 at C = 128; 1024 +- 1 itself has no
    solution with C a multiple of the chunk width)"""
    B, HW = 1, 3
    lib, code = L.load(), L.dtype_code(torch.empty(1, dtype=dtype))
    seen = set()
    for C in SAM_C:
        for R in SAM_R:
            ok = bool(lib.dgtd_sam_supported(B, HW, C, R, code))
            assert ok == gr.sam_supported(B, HW, C, R, dtype), (C, R)
            seen.add(ok)
            xh, xl = Buf((B, HW, C), dtype, torch.ones(B, HW, C)), Buf((B, HW, C), dtype, torch.ones(B, HW, C))
            w1, v1, w2, v2 = (Buf(s, F32, torch.ones(s)) for s in ((R, C), (R, C), (C, R), (R,)))
            out, stats = Buf((B, HW, C), dtype), Buf((gr.sam_stats_floats(B, C, R),), F32)
            args = ("dgtd_sam_fwd", xh.p, xl.p, w1.p, w2.p, v1.p, v2.p, out.p, stats.p, B, HW, C, R, code, _st())
            if ok:
                L.call(*args)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(out.t.float()).all()), (C, R)
            else:
                with pytest.raises(L.DgtdError):
                    L.call(*args)
                torch.cuda.synchronize()
                assert _all_nan(out) and _all_nan(stats), (C, R)
            _guards([out, stats], f"sam ({C}, {R})")
    assert seen == {True, False}


# ============================================================================================== bilinear
def _bil_fwd(L, x, Ho, Wo, align, dtype, tag, at=None):
    B, Hi, Wi, C = x.shape
    X = Buf(x.shape, dtype, x.to(DEV))
    runs = []
    for _ in range(2):
        y = Buf((B, Ho, Wo, C), dtype)
        L.call("dgtd_bilinear_fwd", X.p, y.p, B, Hi, Wi, Ho, Wo, C, int(align), L.dtype_code(X.t), _st())
        runs.append(y)
    torch.cuda.synchronize()
    _guards(runs + [X], tag)
    _same_bits(runs[0].t, runs[1].t, tag)
    return X, runs[0].t


def _bil_bwd(L, dy, Hi, Wi, align, dtype, tag):
    B, Ho, Wo, C = dy.shape
    G = Buf(dy.shape, dtype, dy.to(DEV))
    runs = []
    for _ in range(2):
        dx = Buf((B, Hi, Wi, C), dtype)
        L.call("dgtd_bilinear_bwd", G.p, dx.p, B, Hi, Wi, Ho, Wo, C, int(align), L.dtype_code(G.t), _st())
        runs.append(dx)
    torch.cuda.synchronize()
    _guards(runs + [G], tag)
    _same_bits(runs[0].t, runs[1].t, tag)
    return G, runs[0].t


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("align", [True, False], ids=["align", "half-pixel"])
@pytest.mark.parametrize("case", list(gr.BIL_CASES), ids=str)
def test_bilinear_vs_fp64(L, case, align, dtype):
    Hi, Wi, Ho, Wo = case
    V = gr.vec(dtype)
    assert gr.bil_lpi(Hi, Ho, align) == gr.BIL_CASES[case][0 if align else 1], "the dispatch no longer takes this case where it was meant to go"
    for C in ((V, 3 * V) if case == (7, 9, 19, 13) else (V,)):
        tag = f"bilinear {SHORT[dtype]} {case} C={C} align={align}"
        X, y = _bil_fwd(L, gr.bil_inputs(2, Hi, Wi, C, dtype), Ho, Wo, align, dtype, tag + " fwd")
        ref, err = gr.bil_fwd_terms(X.t, Ho, Wo, align, dtype)
        _check(y, (ref, err, dtype), tag + " fwd", "bilinear fwd")
        G, dx = _bil_bwd(L, gr.bil_inputs(2, Ho, Wo, C, dtype, seed=1), Hi, Wi, align, dtype, tag + " bwd")
        ref, err = gr.bil_bwd_terms(G.t, Hi, Wi, align, dtype)
        _check(dx, (ref, err, dtype), tag + " bwd", "bilinear bwd")
        if case == (16, 16, 16, 16):
            _same_bits(y, X.t, tag + ": the identity resize")
            _same_bits(dx, G.t, tag + ": the identity resize, backward")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("align", [True, False], ids=["align", "half-pixel"])
@pytest.mark.parametrize("which", list(gr.BIL_BIG))
def test_bilinear_grid_stride_vs_fp64(L, which, align, dtype):
    """the grid-stride loops: forward with more than 2048 * 256 items, backward at LPI 1 and LPI 2 (at LPI 8 and 16 the loop needs at
    least 16M output elements: left out)"""
    B, Hi, Wi, Ho, Wo, C = gr.BIL_BIG[which]
    plan = gr.bil_plan(B, Hi, Wi, Ho, Wo, C, align, dtype)
    tag = f"bilinear {which} {SHORT[dtype]} align={align}"
    if which == "fwd":
        assert plan[0] == 2048 and plan[1] >= 2
        X, y = _bil_fwd(L, gr.bil_inputs(B, Hi, Wi, C, dtype), Ho, Wo, align, dtype, tag)
        ref, err = gr.bil_fwd_terms(X.t, Ho, Wo, align, dtype)
        _check(y, (ref, err, dtype), tag, "bilinear fwd")
    else:
        assert plan[2] == (1 if which == "bwd-lpi1" else 2) and plan[3] == 2048 and plan[4] >= 2
        G, dx = _bil_bwd(L, gr.bil_inputs(B, Ho, Wo, C, dtype, seed=1), Hi, Wi, align, dtype, tag)
        ref, err = gr.bil_bwd_terms(G.t, Hi, Wi, align, dtype)
        if dtype == torch.float16:
            frac, ties = gr.sharpness(ref, err, dtype)
            print(f"\n{tag}: {frac:.3f} of the brackets are a single value at fp16 resolution (held to bf16 resolution, see the module docstring)")
        _check(dx, (ref, err, dtype), tag, "bilinear bwd", at=torch.bfloat16 if dtype == torch.float16 else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("align", [True, False], ids=["align", "half-pixel"])
def test_bilinear_nan_goes_where_fp64_puts_it(L, align, dtype):
    """a NaN input pixel poisons the outputs whose taps weigh it, a NaN in dy the input pixels that output reads, and nothing else.
    Exactly, up to the kernel's fp32 index: a tap whose weight is within delta_s of zero (among them the second tap at lambda = 0,
    which the forward reads as F.interpolate does and the backward skips) may go either way; every other output is NaN exactly where
    the weight is non-zero and lies in its bracket otherwise."""
    Hi, Wi, Ho, Wo = 7, 9, 19, 13
    C = gr.vec(dtype)
    b, c = 1, 2
    ah, aw = gr.bil_axis(Hi, Ho, align, DEV), gr.bil_axis(Wi, Wo, align, DEV)
    tag = f"bilinear nan {SHORT[dtype]} align={align}"
    # forward: input pixel (3, 4)
    x = gr.bil_inputs(2, Hi, Wi, C, dtype)
    x0 = x.clone()
    x[b, 3, 4, c] = float("nan")
    X, y = _bil_fwd(L, x, Ho, Wo, align, dtype, tag + " fwd")
    sure, may = ah.sure[:, 3, None] & aw.sure[None, :, 4], ah.may[:, 3, None] & aw.may[None, :, 4]
    assert int(sure.sum()) >= 4
    ref, err = gr.bil_fwd_terms(x0.to(DEV), Ho, Wo, align, dtype)
    y2 = y.clone()
    assert bool(torch.isnan(y2[b, :, :, c][sure]).all()), tag + ": an output that weighs the NaN pixel is not NaN"
    y2[b, :, :, c][may] = nm.round_to(ref[b, :, :, c][may], dtype)
    _check(y2, (ref, err, dtype), tag + " fwd", "bilinear fwd", sharp=False)
    # backward: output pixel (9, 6)
    dy = gr.bil_inputs(2, Ho, Wo, C, dtype, seed=1)
    dy0 = dy.clone()
    dy[b, 9, 6, c] = float("nan")
    G, dx = _bil_bwd(L, dy, Hi, Wi, align, dtype, tag + " bwd")
    sure, may = ah.sure[9, :, None] & aw.sure[6, None, :], ah.may[9, :, None] & aw.may[6, None, :]
    assert int(sure.sum()) >= 1
    ref, err = gr.bil_bwd_terms(dy0.to(DEV), Hi, Wi, align, dtype)
    dx2 = dx.clone()
    assert bool(torch.isnan(dx2[b, :, :, c][sure]).all()), tag + ": an input pixel the NaN output reads is not NaN"
    dx2[b, :, :, c][may] = nm.round_to(ref[b, :, :, c][may], dtype)
    _check(dx2, (ref, err, dtype), tag + " bwd", "bilinear bwd", sharp=False)


# ============================================================================================== refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_refusals_return_an_error_and_leave_the_outputs_untouched(L, dtype):
    V = gr.vec(dtype)
    code = L.dtype_code(torch.empty(1, dtype=dtype))

    def refused(*args, outs):
        with pytest.raises(L.DgtdError):
            L.call(*args)
        torch.cuda.synchronize()
        for o in outs:
            assert _all_nan(o), args[0]
        _guards(outs, args[0])

    for C, R in ((136, 8), (32, 33), (V + V // 2, 2)):           # C > 128, R > 32, C % V != 0
        B, HW = 2, 5
        res, x, g = (Buf((B, HW, C), dtype, torch.ones(B, HW, C)) for _ in range(3))
        w1, w2 = Buf((R, C), F32, torch.ones(R, C)), Buf((C, R), F32, torch.ones(C, R))
        out, dres, dw1, dw2 = Buf((B, HW, C), dtype), Buf((B, HW, C), dtype), Buf((R, C), F32), Buf((C, R), F32)
        stats, scratch = Buf((gr.ca_stats_floats(B, C, R),), F32), Buf((gr.ca_scratch_floats(B, C, R),), F32)
        refused("dgtd_ca_gate_fwd", res.p, x.p, w1.p, w2.p, out.p, stats.p, B, HW, C, R, code, _st(), outs=[out, stats])
        refused("dgtd_ca_gate_bwd", g.p, res.p, w1.p, w2.p, stats.p, dres.p, dw1.p, dw2.p, scratch.p, B, HW, C, R, code, _st(),
                outs=[dres, dw1, dw2, scratch])
        rows = Buf((B, 2 * R * C), F32)
        refused("dgtd_ca_gate_bwd_rows", g.p, res.p, w1.p, w2.p, stats.p, dres.p, rows.p, scratch.p, B, HW, C, R, code, _st(),
                outs=[dres, rows, scratch])
    for n in (V + 1, 3 * V - 1, 0):                               # n % V != 0, n = 0
        m = 4 * V
        x, g, a = Buf((m,), dtype, torch.ones(m)), Buf((m,), dtype, torch.ones(m)), Buf((1,), F32, torch.tensor([0.25]))
        y, dx, da = Buf((m,), dtype), Buf((m,), dtype), Buf((1,), F32)
        refused("dgtd_prelu_fwd", x.p, a.p, y.p, n, code, _st(), outs=[y])
        refused("dgtd_prelu_bwd", x.p, g.p, a.p, dx.p, da.p, n, code, _st(), outs=[dx, da])
    C = V + V // 2                                                # bilinear: C % V != 0
    x, y = Buf((1, 4, 4, C), dtype, torch.ones(1, 4, 4, C)), Buf((1, 8, 8, C), dtype)
    refused("dgtd_bilinear_fwd", x.p, y.p, 1, 4, 4, 8, 8, C, 1, code, _st(), outs=[y])
    dx = Buf((1, 4, 4, C), dtype)
    g = Buf((1, 8, 8, C), dtype, torch.ones(1, 8, 8, C))
    refused("dgtd_bilinear_bwd", g.p, dx.p, 1, 4, 4, 8, 8, C, 1, code, _st(), outs=[dx])
