"""CPU: what the error models of tests/_glue_ref.py (PReLU, CA gate, SAM, bilinear) can and cannot see, without a GPU.

For every case of test_glue_numerics_gpu.py and both 16-bit types the fp64 emulation of the documented kernel arithmetic lies inside
every bracket, each applicable mutation (a bug of the kind the bounds must catch) puts at least one element outside, the launch-geometry
mirrors equal the expectations read off the sources by hand, and the inputs make the references sharp on their own.  The three
grid-stride bilinear shapes take part in the geometry and sharpness checks only (their dense fp64 products are too slow for a mutation
sweep on a CPU; the same code paths are swept at the small shapes)."""
import pytest
import torch

import _glue_ref as gr
import _numerics as nm

HALVES = [torch.bfloat16, torch.float16]
F32, F64 = torch.float32, torch.float64
SHORT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
SHARES = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if SHARES:
        print("\nglue (CPU emulation): largest share of each error bound used, per family: "
              + ", ".join(f"{k} {v:.3f}" for k, v in sorted(SHARES.items())))


def _stage(name, got, terms, family, tag, sharp=False):
    ref, err, od = terms
    n = gr.outside(got.to(od), ref, err, od)
    assert n == 0, f"{tag} {name}: {n} emulated values outside their bracket"
    share = nm.ratio(got.to(od), ref, err)
    SHARES[family] = max(SHARES.get(family, 0.0), share)
    if sharp and ref.numel() >= 64:
        _sharp(ref, err, od, f"{tag} {name}")


def _caught(names, got_of, terms):
    """the stages at which a mutated emulation leaves its bracket"""
    return [n for n in names if gr.outside(got_of(n).to(terms[n][2]), terms[n][0], terms[n][1], terms[n][2]) > 0]


def _sharp(ref, err, od, tag, min_frac=0.9):
    at = od if od in HALVES else torch.bfloat16
    frac, ties = gr.sharpness(ref, err, at)
    assert frac >= min_frac and ties < 0.25, f"{tag}: sharp {frac:.3f}, ties {ties:.3f}"
    return frac, ties


# ---------------------------------------------------------------------------------------------- geometry
def test_geometry_mirrors_match_the_hand_read_expectations():
    for dt in HALVES + [F32]:
        for nv, plan in gr.PRELU_CASES.items():
            assert gr.prelu_plan(nv * gr.vec(dt), dt) == plan, (nv, dt)
        for case, plan in gr.ca_cases(dt).items():
            assert gr.ca_plan(*case, dt) == plan, (case, dt)
        for case, plan in gr.sam_cases(dt).items():
            assert gr.sam_plan(*case, dt) == plan and gr.sam_supported(*case, dt), (case, dt)
    for case, lpis in gr.BIL_CASES.items():
        assert (gr.bil_lpi(case[0], case[2], True), gr.bil_lpi(case[0], case[2], False)) == lpis, case
    assert {v[0] for v in gr.BIL_CASES.values()} | {v[1] for v in gr.BIL_CASES.values()} == {1, 2, 8, 16}
    for al in (True, False):
        assert gr.bil_plan(*gr.BIL_BIG["fwd"], al, torch.bfloat16)[:2] == (2048, 2)
        assert gr.bil_plan(*gr.BIL_BIG["bwd-lpi1"], al, torch.bfloat16)[2:] == (1, 2048, 2)
        assert gr.bil_plan(*gr.BIL_BIG["bwd-lpi2"], al, torch.bfloat16)[2:] == (2, 2048, 2)
    # sam_ok: the chunk count must divide 256, and dw must fit 1024 entries
    assert not gr.sam_supported(1, 16, 24, 2, torch.bfloat16) and not gr.sam_supported(1, 16, 96, 2, torch.bfloat16)
    assert not gr.sam_supported(1, 16, 124, 2, F32)                                                                  # CV = 31
    assert gr.sam_supported(1, 16, 8, 32, torch.bfloat16) and not gr.sam_supported(1, 16, 8, 33, torch.bfloat16)     # 800 entries; R > 32
    assert gr.sam_supported(1, 16, 16, 20, torch.bfloat16) and not gr.sam_supported(1, 16, 16, 21, torch.bfloat16)   # 980 / 1029 entries
    assert gr.sam_supported(1, 16, 128, 2, torch.bfloat16) and not gr.sam_supported(1, 16, 128, 3, torch.bfloat16)   # 770 / 1155


# ---------------------------------------------------------------------------------------------- PReLU
@pytest.mark.parametrize("dtype", HALVES, ids=str)
@pytest.mark.parametrize("nv", list(gr.PRELU_CASES))
def test_prelu_emulation_and_mutations(nv, dtype):
    n = nv * gr.vec(dtype)
    x, g = gr.prelu_inputs(n, dtype, seed=nv % 97)
    tag = f"prelu {SHORT[dtype]} n={n}"
    for slope in gr.PRELU_SLOPES:
        r = gr.prelu_ref(x, g, slope, 0.75, dtype)
        terms = {"y": (r.y, r.y_err, dtype), "dx": (r.dx, r.dx_err, dtype),
                 "da": (r.da.reshape(1), r.da_err.reshape(1), F32)}
        e = gr.prelu_emulate(x, g, slope, 0.75, dtype)
        for k in terms:
            _stage(k, getattr(e, k).reshape(terms[k][0].shape), terms[k], "prelu " + k, tag)
        if n >= 64:
            _sharp(*terms["da"], tag + " da")
        for mut in gr.PRELU_MUTATIONS:
            if mut == "slope_bf16" and (slope != gr.PRELU_SLOPES[1] or n < 64):
                continue                                     # a representable slope; one chunk: too few elements to cross a rounding for certain
            m = gr.prelu_emulate(x, g, slope, 0.75, dtype, mutate=mut)
            hit = _caught(terms, lambda k: getattr(m, k).reshape(terms[k][0].shape), terms)
            want = {"slope_bf16": {"y", "dx"}, "da_last_chunk": {"da"}}[mut]
            if mut == "da_last_chunk" and not bool((x[-gr.vec(dtype):].to(F64) <= 0).any()):
                continue                                     # the last chunk holds no term of the sum
            assert want & set(hit), f"{tag} slope {slope}: mutation {mut} was not caught"
            print(f"{tag} slope {slope}: {mut} caught at {hit}")


def test_prelu_specials_follow_fp64():
    for dtype in HALVES:
        n = (256 * 3 + 77) * 8
        x, g = gr.prelu_inputs(n, dtype, specials=True)
        r = gr.prelu_ref(x, g, 0.25, 0.0, dtype)
        assert bool(torch.isnan(r.y[50])) and bool(torch.isnan(r.da)) and float(r.dx[50]) == 0.25 * float(g[50])
        assert float(r.y[33]) == float("inf") and float(r.y[41]) == float("-inf") and int(torch.isnan(r.y).sum()) == 1
        r0 = gr.prelu_ref(x, g, 0.0, 0.0, dtype)
        assert bool(torch.isnan(r0.y[41]))                   # 0 * -inf, as torch gives


# ---------------------------------------------------------------------------------------------- CA gate
def _ca_terms(inp, dtype, E, rows):
    res, x, g, w1, w2 = inp
    T = gr.ca_fwd_terms(res, x, w1, w2, dtype, E)
    T.update(gr.ca_bwd_terms(g, res, w1, w2, dtype, E, rows=rows))
    return T


@pytest.mark.parametrize("dtype", HALVES + [F32], ids=str)
def test_ca_gate_emulation_and_mutations(dtype):
    for case in gr.ca_cases(dtype):
        for rows in ((False, True) if case in gr.CA_ROWS else (False,)):
            inp = gr.ca_inputs(*case, dtype)
            E = gr.ca_emulate(*inp, dtype, rows=rows)
            assert bool(((E.hidden > 0).any(1) & ((E.hidden == 0).any(1) | (case[3] == 1))).all()), f"{case}: dead and live hidden units"
            T = _ca_terms(inp, dtype, E, rows)
            tag = f"ca {SHORT[dtype]} {case}{' rows' if rows else ''}"
            for k in T:
                _stage(k, getattr(E, k), T[k], "ca " + k, tag, sharp=True)
            for mut in gr.CA_MUTATIONS:
                if not gr.ca_applicable(mut, case, dtype):
                    continue
                M = gr.ca_emulate(*inp, dtype, mutate=mut, rows=rows)
                hit = _caught(T, lambda k: getattr(M, k), _ca_terms(inp, dtype, M, rows))
                assert hit, f"{tag}: mutation {mut} was not caught"
                print(f"{tag}: {mut} caught at {hit}")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("dtype", HALVES, ids=str)
def test_ca_gate_fmaxf_relu_on_a_nan_mean_falls_outside(dtype, bad):
    """what the kernels did before the fix: hidden = fmaxf(NaN, 0) = 0 leaves a finite gate; the reference keeps the NaN"""
    case = (2, 130, 32, 32)
    res, x, g, w1, w2 = gr.ca_inputs(*case, dtype)
    res[1, 17, 5] = bad
    if bad == float("inf"):
        res[1, 17, 6] = bad      # two infinite channel means: in the rows of w1 that weigh them with opposite signs the products give NaN
        assert bool(((w1[:, 5] > 0) != (w1[:, 6] > 0)).any())
    inp = (res, x, g, w1, w2)
    E = gr.ca_emulate(*inp, dtype)
    T = _ca_terms(inp, dtype, E, False)
    for k in T:
        _stage(k, getattr(E, k), T[k], "ca nan " + k, f"ca {bad}")
    assert bool(torch.isnan(E.out[1]).all()) and bool(torch.isfinite(E.out[0]).all()) and bool(torch.isnan(E.dw2).all())
    M = gr.ca_emulate(*inp, dtype, mutate="fmax_relu")
    hit = _caught(T, lambda k: getattr(M, k), _ca_terms(inp, dtype, M, False))
    assert "hidden" in hit, hit
    if bad != bad:
        assert int(torch.isnan(M.out[1]).sum()) == 1         # the sample the module makes NaN came out finite but for the element itself
    print(f"ca {SHORT[dtype]} {bad}: fmax_relu caught at {hit}")


def test_ca_gate_saturating_weights_give_a_gate_of_0_or_1_and_never_nan():
    case = (2, 130, 32, 32)
    inp = gr.ca_inputs(*case, torch.bfloat16, saturate=True)
    E = gr.ca_emulate(*inp, torch.bfloat16)
    a = E.hidden @ inp[4].to(F64).T
    assert float(a.min()) < -60 and float(a.max()) > 60 and float(a.abs().max()) > 99
    T = _ca_terms(inp, torch.bfloat16, E, False)
    for k in T:
        _stage(k, getattr(E, k), T[k], "ca sat " + k, "ca saturating")
    lo, hi = nm.bracket(*T["gate"])
    assert not bool(torch.isnan(lo).any()) and bool((lo[a < -90] <= 0).all()) and bool((hi[a < -90] < 1e-37).all())
    assert bool((hi[a > 60] <= 1 + 2.0 ** -22).all()) and bool((lo[a > 60] >= 1 - 2.0 ** -22).all())


# ---------------------------------------------------------------------------------------------- SAM
def _sam_terms(inp, dtype, E):
    xh, xl, g, w1, w2, v1, v2 = inp
    T = gr.sam_fwd_terms(xh, xl, w1, w2, v1, v2, dtype, E)
    T.update(gr.sam_bwd_terms(g, xh, xl, w1, w2, v1, v2, dtype, E))
    return T


@pytest.mark.parametrize("dtype", HALVES + [F32], ids=str)
def test_sam_emulation_and_mutations(dtype):
    for case in gr.sam_cases(dtype):
        inp = gr.sam_inputs(*case, dtype)
        E = gr.sam_emulate(*inp, dtype)
        for h in (E.hc, E.hw):
            assert bool(((h > 0).any(-1) & (h == 0).any(-1)).all()), f"{case}: dead and live hidden units"
        assert not torch.equal(E.hc[0] > 0, E.hc[1] > 0) or not torch.equal(E.hw[0] > 0, E.hw[1] > 0)     # wrong_mask is visible
        T = _sam_terms(inp, dtype, E)
        tag = f"sam {SHORT[dtype]} {case}"
        for k in T:
            _stage(k, getattr(E, k), T[k], "sam " + k, tag, sharp=True)
        for mut in gr.SAM_MUTATIONS:
            if not gr.sam_applicable(mut, case, dtype):
                continue
            M = gr.sam_emulate(*inp, dtype, mutate=mut)
            hit = _caught(T, lambda k: getattr(M, k), _sam_terms(inp, dtype, M))
            assert hit, f"{tag}: mutation {mut} was not caught"
            print(f"{tag}: {mut} caught at {hit}")


@pytest.mark.parametrize("dtype", HALVES, ids=str)
def test_sam_fmaxf_relu_on_a_nan_mean_falls_outside(dtype):
    case = (2, 256, 32, 2)
    inp = list(gr.sam_inputs(*case, dtype))
    inp[0][1, 17, 5] = float("nan")
    E = gr.sam_emulate(*inp, dtype)
    T = _sam_terms(inp, dtype, E)
    for k in T:
        _stage(k, getattr(E, k), T[k], "sam nan " + k, "sam nan")
    assert bool(torch.isnan(E.out[1]).all()) and bool(torch.isfinite(E.out[0]).all())
    M = gr.sam_emulate(*inp, dtype, mutate="fmax_relu")
    hit = _caught(T, lambda k: getattr(M, k), _sam_terms(inp, dtype, M))
    assert "hc" in hit and "hw" in hit, hit
    print(f"sam {SHORT[dtype]} nan: fmax_relu caught at {hit}")


# ---------------------------------------------------------------------------------------------- bilinear
@pytest.mark.parametrize("align", [True, False], ids=["align", "half-pixel"])
@pytest.mark.parametrize("dtype", HALVES, ids=str)
def test_bilinear_emulation_and_mutations(dtype, align):
    V = gr.vec(dtype)
    for case in gr.BIL_CASES:
        Hi, Wi, Ho, Wo = case
        for C in ((V, 3 * V) if case == (7, 9, 19, 13) else (V,)):
            x, dy = gr.bil_inputs(2, Hi, Wi, C, dtype), gr.bil_inputs(2, Ho, Wo, C, dtype, seed=1)
            tag = f"bilinear {SHORT[dtype]} {case} C={C} align={align}"
            fr, fe = gr.bil_fwd_terms(x, Ho, Wo, align, dtype)
            br, be = gr.bil_bwd_terms(dy, Hi, Wi, align, dtype)
            T = {"fwd": (fr, fe, dtype), "bwd": (br, be, dtype)}
            E = {"fwd": gr.bil_emulate_fwd(x, Ho, Wo, align, dtype), "bwd": gr.bil_emulate_bwd(dy, Hi, Wi, align, dtype)}
            for k in T:
                _stage(k, E[k], T[k], "bilinear " + k, tag, sharp=True)
            if case == (16, 16, 16, 16):
                assert torch.equal(E["fwd"], x.to(F64)) and torch.equal(E["bwd"], dy.to(F64))
            for mut in gr.BIL_MUTATIONS:
                if not gr.bil_applicable(mut, case, align, dtype):
                    continue
                M = {"bwd": gr.bil_emulate_bwd(dy, Hi, Wi, align, dtype, mutate=mut)}
                if mut in ("no_neg_clamp", "swap_align", "lambda16"):
                    M["fwd"] = gr.bil_emulate_fwd(x, Ho, Wo, align, dtype, mutate=mut)
                hit = _caught(M, lambda k: M[k], T)
                assert hit, f"{tag}: mutation {mut} was not caught"
                print(f"{tag}: {mut} caught at {hit}")


def test_bilinear_every_mutation_applies_somewhere():
    for mut in gr.BIL_MUTATIONS:
        assert any(gr.bil_applicable(mut, c, al, torch.float16) for c in gr.BIL_CASES for al in (True, False)), mut


@pytest.mark.parametrize("which", list(gr.BIL_BIG))
def test_bilinear_grid_stride_references_are_sharp(which):
    """the inputs of the three grid-stride shapes give sharp brackets and few ties on the reference alone (fp16: the finer grid)"""
    B, Hi, Wi, Ho, Wo, C = gr.BIL_BIG[which]
    C = 8                                                    # one chunk of channels shows the same statistics
    dtype = torch.float16
    if which == "fwd":
        ref, err = gr.bil_fwd_terms(gr.bil_inputs(B, Hi, Wi, C, dtype), Ho, Wo, True, dtype)
    else:
        ref, err = gr.bil_bwd_terms(gr.bil_inputs(B, Ho, Wo, C, dtype, seed=1), Hi, Wi, True, dtype)
    # backward, fp16: the fp32 index at source index 263 is by itself an eighth of an fp16 ulp; these two are held to bf16 resolution
    frac, ties = gr.sharpness(ref, err, dtype)
    print(f"{which}: at fp16 resolution sharp {frac:.3f}, ties {ties:.3f}")
    if which == "fwd":
        assert frac >= 0.9 and ties < 0.25
    else:
        assert 0.75 < frac < 0.9                              # if this ever holds at fp16 resolution, demand it in the GPU file
        frac, ties = gr.sharpness(ref, err, torch.bfloat16)
        assert frac >= 0.9 and ties < 0.25
