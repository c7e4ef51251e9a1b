"""CPU: what the error model of the attention kernels (tests/_attn_ref.py) can and cannot see, shown by mutation.

A bound that contains the 16-bit rounding of P or dS is a few output ulps wide, so its brackets cannot be single-valued (the
sharpness test of the GEMM / conv bounds).  Instead, for every case of tests/test_attn_numerics_gpu.py and both 16-bit types:
  * an fp64 emulation of the arithmetic the kernels document lies inside every bracket (the bound is not too tight), and
  * each applicable mutation of that arithmetic - a bug of a kind these kernels can have - puts at least one element outside
    (the bound is not too loose).
The cases with many (batch, head) pairs are checked on one pair: every pair is an independent problem of the same size."""
import pytest
import torch

import _attn_ref as ar

HALVES = [torch.bfloat16, torch.float16]
SCALE = 0.125
CASE_IDS = [str(c) for c in ar.CASES]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=str)
@pytest.mark.parametrize("case", list(ar.CASES), ids=CASE_IDS)
def test_plan_matches_the_hand_read_dispatch(case, dtype):
    assert ar.plan(*case, dtype) == ar.expected_plan(case, dtype)


def test_sharp_cases_are_the_multi_unit_ones():
    assert len(ar.SHARP_CASES) == 5
    for c in ar.CASES:
        p = ar.plan(*c, torch.bfloat16)
        assert (sum(p[3]) > 1) == (c in ar.SHARP_CASES)


def _outside(case, sl, dtype, family, mutate):
    """{output: elements outside its bracket}, largest share of a bound used, for the (mutated) emulation on the slice `sl` of case"""
    B, N, Nkv, heads = sl
    q, kv, dout = ar.make_inputs(B, N, Nkv, heads, dtype, family, seed=1)
    got = ar.emulate(q, kv, dout, heads, SCALE, dtype, mutate)
    r = ar.reference(q, kv, dout, heads, SCALE, out_stored=got["out"])
    err = ar.bounds(q, kv, dout, heads, SCALE, dtype, r, launch=case)      # chain lengths of the FULL case: the slice only saves fp64 work
    gh, ref = ar.heads_of(got, heads), ar.ref_of(r)
    bad, share = {}, {}
    for name in ar.OUTPUTS:
        od = ar.out_dtype(name, dtype)
        g = gh[name].to(od)                     # exact: the emulation already holds values of that type
        bad[name] = ar.outside(g, ref[name], err[name], od)
        share[name] = ar.nm.ratio(g, ref[name], err[name])
    return bad, share


def _slice(case):
    B, N, Nkv, heads = case
    return case if B * heads <= 4 else (1, N, Nkv, 1)


@pytest.mark.parametrize("dtype", HALVES, ids=str)
@pytest.mark.parametrize("case", list(ar.CASES), ids=CASE_IDS)
def test_emulation_inside_and_every_mutation_outside(case, dtype):
    sl = _slice(case)
    bad, share = _outside(case, sl, dtype, "standard", None)
    print(f"\n{case} {dtype}: share of each bound the emulation uses: " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
    assert not any(bad.values()), f"the unmutated emulation leaves its brackets: {bad}"
    for mut in ar.MUTATIONS:
        if not ar.applicable(mut, case[2], dtype):
            continue
        bad, _ = _outside(case, sl, dtype, "standard", mut)
        print(f"  {mut}: outside " + ", ".join(f"{k} {v}" for k, v in bad.items() if v))
        assert any(bad.values()), f"mutation {mut} stays inside every bracket: the bounds cannot see it"


@pytest.mark.parametrize("dtype", HALVES, ids=str)
@pytest.mark.parametrize("family", ["sharp", "spiked"])
@pytest.mark.parametrize("case", ar.SHARP_CASES, ids=[str(c) for c in ar.SHARP_CASES])
def test_emulation_inside_other_families(case, family, dtype):
    bad, share = _outside(case, _slice(case), dtype, family, None)
    print(f"\n{case} {family} {dtype}: " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
    assert not any(bad.values()), bad


def test_emulate_unmutated_matches_reference_closely():
    """the emulation is the reference plus roundings: at fp32 'I/O' the two agree to 1e-6 relative"""
    q, kv, dout = ar.make_inputs(2, 100, 37, 2, torch.float32, seed=2)
    got = ar.heads_of(ar.emulate(q, kv, dout, 2, SCALE, torch.float32), 2)
    r = ar.ref_of(ar.reference(q, kv, dout, 2, SCALE))
    for k in ar.OUTPUTS:
        torch.testing.assert_close(got[k], r[k], rtol=1e-5, atol=1e-5)
