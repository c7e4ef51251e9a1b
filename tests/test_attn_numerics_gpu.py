"""GPU: the spatial-reduction attention kernels (csrc/attn_fwd.hip, csrc/attn_bwd.hip) in bf16, fp16 and fp32 against the fp64
reference and the error model of tests/_attn_ref.py (what that model can see is shown by mutation in test_attn_numerics_cpu.py).

Every case calls dgtd_sra_attn_fwd / _bwd / _bwd_workspace through the C ABI.  Inputs are 16-byte aligned views at a non-zero offset
inside NaN-filled buffers; out, lse and dq are pre-filled with NaN, dkv with NaN for the 16-bit types (which must overwrite every
element) and with zeros for fp32 (which accumulates with atomics); the workspace has exactly the reported size, is pre-filled with 0xFF
bytes (NaN as fp32) and is followed by sentinel bytes that must survive.  out, lse, delta (the head of the workspace), dq and dkv must
lie in their brackets, all guards must be intact, the dispatch must be the one the case was chosen for, and a second launch must give
identical bits for everything except the fp32 dq / dkv (LDS and global atomics)."""
import pytest
import torch

import _attn_ref as ar
from _kernel_check import DEV, Buf, _same_bits, check_bracketed

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
F32 = torch.float32
SCALE = 0.125
SENTINEL = 4096
SHORT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}

MARGINS = {}                # "<dtype> <output>" -> largest share of its error bound used (reported at the end of the module)


@pytest.fixture(scope="module", autouse=True)
def L():
    import dgtd
    lib = dgtd._lib
    lib.load()
    yield lib
    if MARGINS:
        print("\nattention: largest share of the error bound used, per dtype and output: "
              + ", ".join(f"{k} {v:.3f}" for k, v in sorted(MARGINS.items())))


def _launch(L, Q, KV, G, case, dtype):
    """forward + backward into fresh guarded buffers; returns the buffers and the workspace"""
    B, N, Nkv, heads = case
    C = heads * 64
    code, st = L.dtype_code(Q.t), torch.cuda.current_stream().cuda_stream
    ws_bytes = L.load().dgtd_sra_attn_bwd_workspace(B, N, heads)
    assert ws_bytes == (B * N * heads * 4 + 255) // 256 * 256 + (64 << 20)
    out, lse, dq = Buf((B, N, C), dtype), Buf((B, heads, N), F32), Buf((B, N, C), dtype)
    dkv = Buf((B, Nkv, 2 * C), F32)
    if dtype == F32:
        dkv.t.zero_()
    ws = torch.full((ws_bytes + SENTINEL,), 0xFF, dtype=torch.uint8, device=DEV)
    L.call("dgtd_sra_attn_fwd", Q.p, KV.p, out.p, lse.p, B, N, Nkv, heads, SCALE, code, st)
    L.call("dgtd_sra_attn_bwd", Q.p, KV.p, out.p, G.p, lse.p, dq.p, dkv.p, ws.data_ptr(), B, N, Nkv, heads, SCALE, code, st)
    return dict(out=out, lse=lse, dq=dq, dkv=dkv), ws, ws_bytes


def _run_case(L, case, dtype, q, kv, dout, tag):
    B, N, Nkv, heads = case
    assert ar.plan(*case, dtype) == ar.expected_plan(case, dtype), "the dispatch no longer takes this case where it was meant to go"
    Q, KV, G = Buf(q.shape, dtype, q), Buf(kv.shape, dtype, kv), Buf(dout.shape, dtype, dout)
    runs = [_launch(L, Q, KV, G, case, dtype) for _ in range(2)]
    torch.cuda.synchronize()
    got = []
    for bufs, ws, ws_bytes in runs:
        for name, b in bufs.items():
            b.guards_intact(f"{tag} {name}")
        assert bool((ws[ws_bytes:] == 0xFF).all()), f"{tag}: the backward wrote past dgtd_sra_attn_bwd_workspace bytes"
        delta = ws[:B * heads * N * 4].view(F32).view(B, heads, N)
        got.append(dict(out=bufs["out"].t, lse=bufs["lse"].t, delta=delta, dq=bufs["dq"].t, dkv=bufs["dkv"].t))
    for t in (Q, KV, G):
        t.guards_intact(f"{tag} inputs")
    for name in ("out", "lse", "delta") + (() if dtype == F32 else ("dq", "dkv")):
        _same_bits(got[0][name], got[1][name], f"{tag} {name}")
    g = got[0]
    r = ar.reference(Q.t, KV.t, G.t, heads, SCALE, out_stored=g["out"])
    err, ref, gh = ar.bounds(Q.t, KV.t, G.t, heads, SCALE, dtype, r), ar.ref_of(r), ar.heads_of(g, heads)
    shares = {}
    for name in ar.OUTPUTS:
        od = ar.out_dtype(name, dtype)
        shares[name] = check_bracketed(gh[name].to(od), ref[name], err[name], od, f"{tag} {name}", f"{SHORT[dtype]} {name}", MARGINS)
    print(f"\n{tag}: share of each bound used: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    return g, r


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", list(ar.CASES), ids=[str(c) for c in ar.CASES])
def test_attention_vs_fp64(L, case, dtype):
    q, kv, dout = ar.make_inputs(*case, dtype, "standard", seed=1, device=DEV)
    _run_case(L, case, dtype, q, kv, dout, f"{SHORT[dtype]} {case}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("family", ["sharp", "spiked"])
@pytest.mark.parametrize("case", ar.SHARP_CASES, ids=[str(c) for c in ar.SHARP_CASES])
def test_attention_peaked_rows_vs_fp64(L, case, family, dtype):
    """sharp: q * 4 (alpha << 1 between register units, rows with P ~ 1); spiked: one key of the last chunk dominates one query row
    (the running-max rescale across chunks), through the backward too"""
    q, kv, dout = ar.make_inputs(*case, dtype, family, seed=2, device=DEV)
    g, r = _run_case(L, case, dtype, q, kv, dout, f"{SHORT[dtype]} {case} {family}")
    if family == "spiked":
        row, key = min(7, case[1] - 1), case[2] - 1 - min(3, case[2] - 1)
        assert r.P[0, 0, row, key] > 0.9                        # the spike is one


SPECIAL_CASES = [(2, 100, 37, 2), (2, 160, 300, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("kind", ["nan-query-row", "nan-v-element", "nan-key-row"])
@pytest.mark.parametrize("case", SPECIAL_CASES, ids=[str(c) for c in SPECIAL_CASES])
def test_attention_nan_goes_where_fp64_puts_it(L, case, kind, dtype):
    """forward and backward outputs are NaN exactly where the fp64 reference is NaN (assert_bracketed demands both directions), and
    bracketed elsewhere: a NaN query row poisons its own out / lse / delta / dq row and dK / dV of its batch element; a NaN element of V
    poisons one out column, delta, dQ and dK of its (batch, head) but not dV; a NaN key row poisons its whole (batch, head)."""
    B, N, Nkv, heads = case
    C = heads * 64
    q, kv, dout = ar.make_inputs(*case, dtype, "standard", seed=3, device=DEV)
    if kind == "nan-query-row":
        q[0, 5, :] = float("nan")
    elif kind == "nan-v-element":
        kv[1, 3, C + 70] = float("nan")                        # V of head 1, channel 6
    else:
        kv[0, Nkv - 2, 64:128] = float("nan")                  # K of head 1, a key of the ragged last tile
    g, r = _run_case(L, case, dtype, q, kv, dout, f"{SHORT[dtype]} {case} {kind}")
    nan_out = torch.isnan(ar.to_heads(g["out"], heads))
    if kind == "nan-query-row":
        assert bool(nan_out[0, :, 5].all()) and int(nan_out.sum()) == C
    elif kind == "nan-v-element":
        assert bool(nan_out[1, 1, :, 6].all()) and int(nan_out.sum()) == N
        dk, dv = ar.kv_to_heads(g["dkv"], heads)
        assert bool(torch.isnan(dk[1, 1]).all()) and not bool(torch.isnan(dv).any())
    else:
        assert bool(nan_out[0, 1].all()) and int(nan_out.sum()) == N * 64


@pytest.mark.parametrize("scale", [0.0, -0.125, float("nan"), float("inf")])
def test_attention_entries_refuse_a_non_positive_scale(L, scale):
    """the 16-bit forward takes the row maximum before scaling (right for scale > 0 only) and the fp32 one scales first: both C entries
    refuse a scale that is not finite and > 0 before any launch (the outputs stay NaN), for every dtype"""
    B, N, Nkv, heads = 1, 32, 32, 1
    for dtype in DTYPES:
        q, kv, dout = ar.make_inputs(B, N, Nkv, heads, dtype, device=DEV)
        code, st = L.dtype_code(q), torch.cuda.current_stream().cuda_stream
        out, lse, dq, dkv = Buf((B, N, 64), dtype), Buf((B, heads, N), F32), Buf((B, N, 64), dtype), Buf((B, Nkv, 128), F32)
        ws = torch.empty(L.load().dgtd_sra_attn_bwd_workspace(B, N, heads), dtype=torch.uint8, device=DEV)
        with pytest.raises(L.DgtdError, match="scale"):
            L.call("dgtd_sra_attn_fwd", q.data_ptr(), kv.data_ptr(), out.p, lse.p, B, N, Nkv, heads, scale, code, st)
        with pytest.raises(L.DgtdError, match="scale"):
            L.call("dgtd_sra_attn_bwd", q.data_ptr(), kv.data_ptr(), q.data_ptr(), dout.data_ptr(), lse.p, dq.p, dkv.p, ws.data_ptr(),
                   B, N, Nkv, heads, scale, code, st)
        torch.cuda.synchronize()
        for b in (out, lse, dq, dkv):
            assert bool(torch.isnan(b.t.float()).all())
