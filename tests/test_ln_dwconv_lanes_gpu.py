"""GPU: LayerNorm (csrc/layernorm.hip) and the LDS-tiled depthwise 7x7 (csrc/dwconv_tiled.hip) through the C ABI, at the shapes
where their lane mapping can go wrong.

LayerNorm reduces a row inside a power-of-two group of G lanes with DPP / permlane steps (common.h, group_sum<G>): a wrong lane
pairing at any G gives a wrong mean.  The channel counts below cover every G (1 .. 64), rows that leave lanes of a group idle
(C = 24, 320), and 2 and 4 chunks per lane; the row counts cover a single row, fewer rows than one wave holds, a ragged last
workgroup and more than one workgroup.  The depthwise shapes cover one tile with three idle waves (1x1), exact tiles, ragged tiles
in both directions and more than one tile per image, for all four epilogue modes.

All tensors are 16-byte aligned views inside NaN-filled buffers (a read outside an input poisons the result, a write outside an
output breaks a guard), and every launch is repeated into fresh buffers and must give the same bits."""
import ctypes as C
import math

import pytest
import torch

from _kernel_check import DEV, F64, Buf, _bits, _run_twice

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHORT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
F32 = torch.float32
EPS = 1e-6


@pytest.fixture(scope="module")
def L():
    import dgtd
    lib = dgtd._lib
    lib.load()
    return lib


def _rand(*shape, seed, dtype=F32, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


class ReduceEntry(C.Structure):
    """dgtd_reduce_entry of include/dgtd.h"""
    _fields_ = [("ws", C.c_void_p), ("nblocks", C.c_int32), ("ncols", C.c_int32), ("outA", C.c_void_p), ("nA", C.c_int32),
                ("outB", C.c_void_p), ("dtB", C.c_int32), ("tr_rows", C.c_int32), ("tr_cols", C.c_int32), ("outC", C.c_void_p)]


# ---------------------------------------------------------------------------------------------- LayerNorm
LN_CASES = [(c, dt) for dt in DTYPES for c in (8, 24, 64, 128, 256, 320, 512, 1024)] + [(2048, torch.bfloat16), (2048, torch.float16)]
LN_ROWS = (1, 3, 130, 777)


def _ln_geometry(C_, dtype):
    """(rows per lane-group step, rows per workgroup trip) of the kernels' mapping: 16-byte chunks, G = the power of two >= chunks per
    row (at most 64) lanes per row, 4 waves, U rows in flight per group."""
    cpr = C_ // (4 if dtype == F32 else 8)
    G = 1
    while G < cpr and G < 64:
        G *= 2
    npl = -(-cpr // G)
    rpb = (64 // G) * 4
    return rpb, rpb * (4 if npl <= 2 else 2)


def _ln_ref(x, w, b, dy, dres):
    """fp64 LayerNorm forward and backward from the rounded inputs"""
    x, w, b, dy = x.to(F64), w.to(F64), b.to(F64), dy.to(F64)
    mu = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + EPS)
    xh = (x - mu) * rs
    g = dy * w
    dx = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return {"y": xh * w + b, "mean": mu[:, 0], "rstd": rs[:, 0], "dx": dx, "dx_add": dx + dres.to(F64),
            "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0)}


def _ln_fwd(L, x, w, b, rows, C_, name):
    def fn(o):
        L.call("dgtd_layernorm_fwd", x.p, w.p, b.p, o[0].p, o[1].p, o[2].p, rows, C_, EPS, L.dtype_code(x.t), L.stream_ptr())
    return _run_twice(fn, [((rows, C_), x.t.dtype), ((rows,), F32), ((rows,), F32)], name)


def _ln_bwd(L, dy, x, w, mean, rstd, dres, rows, C_, ws, name, partial=False):
    dt = L.dtype_code(x.t)

    def fn(o):
        if partial:
            nb = C.c_int(0)
            L.call("dgtd_layernorm_bwd_partial", dy.p, x.p, w.p, mean.p, rstd.p, dres.p if dres else None, o[0].p, ws.data_ptr(), rows, C_, dt,
                   C.byref(nb), L.stream_ptr())
            assert 0 < nb.value * 2 * C_ * 4 <= ws.numel(), "partial rows must fit dgtd_layernorm_bwd_workspace"
            e = ReduceEntry(ws.data_ptr(), nb.value, 2 * C_, o[1].p, C_, o[2].p, 0, 0, 0, None)     # dtB 0 = DGTD_F32
            L.call("dgtd_multi_reduce", C.addressof(e), 1, L.stream_ptr())
        elif dres:
            L.call("dgtd_layernorm_bwd_add", dy.p, x.p, w.p, mean.p, rstd.p, dres.p, o[0].p, o[1].p, o[2].p, ws.data_ptr(), rows, C_, dt,
                   L.stream_ptr())
        else:
            L.call("dgtd_layernorm_bwd", dy.p, x.p, w.p, mean.p, rstd.p, o[0].p, o[1].p, o[2].p, ws.data_ptr(), rows, C_, dt, L.stream_ptr())
    return _run_twice(fn, [((rows, C_), x.t.dtype), ((C_,), F32), ((C_,), F32)], name)


def _as_buf(t):
    return Buf(tuple(t.shape), t.dtype, init=t)


@pytest.mark.parametrize("C_,dtype", LN_CASES, ids=[f"C{c}-{SHORT[d]}" for c, d in LN_CASES])
def test_layernorm_lane_groups(L, C_, dtype):
    """(a) forward, backward and backward-with-residual against fp64 at the tolerances of test_ops_gpu.test_layernorm_fwd_bwd;
    (b) a row of a 777-row launch has the bits of a one-row launch of that row (first row, last row, a row at a workgroup boundary);
    (c) dgtd_layernorm_bwd_partial + dgtd_multi_reduce give the bits of dgtd_layernorm_bwd."""
    assert L.F32 == 0
    tol = 2e-5 if dtype == F32 else 3e-2
    gtol = 2e-4 if dtype == F32 else 5e-2
    ws = torch.full((int(L.load().dgtd_layernorm_bwd_workspace(C_)),), 0xFF, dtype=torch.uint8, device=DEV)     # NaN as fp32
    w, b = Buf((C_,), F32, init=1 + 0.1 * _rand(C_, seed=1)), Buf((C_,), F32, init=0.1 * _rand(C_, seed=2))
    for rows in LN_ROWS:
        tag = f"ln[C={C_},{SHORT[dtype]},rows={rows}]"
        x = Buf((rows, C_), dtype, init=_rand(rows, C_, seed=C_ + rows, dtype=dtype))
        dy = Buf((rows, C_), dtype, init=_rand(rows, C_, seed=3, dtype=dtype))
        dres = Buf((rows, C_), dtype, init=_rand(rows, C_, seed=4, dtype=dtype))
        ref = _ln_ref(x.t, w.t, b.t, dy.t, dres.t)
        y, mean, rstd = _ln_fwd(L, x, w, b, rows, C_, tag + ".fwd")
        torch.testing.assert_close(y.to(F64), ref["y"], atol=tol, rtol=tol, msg=lambda m: f"{tag} y: {m}")
        torch.testing.assert_close(mean.to(F64), ref["mean"], atol=2e-5, rtol=2e-5, msg=lambda m: f"{tag} mean: {m}")
        torch.testing.assert_close(rstd.to(F64), ref["rstd"], atol=2e-5, rtol=2e-5, msg=lambda m: f"{tag} rstd: {m}")
        mb, rb = _as_buf(mean), _as_buf(rstd)
        dx, dg, db = _ln_bwd(L, dy, x, w, mb, rb, None, rows, C_, ws, tag + ".bwd")
        dxa, dga, dba = _ln_bwd(L, dy, x, w, mb, rb, dres, rows, C_, ws, tag + ".bwd_add")
        torch.testing.assert_close(dx.to(F64), ref["dx"], atol=tol, rtol=tol, msg=lambda m: f"{tag} dx: {m}")
        torch.testing.assert_close(dxa.to(F64), ref["dx_add"], atol=tol, rtol=tol, msg=lambda m: f"{tag} dx (bwd_add): {m}")
        for got, name in ((dg, "dgamma"), (dga, "dgamma (bwd_add)")):
            torch.testing.assert_close(got.to(F64), ref["dgamma"], atol=gtol * math.sqrt(rows), rtol=gtol, msg=lambda m: f"{tag} {name}: {m}")
        for got, name in ((db, "dbeta"), (dba, "dbeta (bwd_add)")):
            torch.testing.assert_close(got.to(F64), ref["dbeta"], atol=gtol * math.sqrt(rows), rtol=gtol, msg=lambda m: f"{tag} {name}: {m}")
        # (c) the first stage alone + the shared second stage
        dxp, dgp, dbp = _ln_bwd(L, dy, x, w, mb, rb, None, rows, C_, ws, tag + ".bwd_partial", partial=True)
        for a, p, name in ((dx, dxp, "dx"), (dg, dgp, "dgamma"), (db, dbp, "dbeta")):
            assert torch.equal(_bits(a), _bits(p)), f"{tag} {name}: bwd_partial + multi_reduce differs from bwd"
        # (b) row independence
        if rows == LN_ROWS[-1]:
            rpb, trip = _ln_geometry(C_, dtype)
            boundary = trip if trip < rows else (rpb if rpb < rows else 64)
            for r in (0, rows - 1, boundary):
                x1, dy1 = _as_buf(x.t[r:r + 1]), _as_buf(dy.t[r:r + 1])
                y1, m1, r1 = _ln_fwd(L, x1, w, b, 1, C_, f"{tag}.fwd.row{r}")
                dx1, _, _ = _ln_bwd(L, dy1, x1, w, _as_buf(m1), _as_buf(r1), None, 1, C_, ws, f"{tag}.bwd.row{r}")
                for a, p, name in ((y[r:r + 1], y1, "y"), (mean[r:r + 1], m1, "mean"), (rstd[r:r + 1], r1, "rstd"), (dx[r:r + 1], dx1, "dx")):
                    assert torch.equal(_bits(a), _bits(p)), f"{tag} {name}: row {r} of the launch differs from a one-row launch of it"


# ---------------------------------------------------------------------------------------------- depthwise 7x7, LDS-tiled kernel
DW_C = (128, 256)
DW_HW = ((1, 1), (4, 16), (5, 17), (9, 40))
DW_B, DW_K = 2, 7
_DW_CACHE = {}


def _dw_case(C_, H, W, dtype):
    """inputs (as guarded buffers) and the fp64 pre-activation conv(x) + bias, computed once and shared by the four modes"""
    key = (C_, H, W, dtype)
    if key not in _DW_CACHE:
        x = _rand(DW_B, H, W, C_, seed=1, dtype=dtype)
        aux = _rand(DW_B, H, W, C_, seed=4, dtype=dtype)
        w = _rand(C_, 1, DW_K, DW_K, seed=2) / DW_K                          # Conv2d layout, fp32
        bias = 0.1 * _rand(C_, seed=3)
        conv = torch.nn.functional.conv2d(x.to(F64).cpu().permute(0, 3, 1, 2), w.to(F64).cpu(), None, padding=DW_K // 2, groups=C_)
        conv = conv.permute(0, 2, 3, 1).contiguous().to(DEV)
        wt = w.reshape(C_, DW_K * DW_K).t().contiguous()                      # [K*K, C]: tap rows contiguous in C
        _DW_CACHE[key] = {"x": _as_buf(x), "aux": _as_buf(aux), "wt": _as_buf(wt), "bias": _as_buf(bias), "conv": conv,
                          "pre": conv + bias.to(F64)}
    return _DW_CACHE[key]


def _dw_expected(pre, aux, mode):
    phi = 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    if mode == 0:
        return pre
    if mode == 1:
        return pre * phi
    if mode == 2:
        return aux.to(F64) * (phi + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi))
    return pre + aux.to(F64)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=[SHORT[d] for d in DTYPES])
def test_dwconv7_tiled_modes(L, dtype, mode):
    """dgtd_dwconv_fwd, K = 7, C % 128 == 0 (the LDS-tiled kernel), against an fp64 grouped conv2d + the mode's epilogue at the
    tolerances of the depthwise tests of test_ops_gpu.py (fp32 1e-4; 16-bit atol 3e-2, rtol 2e-2).  Mode 0 also runs without a bias."""
    atol, rtol = (1e-4, 1e-4) if dtype == F32 else (3e-2, 2e-2)
    for C_ in DW_C:
        for H, W in DW_HW:
            c = _dw_case(C_, H, W, dtype)
            tag = f"dwconv7[{DW_B}x{H}x{W}x{C_},{SHORT[dtype]},mode{mode}]"
            for bias in ((c["bias"], None) if mode == 0 else (c["bias"],)):
                def fn(o):
                    L.call("dgtd_dwconv_fwd", c["x"].p, c["wt"].p, bias.p if bias else None, c["aux"].p if mode >= 2 else None, o[0].p,
                           DW_B, H, W, C_, DW_K, mode, L.dtype_code(c["x"].t), L.stream_ptr())
                y, = _run_twice(fn, [((DW_B, H, W, C_), dtype)], tag)
                ref = _dw_expected(c["pre"] if bias else c["conv"], c["aux"].t, mode)
                torch.testing.assert_close(y.to(F64), ref, atol=atol, rtol=rtol, msg=lambda m: f"{tag}{'' if bias else ' no bias'}: {m}")
