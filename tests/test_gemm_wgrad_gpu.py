"""GPU: the token-reducing weight-gradient GEMM (csrc/gemm_wgrad.hip, dgtd_gemm_wgrad_batched) against fp64 at rounding-level bounds
(tests/_numerics.py, the protocol of test_kernel_numerics_gpu.py).

Reference = dy.double().T @ x.double() from the exact 16-bit operands.  The kernel accumulates each token chunk (at most 4096 tokens) in
fp32 on the MFMA, sums the S chunk partials in fp32 and rounds once, so

    err = (C_MFMA + S_max * U32) * (|dy|^T |x|)

with C_MFMA = 2^-21 (fp32 accumulation of a 16-bit MFMA reduction of length <= 4096: cdna_hip_programming.md § "FP32-input MFMA"
measured 0.75-1.5e-7 * sum|a b| at K <= 1024 and 3.5e-7 at K = 4096 against fp64) and U32 = 2^-24 per fp32 addition of the second
stage; S_max is the chunk count the host logic picks, read back from dgtd_gemm_wgrad_workspace.  No constant is fitted to an observed
error.  Every output must lie in [round(ref - err), round(ref + err)] and at least 90 % of the brackets must be a single value.
Operands are 0.5 + 0.5 N(0,1) rounded to the dtype (little cancellation: the reference alone gives >= 0.996 single-valued brackets).
Outputs and workspace are pre-filled with NaN, all operands are aligned views at a non-zero offset inside NaN-filled buffers whose
guards must stay NaN, and a second launch must give the same bits.
"""
import math

import pytest
import torch

import _numerics as nm

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALVES = [torch.bfloat16, torch.float16]
F64 = torch.float64
U32 = 2.0 ** -24            # unit roundoff of one fp32 rounding to nearest
C_MFMA = 2.0 ** -21         # see the module docstring
KSTEP = 64                  # tokens per k-step of the kernel
MAX_CHUNK = 4096            # longest token chunk the host logic may choose (what C_MFMA is stated for)

MARGINS = {}


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


def _raw(name, *args):
    """the C entry's status, without raising"""
    import dgtd
    return int(getattr(dgtd._lib.load(), name)(*args))


class Buf:
    """`batch` entries of `shape`, `stride` elements apart, at a 16-byte aligned non-zero offset inside a NaN-filled buffer.  Everything
    that is not an entry (the pads on either side, the gaps between entries) is NaN and counts as guard."""

    def __init__(self, batch, shape, dtype, init=None, stride=None, pad=None):
        n = math.prod(shape)
        self.n, self.batch = n, batch
        self.stride = stride if stride is not None else n
        assert self.stride >= n and self.stride % 8 == 0
        self.pad = pad if pad is not None else 3 * shape[-1]
        assert self.pad % 8 == 0 and self.pad > 0
        self.flat = torch.full((batch * self.stride + 2 * self.pad,), float("nan"), dtype=dtype, device=DEV)
        self.slots = self.flat[self.pad:self.pad + batch * self.stride].view(batch, self.stride)
        self.t = self.slots[:, :n].view((batch,) + tuple(shape))          # a strided view: writes go to the entries only
        if init is not None:
            self.t.copy_(init)
        assert self.slots.data_ptr() % 16 == 0

    @property
    def p(self):
        return self.slots.data_ptr()

    def guards_intact(self, name):
        g = torch.cat([self.flat[:self.pad], self.slots[:, self.n:].reshape(-1), self.flat[self.pad + self.batch * self.stride:]])
        assert bool(torch.isnan(g.float()).all()), f"{name}: the kernel wrote outside its output"


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _check(got, ref, err, dtype, name, family):
    lo, hi = nm.bracket(ref, err, dtype)
    nm.assert_bracketed(got, lo, hi, name, ref=ref, err=err)
    frac = nm.assert_sharp(lo, hi, name=name)
    r = nm.ratio(got, ref, err)
    MARGINS[family] = max(MARGINS.get(family, 0.0), r)
    print(f"{name}: share of the bound used {r:.3f}, single-valued brackets {frac:.4f}")


def _operands(batch, M, N, K, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dy = (0.5 + 0.5 * torch.randn((batch, M, N), generator=g, device=DEV)).to(dt)
    x = (0.5 + 0.5 * torch.randn((batch, M, K), generator=g, device=DEV)).to(dt)
    return dy, x


def _chunks(batch, M, N, K):
    """S the host logic picks for this shape (dgtd_gemm_wgrad_workspace = batch * S * N * K * 4 bytes)"""
    ws = _raw("dgtd_gemm_wgrad_workspace", batch, M, N, K)
    assert ws > 0 and ws % (batch * N * K * 4) == 0, ws
    return ws // (batch * N * K * 4)


def _launch(DY, X, batch, M, N, K, dt, s_dw=None):
    """one launch into fresh NaN-filled output and workspace; returns (dw Buf, workspace tensor)"""
    S = _chunks(batch, M, N, K)
    DW = Buf(batch, (N, K), dt, stride=s_dw)
    ws = torch.full((batch * S * N * K + 8,), float("nan"), dtype=torch.float32, device=DEV)
    rc = _raw("dgtd_gemm_wgrad_batched", DY.p, X.p, DW.p, ws[4:].data_ptr(), batch, M, N, K, DY.stride, X.stride, DW.stride, _code(dt), _st())
    assert rc == 0, rc
    return DW, ws


def _run_case(batch, M, N, K, dt, strides=None, min_chunks=1, seed=11):
    tag = f"wgrad b={batch} M={M} N={N} K={K} {str(dt)[6:]}" + (" strided" if strides else "")
    assert _raw("dgtd_gemm_wgrad_supported", M, N, K, _code(dt)) == 1, tag
    S = _chunks(batch, M, N, K)
    assert S >= min_chunks, (tag, S)
    assert math.ceil(M / S / KSTEP) * KSTEP <= MAX_CHUNK, f"{tag}: {S} chunks leave a chunk longer than {MAX_CHUNK} tokens"
    dy, x = _operands(batch, M, N, K, dt, seed)
    s_dy, s_x, s_dw = strides if strides else (None, None, None)
    DY, X = Buf(batch, (M, N), dt, dy, stride=s_dy), Buf(batch, (M, K), dt, x, stride=s_x)
    dy64, x64 = DY.t.to(F64), X.t.to(F64)
    ref = dy64.transpose(1, 2) @ x64
    err = (C_MFMA + S * U32) * (dy64.abs().transpose(1, 2) @ x64.abs())

    first, ws1 = _launch(DY, X, batch, M, N, K, dt, s_dw)
    second, _ = _launch(DY, X, batch, M, N, K, dt, s_dw)
    torch.cuda.synchronize()
    first.guards_intact(tag)
    assert bool(torch.isnan(ws1[:4]).all()) and bool(torch.isnan(ws1[-4:]).all()), f"{tag}: the kernel wrote outside its workspace"
    if S > 1:
        assert not bool(torch.isnan(ws1[4:-4]).any()), f"{tag}: a partial tile of the workspace was never written"
    assert torch.equal(_bits(first.t), _bits(second.t)), f"{tag}: a second launch on the same inputs gave different bits"
    _check(first.t, ref, err, dt, f"{tag} S={S}", "gemm_wgrad")


CASES = [  # batch, M, N, K, fewest chunks the host logic must pick here
    (1, 64, 64, 64, 1),          # one k-step, one tile
    (1, 192, 128, 64, 1),        # an odd number of k-steps: pipeline prologue and tail
    (1, 1024, 320, 128, 2),      # five 64-wide row tiles (N % 128 != 0) x one 128-wide column tile, two chunks
    (1, 1024, 128, 320, 2),      # the N <-> K twin: an asymmetry between the two operands shows
    (1, 1088, 64, 64, 3),        # 17 k-steps: the last chunk is shorter than the others
    (3, 256, 64, 192, 1),        # batch, dense strides
    (2, 8192, 128, 128, 2),      # the 4096-token cap forces at least two chunks per entry
]


@pytest.mark.parametrize("dt", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("batch,M,N,K,min_chunks", CASES)
def test_wgrad_against_fp64(batch, M, N, K, min_chunks, dt):
    _run_case(batch, M, N, K, dt, min_chunks=min_chunks)


@pytest.mark.parametrize("dt", HALVES, ids=["bf16", "fp16"])
def test_wgrad_strides_larger_than_dense(dt):
    """all three tensors with gaps between the entries: the gaps of dw stay NaN, the NaN gaps of dy and x reach no output"""
    batch, M, N, K = 3, 256, 128, 128
    _run_case(batch, M, N, K, dt, strides=(M * N + 64, M * K + 128, N * K + 24))


@pytest.mark.parametrize("dt", HALVES, ids=["bf16", "fp16"])
def test_wgrad_single_chunk_stores_directly(dt):
    """a shape with one chunk needs no workspace at all (NULL is accepted) and must not touch one that is passed"""
    batch, M, N, K = 1, 192, 128, 64
    assert _chunks(batch, M, N, K) == 1
    dy, x = _operands(batch, M, N, K, dt, 5)
    DY, X = Buf(batch, (M, N), dt, dy), Buf(batch, (M, K), dt, x)
    a, ws = _launch(DY, X, batch, M, N, K, dt)
    b = Buf(batch, (N, K), dt)
    assert _raw("dgtd_gemm_wgrad_batched", DY.p, X.p, b.p, None, batch, M, N, K, 0, 0, 0, _code(dt), _st()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all()), "a single-chunk launch wrote into the workspace"
    assert torch.equal(_bits(a.t), _bits(b.t))


def test_wgrad_refusals_do_not_launch():
    import dgtd
    L = dgtd._lib.load()
    dt = torch.bfloat16
    code, st = _code(dt), _st()
    assert _raw("dgtd_gemm_wgrad_supported", 96, 64, 64, code) == 0          # M no multiple of the k-step
    assert _raw("dgtd_gemm_wgrad_supported", 64, 96, 64, code) == 0          # N % 64
    assert _raw("dgtd_gemm_wgrad_supported", 64, 64, 96, code) == 0          # K % 64
    assert _raw("dgtd_gemm_wgrad_supported", 64, 64, 64, _code(torch.float32)) == 0
    assert _raw("dgtd_gemm_wgrad_supported", 1 << 22, 1024, 64, code) == 0   # M * N = 2^32 elements
    assert _raw("dgtd_gemm_wgrad_supported", 64, 64, 64, code) == 1

    M, N, K = 128, 128, 128
    dy, x = _operands(2, M, N, K, dt, 3)
    DY, X = Buf(2, (M, N), dt, dy), Buf(2, (M, K), dt, x)
    DY96, X96 = Buf(1, (96, N), dt, dy[:1, :96]), Buf(1, (96, K), dt, x[:1, :96])
    DYn, Xf = Buf(1, (M, 96), dt, dy[:1, :, :96]), Buf(1, (M, K), torch.float32, x[:1].float())
    DYf = Buf(1, (M, N), torch.float32, dy[:1].float())
    outs = []

    def refused(what, dyp, xp, batch, m, n, k, s_dw=None, odt=dt, dw_shift=0, cd=code):
        DW = Buf(batch, (n, k), odt, stride=s_dw if s_dw and s_dw >= n * k else None)
        ws = torch.full((batch * 64 * n * k // 16 + 8,), float("nan"), dtype=torch.float32, device=DEV)
        rc = _raw("dgtd_gemm_wgrad_batched", dyp, xp, DW.p + dw_shift, ws.data_ptr(), batch, m, n, k, m * n, m * k,
                  s_dw if s_dw is not None else n * k, cd, st)
        assert rc != 0, f"{what}: accepted"
        assert L.dgtd_last_error(), what
        outs.append((what, DW, ws))

    refused("M = 96", DY96.p, X96.p, 1, 96, N, K)
    refused("N = 96", DYn.p, X.p, 1, M, 96, K)
    refused("fp32", DYf.p, Xf.p, 1, M, N, K, odt=torch.float32, cd=_code(torch.float32))
    refused("mis-aligned dw", DY.p, X.p, 1, M, N, K, dw_shift=2)
    refused("s_dw < N K with batch = 2", DY.p, X.p, 2, M, N, K, s_dw=N * K - 8)
    assert _raw("dgtd_gemm_wgrad_batched", None, X.p, outs[0][1].p, None, 1, M, N, K, 0, 0, 0, code, st) != 0   # null operand
    torch.cuda.synchronize()
    for what, DW, ws in outs:
        assert bool(torch.isnan(DW.flat.float()).all()) and bool(torch.isnan(ws).all()), f"{what}: refused, but something was launched"


@pytest.mark.parametrize("dt", HALVES, ids=["bf16", "fp16"])
def test_wgrad_nan_reaches_exactly_its_columns(dt):
    """a NaN in one token row of x poisons all N rows of dw in exactly the K columns where x is NaN (two chunks: through the reduce)"""
    batch, M, N, K = 1, 1024, 128, 128
    assert _chunks(batch, M, N, K) >= 2
    dy, x = _operands(batch, M, N, K, dt, 9)
    cols = torch.tensor([0, 7, 31, 32, 63, 64, 100, 127], device=DEV)
    x[0, 700, cols] = float("nan")
    DY, X = Buf(batch, (M, N), dt, dy), Buf(batch, (M, K), dt, x)
    DW, _ = _launch(DY, X, batch, M, N, K, dt)
    torch.cuda.synchronize()
    want = torch.zeros((1, N, K), dtype=torch.bool, device=DEV)
    want[:, :, cols] = True
    assert torch.equal(torch.isnan(DW.t.float()), want)
    DW.guards_intact("nan case")
