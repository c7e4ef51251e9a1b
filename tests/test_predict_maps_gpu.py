"""GPU: dgtd_predict_maps / ops.predict_maps (csrc/predict_maps.hip) against the float64 restatement of tests/_predict_ref.py.
Every pixel of every map is checked: outside the tie band (v + 0.5 within eps of an integer, eps derived in _predict_ref from the
fp32 error model) the byte must be exact, inside it one of the two neighbours; the tests assert that the band holds at most 5 % of
the pixels of their own inputs, so that a degenerate input cannot hide a wrong kernel."""
import numpy as np
import pytest
import torch

import _predict_ref as R

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
POISON = 0xA5
B = 3
BIDX = [2, 0, 1, 1, 0, 2, 2, 1]      # the eight target sizes read the three planes out of order, several jobs per plane


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def data():
    """{(S, dtype name): (logits [B,1,S,S] on the device, the same values as float64 numpy)}: computed once, never modified."""
    out = {}
    for S in (32, 64):
        x = torch.from_numpy(R.logits(B, S, seed=S))
        for name, dt in DTYPES.items():
            xd = x.to(dt)
            out[(S, name)] = (xd.reshape(B, 1, S, S).cuda(), xd.double().numpy())
    return out


def run(dgtd, logits, sizes, bidx=None, minmax=False):
    """(host bytes of the whole poisoned buffer, offsets, total): the op writes into a buffer pre-filled with POISON and 64 bytes longer
    than the layout."""
    offsets, total = dgtd._lib.predict_maps_layout(sizes)
    out = torch.full((total + 64,), POISON, dtype=torch.uint8, device="cuda")
    packed, offs = dgtd.ops.predict_maps(logits, sizes, bidx, minmax=minmax, out=out)
    assert packed is out and offs == offsets
    return out.cpu().numpy(), offsets, total


def check_maps(host, offsets, sizes, bidx, planes, minmax, min_range=None):
    covered = np.zeros(host.size, bool)
    for j, ((H, W), off) in enumerate(zip(sizes, offsets)):
        got = host[off:off + H * W].reshape(H, W)
        covered[off:off + H * W] = True
        plane = planes[bidx[j]]
        v, rng = R.levels(plane, H, W, minmax)
        if minmax:
            if rng == 0.0:                                       # a constant map: all 0
                assert not got.any(), (j, H, W)
                continue
            assert min_range is None or rng >= min_range, (j, H, W, rng)
            eps = R.eps_minmax(R.max_abs(plane), rng)
        else:
            eps = R.eps_plain(R.max_abs(plane))
        share = R.tie_share(v, eps)
        ok = R.accepts(got, v, eps)
        off_by = np.abs(got.astype(np.int64) - R.quantise(v).astype(np.int64)).max()
        print(f"job {j} {H}x{W} plane {bidx[j]} minmax={minmax}: eps {eps:.2e} tie share {share:.4f} rejected {int((~ok).sum())} max level diff {off_by}")
        if H * W >= 100:
            assert share <= 0.05, (j, H, W, share)               # the condition on the inputs
        assert ok.all(), (j, H, W, int((~ok).sum()))
        assert off_by <= 1
    assert (host[~covered] == POISON).all()                      # the alignment padding and the tail keep the poison


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("name", list(DTYPES))
def test_plain_maps_of_every_size(dgtd, data, S, name):
    logits, planes = data[(S, name)]
    sizes = R.target_sizes(S)
    host, offsets, total = run(dgtd, logits, sizes, BIDX)
    check_maps(host, offsets, sizes, BIDX, planes, minmax=False)
    # the identity job: the bytes are the quantised sigmoid of the source itself (no blend error at all)
    j = sizes.index((S, S))
    got = host[offsets[j]:offsets[j] + S * S].reshape(S, S)
    assert R.accepts(got, 255.0 * R.sigmoid(planes[BIDX[j]]), R.eps_plain(0.0)).all()


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("name", list(DTYPES))
def test_minmax_maps_with_different_ranges_in_one_launch(dgtd, data, S, name):
    """Plane 1 is scaled down so that its sigmoid range differs from the other planes': extrema leaking between the jobs of a launch
    would show in its bytes.  (1, 1) is a constant map."""
    logits, _ = data[(S, name)]
    logits = logits.clone()
    logits[1] = (logits[1].float() * 0.25).to(logits.dtype)
    planes = logits[:, 0].double().cpu().numpy()
    sizes = [(S, S), (33, 47), (1, 1), (17, 9), (5, 67), (300, 500), (33, 47)]
    bidx = [1, 0, 2, 1, 2, 1, 2]
    ranges = [R.levels(planes[b], h, w, True)[1] for (h, w), b in zip(sizes, bidx)]
    assert max(ranges) - min(r for r in ranges if r > 0) > 0.05   # the ranges do differ
    host, offsets, total = run(dgtd, logits, sizes, bidx, minmax=True)
    check_maps(host, offsets, sizes, bidx, planes, minmax=True, min_range=0.5)


def test_saturation_nan_and_constant_maps(dgtd):
    S = 32
    x = torch.from_numpy(R.logits(B, S, seed=7))
    x[0], x[1] = 40.0, -40.0
    x[2, 5, 9] = float("nan")
    planes = x.double().numpy()
    sizes, bidx = [(33, 47), (33, 47), (S, S), (33, 47)], [0, 1, 2, 2]
    host, offsets, total = run(dgtd, x.cuda(), sizes, bidx)
    m = lambda j: host[offsets[j]:offsets[j] + sizes[j][0] * sizes[j][1]].reshape(sizes[j])
    assert (m(0) == 255).all() and (m(1) == 0).all()             # logits of +-40: exactly 255 and 0
    assert m(2)[5, 9] == 0                                       # a NaN logit: 0
    check_maps(host, offsets, sizes, bidx, planes, minmax=False)  # and every other pixel as the restatement (0 * NaN = NaN there too)
    # min-max on constant maps: all 0
    host, offsets, total = run(dgtd, x.cuda(), [(33, 47), (S, S), (5, 67)], [0, 1, 1], minmax=True)
    for off, (h, w) in zip(offsets, [(33, 47), (S, S), (5, 67)]):
        assert not host[off:off + h * w].any()


@pytest.mark.parametrize("minmax", [False, True])
def test_two_calls_are_bit_identical(dgtd, data, minmax):
    logits, _ = data[(64, "bf16")]
    sizes = [(64, 64), (33, 47), (17, 9), (5, 67), (300, 500)]
    a = run(dgtd, logits, sizes, BIDX[:5], minmax)[0]
    b = run(dgtd, logits, sizes, BIDX[:5], minmax)[0]
    assert np.array_equal(a, b)


def raw_call(dgtd, logits, jobs, out, normalize=0, njobs=None, dt=None, Bn=None, out_bytes=None, ws=None):
    """The entry itself with a hand-made table: ``jobs`` = (out_off, H, W, batch, reserved0) per job."""
    L = dgtd._lib
    n = len(jobs)
    pinned = torch.empty(max(n, 1) * 32, dtype=torch.uint8, pin_memory=True)
    table = (L.PredictJob * max(n, 1)).from_buffer(pinned.numpy())
    for j, (off, H, W, b, r0) in enumerate(jobs):
        table[j].out_off, table[j].H, table[j].W, table[j].batch = off, H, W, b
        table[j].reserved[0], table[j].reserved[1], table[j].reserved[2] = r0, 0, 0
    dev = pinned.cuda()
    if ws is None:
        ws = torch.empty(16 * max(n, 1) + 16, dtype=torch.uint8, device="cuda")
    S = logits.shape[-1]
    L.call("dgtd_predict_maps", L.ptr(logits), L.dtype_code(logits) if dt is None else dt, logits.shape[0] if Bn is None else Bn, S, L.ptr(dev),
           pinned.data_ptr(), n if njobs is None else njobs, L.ptr(out), out.numel() if out_bytes is None else out_bytes, normalize, L.ptr(ws),
           ws.numel(), L.stream_ptr())
    torch.cuda.synchronize()
    return pinned, dev


def test_every_refusal_returns_an_error_and_leaves_the_output_untouched(dgtd, data):
    logits, _ = data[(32, "f32")]
    L = dgtd._lib
    out = torch.full((4096,), POISON, dtype=torch.uint8, device="cuda")
    good = [(0, 5, 7, 0, 0), (48, 3, 1, 2, 0)]
    bad_tables = {
        "H = 0": [(0, 0, 7, 0, 0)], "W = 0": [(0, 5, 0, 0, 0)], "H above 2^24": [(0, (1 << 24) + 1, 1, 0, 0)], "W above 2^24": [(0, 1, (1 << 24) + 1, 0, 0)],
        "misaligned offset": [good[0], (40, 3, 1, 2, 0)], "negative offset": [(-16, 5, 7, 0, 0)], "map past the end": [good[0], (4096 - 16, 5, 7, 0, 0)],
        "batch = B": [good[0], (48, 3, 1, B, 0)], "batch = -1": [(0, 5, 7, -1, 0)], "reserved field": [good[0], (48, 3, 1, 2, 1)],
    }
    for what, jobs in bad_tables.items():
        with pytest.raises(L.DgtdError, match="predict_maps"):
            raw_call(dgtd, logits, jobs, out)
        print(what, "->", L.load().dgtd_last_error().decode())
    for what, kw in {"no jobs": {"njobs": 0}, "too many jobs": {"njobs": 65536}, "fp64": {"dt": L.F64}, "unknown dtype": {"dt": 9},
                     "unknown normalize": {"normalize": 2}, "output too short": {"out_bytes": 50},
                     "workspace too small": {"normalize": 1, "ws": torch.empty(8, dtype=torch.uint8, device="cuda")}}.items():
        with pytest.raises(L.DgtdError, match="predict_maps"):
            raw_call(dgtd, logits, good, out, **kw)
        print(what, "->", L.load().dgtd_last_error().decode())
    with pytest.raises(L.DgtdError):
        L.predict_maps_layout([(1, 1)] * 65536)
    with pytest.raises(L.DgtdError):
        dgtd.ops.predict_maps(logits, [(5, 7)], out=torch.empty(8, dtype=torch.uint8, device="cuda"))      # the op's own check of `out`
    torch.cuda.synchronize()
    assert (out == POISON).all()
    raw_call(dgtd, logits, good, out)                                                                       # and the good table does run
    host = out.cpu().numpy()
    assert (host[:35] != POISON).any() and (host[35:48] == POISON).all() and (host[51:] == POISON).all()


@pytest.mark.parametrize("minmax", [False, True])
def test_captured_in_a_graph_and_replayed_twice(dgtd, data, minmax):
    logits, _ = data[(32, "f16")]
    sizes, bidx = [(33, 47), (5, 67), (32, 32), (3, 1)], [1, 2, 0, 0]
    eager, offsets, total = run(dgtd, logits, sizes, bidx, minmax)          # also the warm-up the capture needs
    static_out = torch.full((total + 64,), POISON, dtype=torch.uint8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dgtd.ops.predict_maps(logits, sizes, bidx, minmax=minmax, out=static_out)
    for _ in range(2):
        static_out.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(static_out.cpu().numpy(), eager)


def test_one_entry_call_one_upload_per_batch(dgtd, data, monkeypatch):
    """Counted at the op's boundary: one C entry call (one launch in plain mode, three with min-max: csrc/predict_maps.hip) and one
    copy (the job table) per call, whatever the number of maps; the library's own call records agree."""
    logits, _ = data[(32, "f32")]
    L = dgtd._lib
    sizes = R.target_sizes(32)
    run(dgtd, logits, sizes, BIDX)                                           # warm-up: the pinned tables exist
    calls, copies = [], []
    real_call, real_copy = L.call, torch.Tensor.copy_
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, *a, **k: (copies.append((self.device.type, a[0].device.type)), real_copy(self, *a, **k))[1])
    L.profile_native(True)
    try:
        offsets, total = L.predict_maps_layout(sizes)
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        dgtd.ops.predict_maps(logits, sizes, BIDX, out=out)
        dgtd.ops.predict_maps(logits, sizes, BIDX, minmax=True, out=out)
        rec = L.profile_native_summary()
    finally:
        L.profile_native(False)
        monkeypatch.undo()
    assert calls == ["dgtd_predict_maps"] * 2 and copies == [("cuda", "cpu")] * 2
    assert sorted(rec) == ["dgtd_predict_maps[8x<-32 minmax]", "dgtd_predict_maps[8x<-32 plain]"]
    assert all(v["calls"] == 1 and v["amount"] == 4 * B * 32 * 32 + sum(h * w for h, w in sizes) for v in rec.values())


def test_a_map_behind_two_gibibytes(dgtd, data):
    """Offsets are 64-bit: a job whose bytes lie past 2^31 in the packed buffer."""
    logits, planes = data[(32, "f32")]
    base = 1 << 31
    out = torch.empty(base + 4096, dtype=torch.uint8, device="cuda")
    out[base - 64:] = POISON
    H, W = 5, 67
    raw_call(dgtd, logits, [(base + 16, H, W, 1, 0)], out)
    tail = out[base - 64:].cpu().numpy()
    got = tail[80:80 + H * W].reshape(H, W)
    v, _ = R.levels(planes[1], H, W)
    assert R.accepts(got, v, R.eps_plain(R.max_abs(planes[1]))).all()
    assert (tail[:80] == POISON).all() and (tail[80 + H * W:] == POISON).all()
