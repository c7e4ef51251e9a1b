"""GPU: dgtd_sod_metrics_ragged (dgtd.ops.sod_metrics_ragged) - S/E/F-measure and MAE of a batch of uint8 maps, each image at its own
size, on the packed bytes of ops.predict_maps.  Two yardsticks, no tolerance of this file's own: every row is bit-identical to the row
the dense entry gives for that image alone (float inputs that quantise to the same bytes), and agrees with the NumPy restatement of
py_sod_metrics (tests/_sod_metrics_ref.py, fed the uint8 arrays directly) under the acceptance rule of tests/test_sod_metrics_gpu.py:
integer-count curves bit-identical, the E-measure curve bit-identical where the package's ``x ** 2`` equals ``x * x`` (rtol 1e-15
otherwise), the scalars within TOL = 1e-12."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import _sod_metrics_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-12
POISON = 0xA5
# an image below one 16-byte load, odd widths and tails, one image swept by several blocks
SIZES = [(1, 1), (2, 3), (3, 5), (17, 16), (16, 17), (33, 47), (64, 48), (129, 255), (300, 200)]
ORDER = [4, 8, 0, 6, 2, 7, 1, 5, 3]          # job j is stored image ORDER[j]: the jobs are listed in another order than they are stored


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


def opmod(dgtd):
    """The module ops/sod_metrics.py (``dgtd.ops.sod_metrics`` is the function of that name)."""
    return sys.modules[dgtd.ops.__name__ + ".sod_metrics"]


def smooth8(rng, H, W, lo=4):
    """A smooth seeded prediction as bytes: coarse noise, bilinear up-sampling, sigmoid, save_image's rounding."""
    z = torch.from_numpy(rng.standard_normal((1, 1, lo, lo))).float() * 3
    s = torch.sigmoid(torch.nn.functional.interpolate(z, size=(H, W), mode="bilinear", align_corners=False))[0, 0]
    return (s * 255 + 0.5).clamp(0, 255).to(torch.uint8).numpy()


def blob8(rng, H, W):
    return ((smooth8(rng, H, W, lo=6) > 127) * 255).astype(np.uint8)


def pack(dgtd, preds, gts, order=None, tail=64):
    """Both lists into poisoned packed buffers in STORAGE order; ``RaggedMaps`` lists them in ``order``."""
    sizes = [p.shape for p in preds]
    offsets, total = dgtd._lib.predict_maps_layout(sizes)
    hp = np.full(total + tail, POISON, np.uint8)
    hg = np.full(total + tail, POISON, np.uint8)
    for p, g, off in zip(preds, gts, offsets):
        hp[off:off + p.size] = p.reshape(-1)
        hg[off:off + g.size] = g.reshape(-1)
    order = list(range(len(preds))) if order is None else order
    return dgtd.ops.RaggedMaps(torch.from_numpy(hp).cuda(), torch.from_numpy(hg).cuda(), [sizes[i] for i in order], [offsets[i] for i in order])


def restated(p8, g8):
    """tests/_sod_metrics_ref.py stepped on the uint8 arrays directly (per_image() without its quantisation)."""
    S, E, F, M = R.Smeasure(), R.Emeasure(), R.Fmeasure(), R.MAE()
    for m in (S, E, F, M):
        m.step(p8, g8)
    return dict(mae=float(M.maes[0]), sm=float(S.sms[0]), adp_em=float(E.adaptive_ems[0]), adp_fm=float(F.adaptive_fms[0]),
                em_curve=np.asarray(E.changeable_ems[0], np.float64), fm_curve=F.changeable_fms[0], precision=F.precisions[0], recall=F.recalls[0])


def square_is_pow(g8):
    n, c = g8.size, int(np.count_nonzero(g8 > 128))
    if c in (0, n):
        return True
    return all(v ** 2 == v * v for v in (1 - c / n, 0 - c / n))


def check_row(got, b, p8, g8, name):
    """The acceptance rule of tests/test_sod_metrics_gpu.py::_check for row ``b`` of ``got``."""
    want = restated(p8, g8)
    for k in ("fm_curve", "precision", "recall"):
        assert np.array_equal(getattr(got, k)[b].cpu().numpy(), want[k]), (name, b, k)
    em = got.em_curve[b].cpu().numpy()
    if square_is_pow(g8):
        assert np.array_equal(em, want["em_curve"]), (name, b)
    else:
        np.testing.assert_allclose(em, want["em_curve"], rtol=1e-15, atol=0, err_msg=f"{name} {b}")
    for k in ("mae", "sm", "adp_em", "adp_fm"):
        v = float(getattr(got, k)[b])
        print(name, b, k, v, want[k])
        assert abs(v - want[k]) <= TOL, (name, b, k, v, want[k])


def dense_row(dgtd, p8, g8):
    """The dense entry on this image alone: B = 1, float inputs that quantise to the same bytes."""
    pf = (torch.from_numpy(p8).float() + 0.5) / 255
    assert np.array_equal(R.quantise(pf.numpy()), p8)                      # (x * 255) truncates back to p8
    gf = torch.from_numpy((g8 > 128).astype(np.float32))
    return opmod(dgtd).sod_metrics_rows(pf.cuda()[None], gf.cuda()[None])[0]


def mixed(kind):
    rng = np.random.default_rng(20 if kind == "smooth" else 21)
    preds, gts = [], []
    for i, (H, W) in enumerate(SIZES):
        preds.append(smooth8(rng, H, W) if kind == "smooth" else rng.integers(0, 256, (H, W), dtype=np.uint8))
        gts.append(blob8(rng, H, W) if i % 2 == 0 else (rng.integers(0, 2, (H, W), dtype=np.uint8) * 255).astype(np.uint8))
    return preds, gts


def test_quantisation_premise_holds_for_all_bytes():
    p = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.quantise(((torch.from_numpy(p).float() + 0.5) / 255).numpy()), p)


@pytest.mark.parametrize("kind", ["smooth", "random"])
def test_mixed_sizes_in_one_call(dgtd, kind):
    preds, gts = mixed(kind)
    maps = pack(dgtd, preds, gts, ORDER)
    rows = dgtd.ops.sod_metrics_ragged_rows(maps)
    got = opmod(dgtd).split_rows(rows)
    torch.cuda.synchronize()
    assert (maps.pred8[-64:] == POISON).all() and (maps.gt8[-64:] == POISON).all()
    for j, i in enumerate(ORDER):
        assert torch.equal(rows[j], dense_row(dgtd, preds[i], gts[i])), (kind, SIZES[i])       # (a) bit-identical to the dense entry
        if SIZES[i] != (1, 1):                                                                 # (b) 1x1: the E-measure divides by EPS
            check_row(got, j, preds[i], gts[i], f"{kind} {SIZES[i]}")


def edge_maps():
    rng = np.random.default_rng(5)
    preds, gts, names = [], [], []
    for (H, W) in [(48, 40), (37, 53)]:
        smooth = smooth8(rng, H, W)
        g = np.zeros((H, W), np.uint8)
        g[10:30, 5:25] = 255
        g1 = np.zeros((H, W), np.uint8)
        g1[17, W - 1] = 255
        g2 = np.zeros((H, W), np.uint8)
        g2[H - 1, 3:30] = 255
        for name, p, t in [("empty gt", smooth, np.zeros((H, W), np.uint8)), ("full gt", smooth, np.full((H, W), 255, np.uint8)),
                           ("pred 0", np.zeros((H, W), np.uint8), g), ("pred 255", np.full((H, W), 255, np.uint8), g),
                           ("one pixel, last column", smooth, g1), ("centroid on the last row", smooth, g2)]:
            preds.append(p), gts.append(t), names.append(f"{name} {H}x{W}")
    return preds, gts, names


def test_edge_maps_inside_a_ragged_call(dgtd):
    preds, gts, names = edge_maps()
    got = dgtd.ops.sod_metrics_ragged(pack(dgtd, preds, gts))
    for b, name in enumerate(names):
        check_row(got, b, preds[b], gts[b], name)
    for b in (4, 5, 10, 11):                                   # NaN S-measure terms report 0, as Python's max(0, nan)
        assert float(got.sm[b]) == 0.0, names[b]


def test_two_calls_agree_and_rows_do_not_depend_on_the_company(dgtd):
    preds, gts = mixed("smooth")
    maps = pack(dgtd, preds, gts, ORDER)
    a, b = dgtd.ops.sod_metrics_ragged_rows(maps), dgtd.ops.sod_metrics_ragged_rows(maps)
    assert torch.equal(a, b)
    i = 7                                                      # 129 x 255: alone, and among eight others (job 5 of ORDER)
    alone = dgtd.ops.sod_metrics_ragged_rows(pack(dgtd, [preds[i]], [gts[i]]))
    assert torch.equal(alone[0], a[ORDER.index(i)])


def raw_call(dgtd, maps_or_ptrs, jobs, out, njobs=None, nbytes=None, ws=None, null=None):
    """The C entry with a job table of this test's making: ``jobs`` = (off, H, W) per job.  Returns the status code."""
    L = dgtd._lib
    pred8, gt8 = maps_or_ptrs
    n = len(jobs)
    host = (L.PredictJob * n)()
    for j, (off, H, W) in enumerate(jobs):
        host[j].out_off, host[j].H, host[j].W, host[j].batch = off, H, W, -3            # `batch` is ignored by this entry
    dev = torch.from_numpy(np.frombuffer(bytes(host), np.uint8).copy()).cuda()
    ws = torch.empty(L.load().dgtd_sod_metrics_workspace(max(n, 1)), dtype=torch.uint8, device="cuda") if ws is None else ws
    args = {"pred8": pred8.data_ptr(), "gt8": gt8.data_ptr(), "bytes": pred8.numel() if nbytes is None else nbytes, "jobs_dev": dev.data_ptr(),
            "jobs_host": ctypes.cast(host, ctypes.c_void_p).value, "njobs": n if njobs is None else njobs, "out": out.data_ptr(),
            "ws": ws.data_ptr(), "stream": L.stream_ptr()}
    if null:
        args[null] = None
    rc = L.load().dgtd_sod_metrics_ragged(*args.values())
    torch.cuda.synchronize()
    return rc


def test_every_refusal_returns_an_error_and_leaves_out_untouched(dgtd):
    L = dgtd._lib
    pred8 = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    gt8 = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((2, opmod(dgtd).ROW), -7.0, dtype=torch.float64, device="cuda")
    good = [(0, 5, 7), (48, 3, 1)]
    bad_tables = {
        "H = 0": [(0, 0, 7)], "W = 0": [(0, 5, 0)], "H < 0": [(0, -5, 7)], "H above 2^24": [(0, (1 << 24) + 1, 1)], "W above 2^24": [(0, 1, (1 << 24) + 1)],
        "H*W above 2^31": [(0, 1 << 16, (1 << 15) + 1)], "misaligned offset": [good[0], (40, 3, 1)], "negative offset": [(-16, 5, 7)],
        "map past the end": [good[0], (4096 - 16, 5, 7)],
    }
    for what, jobs in bad_tables.items():
        kw = {"nbytes": 1 << 40} if what == "H*W above 2^31" else {}
        assert raw_call(dgtd, (pred8, gt8), jobs, out, **kw) != 0, what
        print(what, "->", L.load().dgtd_last_error().decode())
    for what, kw in {"no jobs": {"njobs": 0}, "negative job count": {"njobs": -1}, "too many jobs": {"njobs": 65536}, "buffer too short": {"nbytes": 50},
                     "null pred8": {"null": "pred8"}, "null gt8": {"null": "gt8"}, "null device table": {"null": "jobs_dev"},
                     "null host table": {"null": "jobs_host"}, "null workspace": {"null": "ws"}}.items():
        assert raw_call(dgtd, (pred8, gt8), good, out, **kw) != 0, what
        print(what, "->", L.load().dgtd_last_error().decode())
    assert (out == -7.0).all()
    assert raw_call(dgtd, (pred8, gt8), good, out, null="out") != 0
    with pytest.raises(L.DgtdError):                           # CPU tensors
        dgtd.ops.sod_metrics_ragged(dgtd.ops.RaggedMaps(torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), [(5, 7)], [0]))
    with pytest.raises(L.DgtdError, match="sod_metrics_ragged"):   # through the op: the entry's refusal becomes the exception
        dgtd.ops.sod_metrics_ragged(dgtd.ops.RaggedMaps(pred8, gt8, [(5, 7)], [8]))
    assert raw_call(dgtd, (pred8, gt8), good, out) == 0        # and the good table does run
    assert not (out == -7.0).any()


def test_captured_in_a_graph_and_replayed_twice(dgtd):
    S = opmod(dgtd)
    sets = [mixed("smooth"), mixed("random"), (mixed("random")[0], mixed("smooth")[1])]
    packs = [pack(dgtd, p, g, ORDER) for p, g in sets]
    eager = []
    for m in packs:                                            # the eager results (and the warm-up the capture needs)
        state, slot = torch.zeros(S.STATE, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
        rows = S.sod_metrics_ragged_rows(m)
        S.sod_metrics_accumulate(rows, state, slot)
        eager.append((rows, state, slot))
    static = dgtd.ops.RaggedMaps(packs[0].pred8.clone(), packs[0].gt8.clone(), packs[0].sizes, packs[0].offsets)
    state, slot = torch.zeros(S.STATE, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # one stream, no parallel branches
        rows = S.sod_metrics_ragged_rows(static)
        S.sod_metrics_accumulate(rows, state, slot)
    for k in (1, 2):
        static.pred8.copy_(packs[k].pred8)
        static.gt8.copy_(packs[k].gt8)
        state.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(rows, eager[k][0]) and torch.equal(state, eager[k][1]) and torch.equal(slot, eager[k][2])
        assert not torch.equal(rows, eager[k - 1][0])          # the rows follow the bytes


def test_a_map_behind_two_gibibytes(dgtd):
    """Offsets are 64-bit: a map placed past 2^31 in both buffers scores like the same map at offset 0."""
    rng = np.random.default_rng(9)
    H, W = 33, 47
    p8, g8 = smooth8(rng, H, W), blob8(rng, H, W)
    near = dgtd.ops.sod_metrics_ragged_rows(pack(dgtd, [p8], [g8]))
    base = (1 << 31) + 4096
    bufs = []
    for a in (p8, g8):
        t = torch.empty(base + H * W + 64, dtype=torch.uint8, device="cuda")
        t[base - 64:] = POISON
        t[base:base + H * W] = torch.from_numpy(a.reshape(-1)).cuda()
        bufs.append(t)
    far = dgtd.ops.sod_metrics_ragged_rows(dgtd.ops.RaggedMaps(bufs[0], bufs[1], [(H, W)], [base]))
    assert torch.equal(far, near)


class RestatedWrappers:
    """The reference's S/E/F/MAE wrappers over ragged batches: every image stepped on its uint8 arrays, ONE running value appended
    per batch, compute_metrics = the mean of those values (tests/_sod_metrics_ref.py: Wrappers, which takes equal-sized float maps)."""

    def __init__(self):
        self.w = R.Wrappers()

    def process(self, preds, gts):
        w = self.w
        for p8, g8 in zip(preds, gts):
            for m in (w.S, w.E, w.F, w.M):
                m.step(p8, g8)
        w.results["Smeasure"].append(w.S.get_results()["sm"])
        w.results["Emeasure"].append(w.E.get_results()["em"]["curve"].max())
        w.results["Fmeasure"].append(w.F.get_results()["fm"]["curve"].max())
        w.results["MAE"].append(w.M.get_results()["mae"])


def test_accumulator_contract_over_ragged_batches(dgtd, monkeypatch):
    rng = np.random.default_rng(11)
    sizes = [(96, 80), (33, 47), (64, 48), (50, 77), (17, 16), (120, 90), (75, 200), (41, 41)]
    imgs = [(smooth8(rng, H, W), blob8(rng, H, W)) for (H, W) in sizes]
    groups = [imgs[0:1], imgs[1:4], imgs[4:7], imgs[7:8]]                  # batches of 1, 3, 3 and 1 images
    batches = [pack(dgtd, [p for p, _ in grp], [g for _, g in grp]) for grp in groups]
    cfg = [{"type": "Emeasure"}, {"type": "Fmeasure"}, {"type": "Smeasure"}, {"type": "MAE"}]
    evs = dgtd.runner.metrics.build_evaluators(cfg, lambda m: None, sod_metrics="device", score_size="original")
    dgtd.ops.sod_metrics_ragged_rows(batches[1])                           # warm-up: the pinned job tables exist
    calls = []
    real = dgtd._lib.call
    monkeypatch.setattr(dgtd._lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])

    def validate():
        for ev in evs:                                                     # what Runner.validate does before a pass
            ev.results.clear()
            ev.reset()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for maps in batches:
                for ev in evs:
                    ev.process(None, maps)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        out = {}
        for ev in evs:
            out.update(ev.compute_metrics())
        return out, evs[0].summary()

    got, summary = validate()
    assert calls == ["dgtd_sod_metrics_ragged", "dgtd_sod_metrics_accumulate"] * len(batches)   # one chain per batch for all four
    ref = RestatedWrappers()
    for grp in groups:
        ref.process([p for p, _ in grp], [g for _, g in grp])
    want = ref.w.compute_metrics()
    assert set(got) == set(want)
    for k in want:
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    want_s = ref.w.summary()
    assert set(summary) == set(want_s)
    for k in want_s:
        assert abs(summary[k] - want_s[k]) <= TOL, (k, summary[k], want_s[k])
    again, summary2 = validate()
    assert again == got and summary2 == summary
