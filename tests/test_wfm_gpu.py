"""GPU: dgtd.ops.edt_nearest, dgtd.ops.weighted_fmeasure_rows and the device WeightedFmeasure evaluator (csrc/wfm.hip) against the
NumPy restatement (tests/_wfm_ref.py) and the scipy recordings of tests/golden/wfm.npz.  The transform is integer arithmetic and must
be exact.  The per-image Q must agree to WFM_TOL: helper and kernel add the 49 taps in the same order with every operation rounded,
so what differs is fp64 exp (the device's against NumPy's), the summation order of the three image sums (fixed tree on the device,
pairwise in NumPy) and the last bits of the kernel weights (libm's exp and a sequential sum against NumPy's)."""
import os

import numpy as np
import pytest
import torch

import _sod_metrics_ref as SR
import _wfm_ref as R

pytestmark = pytest.mark.gpu
# The bound of the fp64 scalars in test_sod_metrics_gpu.py.  MEASURED_MAX is the largest |device - helper| seen over every case of this
# file on an MI355X (most cases differ by 0): the device's fp64 exp needed no wider bound.
MEASURED_MAX = 2.3e-16
WFM_TOL = 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wfm.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {n: {k: z[f"{k}_{n}"] for k in ("pred", "gt", "q", "idx", "dst") if f"{k}_{n}" in z.files} for n in z["names"].tolist()}


def _smooth(rng, B, H, W, lo=4):
    z = torch.from_numpy(rng.standard_normal((B, 1, lo, lo))).float() * 3
    return torch.sigmoid(torch.nn.functional.interpolate(z, size=(H, W), mode="bilinear", align_corners=False))[:, 0]


_EDT = {}


def _ref_edt(mask: np.ndarray):
    """The helper's transform, computed once per mask and left unchanged."""
    key = (mask.shape, mask.tobytes())
    if key not in _EDT:
        d2, index = R.edt_nearest(mask)
        d2.setflags(write=False)
        index.setflags(write=False)
        _EDT[key] = (d2, index)
    return _EDT[key]


def _ref_q(pred_f32: np.ndarray, gt_f32: np.ndarray) -> float:
    """The helper's Q from the same uint8 quantisation the kernel applies, with the cached transform."""
    def edt(bg):
        d2, index = _ref_edt(~bg)
        return np.sqrt(d2.astype(np.float64)), index
    return R.step(SR.quantise(pred_f32), SR.quantise(gt_f32), edt=edt)


def _masks(seed, B, H, W):
    """Seeded masks: a smooth blob, sparse points, dense noise, ... cycled over the batch."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        kind = b % 3
        if kind == 0:
            out.append(_smooth(rng, 1, H, W, lo=6)[0].numpy() > 0.55)
        elif kind == 1:
            out.append(rng.random((H, W)) < 0.0005)
        else:
            out.append(rng.random((H, W)) < 0.4)
    return np.stack(out)


def _check_edt(masks: np.ndarray, name):
    import dgtd
    d2, index = dgtd.ops.edt_nearest(torch.from_numpy(masks).cuda())
    assert d2.dtype == index.dtype == torch.int32 and d2.shape == index.shape == masks.shape
    d2, index = d2.cpu().numpy(), index.cpu().numpy()
    for b, m in enumerate(masks.reshape(-1, *masks.shape[-2:])):
        want_d2, want_index = _ref_edt(m)
        assert np.array_equal(d2.reshape(-1, *m.shape)[b], want_d2), (name, b)
        assert np.array_equal(index.reshape(-1, *m.shape)[b], want_index), (name, b)


def test_edt_matches_scipy_recordings(golden):
    import dgtd
    for name, c in golden.items():
        mask = c["gt"] > 128
        _check_edt(mask, name)                                  # [H,W] layout, against the helper
        if mask.any():                                          # and against scipy's own output
            d2, index = dgtd.ops.edt_nearest(torch.from_numpy(mask).cuda())
            W = mask.shape[1]
            assert np.array_equal(index.cpu().numpy(), c["idx"][0].astype(np.int32) * W + c["idx"][1]), name
            assert np.array_equal(np.sqrt(d2.cpu().numpy().astype(np.float64)), c["dst"]), name


SHAPES = [(3, 384, 384), (2, 512, 512), (3, 75, 301)]          # the masks (and their reference transform) are shared by both tests


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_edt_seeded_masks(B, H, W):
    _check_edt(_masks(H * 5 + W, B, H, W), f"{B}x{H}x{W}")


def test_edt_empty_full_and_single_column():
    H, W = 45, 70                                               # W is no multiple of the 64-lane column blocks
    masks = _masks(3, 4, H, W)
    masks[1] = False                                            # empty image: -1 in both outputs
    masks[2] = True                                             # full image: every pixel is its own nearest
    import dgtd
    d2, index = dgtd.ops.edt_nearest(torch.from_numpy(masks).cuda())
    assert bool((d2[1] == -1).all()) and bool((index[1] == -1).all())
    assert bool((d2[2] == 0).all()) and torch.equal(index[2].cpu().flatten(), torch.arange(H * W, dtype=torch.int32))
    _check_edt(masks, "empty/full")
    _check_edt(_masks(4, 2, 57, 1), "one column")
    _check_edt(_masks(5, 2, 1, 57), "one row")


def test_edt_widest_supported_row_and_refusal():
    import dgtd
    Wmax = dgtd.ops.wfm.EDT_MAX_W
    mask = np.random.default_rng(9).random((1, 1, Wmax)) < 0.001
    _check_edt(mask, "widest")
    for shape in ((1, 1, Wmax + 1), (1, Wmax + 1, 1)):         # a map the kernel cannot serve: error status, nothing launched
        with pytest.raises(dgtd._lib.DgtdError, match="exceeds"):
            dgtd.ops.edt_nearest(torch.zeros(shape, dtype=torch.uint8, device="cuda"))
    with pytest.raises(dgtd._lib.DgtdError, match="exceeds"):
        dgtd.ops.weighted_fmeasure_rows(torch.zeros(1, 1, Wmax + 1, device="cuda"), torch.zeros(1, 1, Wmax + 1, device="cuda"))


def test_cpu_tensors_refused():
    import dgtd
    with pytest.raises(dgtd._lib.DgtdError):
        dgtd.ops.edt_nearest(torch.zeros(1, 8, 8, dtype=torch.bool))
    with pytest.raises(dgtd._lib.DgtdError):
        dgtd.ops.weighted_fmeasure_rows(torch.rand(1, 8, 8), torch.rand(1, 8, 8))
    with pytest.raises(dgtd._lib.DgtdError):
        dgtd.ops.weighted_fmeasure_accumulate(torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.float64),
                                              torch.zeros(1, dtype=torch.float64))


def _case(seed, B, H, W, mask_seed=None):
    rng = np.random.default_rng(seed)
    pred = _smooth(rng, B, H, W)
    gt = torch.from_numpy(_masks(seed + 1 if mask_seed is None else mask_seed, B, H, W)).float()
    pred[0] = (pred[0] * 0.5 + gt[0] * 0.5).clamp(0, 1)         # a prediction that follows its gt: EA < E on part of the foreground
    pred[0, :3, :5] = 0.0
    pred[0, -2:, -4:] = 1.0
    return pred, gt


def _check_rows(pred, gt, got, name):
    p, g = pred.float().cpu().numpy(), gt.cpu().numpy()
    worst = 0.0
    for b in range(p.shape[0]):
        want = _ref_q(p[b], g[b])
        err = abs(float(got[b]) - want)
        worst = max(worst, err)
        print(f"wfm {name} image {b}: device {float(got[b])!r} helper {want!r} |diff| {err:.3e}")
        assert err <= WFM_TOL, (name, b, float(got[b]), want)
    return worst


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_rows_match_restatement(B, H, W, dtype):
    import dgtd
    pred, gt = _case(H * 7 + W, B, H, W, mask_seed=H * 5 + W)
    pred = pred.to(dtype)
    got = dgtd.ops.weighted_fmeasure_rows(pred.cuda().unsqueeze(1), gt.cuda().unsqueeze(1))
    assert got.dtype == torch.float64 and got.shape == (B,)
    _check_rows(pred, gt, got, f"{B}x{H}x{W} {dtype}")
    again = dgtd.ops.weighted_fmeasure_rows(pred.cuda(), gt.cuda())     # [B,H,W] layout too; a second launch is bit-identical
    assert torch.equal(got, again)


def test_rows_match_scipy_recordings(golden):
    import dgtd
    for name, c in golden.items():
        pred = ((c["pred"].astype(np.float32) + 0.5) / 255).astype(np.float32)     # mid-bin: quantises back to the recorded uint8
        gt = (c["gt"] > 128).astype(np.float32)
        assert np.array_equal(SR.quantise(pred), c["pred"])
        got = dgtd.ops.weighted_fmeasure_rows(torch.from_numpy(pred)[None].cuda(), torch.from_numpy(gt)[None].cuda())
        err = abs(float(got[0]) - float(c["q"]))
        print(f"wfm golden {name}: device {float(got[0])!r} scipy formula {float(c['q'])!r} |diff| {err:.3e}")
        assert err <= WFM_TOL, (name, float(got[0]), float(c["q"]))
        _check_rows(torch.from_numpy(pred)[None], torch.from_numpy(gt)[None], got, f"golden {name}")


def test_edge_cases_and_empty_gt_is_exactly_zero():
    import dgtd
    H, W = 48, 40
    rng = np.random.default_rng(5)
    smooth = _smooth(rng, 1, H, W)[0]
    g = torch.zeros(H, W)
    g[10:30, 5:25] = 1
    g1 = torch.zeros(H, W)
    g1[17, W - 1] = 1
    just_below = torch.full((H, W), float(np.nextafter(np.float32(129 / 255), np.float32(0))))    # quantises to 128: background
    pairs = [(g.clone(), g),                                    # perfect binary prediction
             (smooth, torch.zeros(H, W)),                       # empty gt
             (smooth, torch.ones(H, W)),                        # all-foreground gt
             (torch.zeros(H, W), g), (torch.ones(H, W), g),     # constant predictions
             (torch.full((H, W), 0.5), g),
             (smooth, g1),                                      # single foreground pixel in the last column
             (smooth, just_below)]                              # empty after quantisation
    pred, gt = torch.stack([p for p, _ in pairs]), torch.stack([q for _, q in pairs])
    got = dgtd.ops.weighted_fmeasure_rows(pred.cuda(), gt.cuda())
    _check_rows(pred, gt, got, "edge")
    host = got.cpu()
    assert host[1].item() == 0.0 and host[7].item() == 0.0      # exactly 0, not merely small
    assert not torch.signbit(host[1]) and bool(torch.isfinite(host).all())
    assert abs(host[0].item() - 1.0) <= 1e-15


def _guarded(n, dtype, fill):
    pad = 64
    flat = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
    return flat, flat[pad:pad + n]


def _guards_intact(flat, n, name):
    g = torch.cat([flat[:64], flat[64 + n:]])
    ok = torch.isnan(g).all() if flat.is_floating_point() else (g == 0xA5).all()
    assert bool(ok), f"{name}: the kernels wrote outside their buffer"


def test_guard_buffers_and_bit_identical_relaunch():
    import dgtd
    L = dgtd._lib
    B, H, W = 3, 53, 77
    pred, gt = _case(21, B, H, W)
    pred, gt = pred.cuda().contiguous(), gt.cuda().contiguous()
    nws = L.load().dgtd_wfm_workspace(B, H, W)
    runs = []
    for _ in range(2):
        oflat, out = _guarded(B, torch.float64, float("nan"))
        wflat, ws = _guarded(nws, torch.uint8, 0xA5)
        L.call("dgtd_wfm", L.ptr(pred), L.dtype_code(pred), L.ptr(gt), L.ptr(out), L.ptr(ws), B, H, W, L.stream_ptr())
        _guards_intact(oflat, B, "out")
        _guards_intact(wflat, nws, "workspace")
        assert bool(torch.isfinite(out).all())                 # every element written
        runs.append(out.clone())
    assert torch.equal(runs[0], runs[1])
    _check_rows(pred, gt, runs[0], "guarded")
    # the transform alone: int32 outputs inside NaN-patterned fp32 buffers
    mask = (gt > 0.5).to(torch.uint8).contiguous()
    outs = []
    for _ in range(2):
        dflat, d2 = _guarded(B * H * W, torch.float32, float("nan"))
        iflat, ix = _guarded(B * H * W, torch.float32, float("nan"))
        L.call("dgtd_edt_nearest", L.ptr(mask), L.ptr(d2), L.ptr(ix), B, H, W, L.stream_ptr())
        _guards_intact(dflat, B * H * W, "dist2")
        _guards_intact(iflat, B * H * W, "index")
        outs.append((d2.view(torch.int32).clone(), ix.view(torch.int32).clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for b in range(B):
        want_d2, want_index = _ref_edt(mask[b].cpu().numpy() != 0)
        assert np.array_equal(outs[0][0].view(B, H, W)[b].cpu().numpy(), want_d2)
        assert np.array_equal(outs[0][1].view(B, H, W)[b].cpu().numpy(), want_index)


def test_accumulate_running_mean():
    import dgtd
    state = torch.zeros(2, dtype=torch.float64, device="cuda")
    slots = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    a = torch.tensor([0.25, 0.5, 0.0], dtype=torch.float64, device="cuda")
    b = torch.tensor([1.0], dtype=torch.float64, device="cuda")
    dgtd.ops.weighted_fmeasure_accumulate(a, state, slots[0:1])
    dgtd.ops.weighted_fmeasure_accumulate(b, state, slots[1:2])
    assert state.tolist() == [4.0, 1.75] and slots.tolist() == [0.25, 0.4375]


def _batches(seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for B in (1, 3, 2, 1):
        p, g = _case(int(rng.integers(1 << 30)), 3, 72, 56)
        out.append((p[:B].unsqueeze(1), g[:B].unsqueeze(1)))
    out[2][1][1].zero_()                                        # one image with an empty gt inside a batch
    return out


def test_evaluator_contract(monkeypatch):
    import dgtd
    cfg = [{"type": "Smeasure"}, {"type": "WeightedFmeasure"}]
    evs = dgtd.runner.metrics.build_evaluators(cfg, lambda m: None, sod_metrics="device")
    wf = evs[1]
    batches = [(p.cuda(), g.cuda()) for p, g in _batches()]
    calls = []
    real = dgtd._lib.call
    monkeypatch.setattr(dgtd._lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])

    def validate():
        for ev in evs:                                          # what Runner.validate does before a pass
            ev.results.clear()
            ev.reset()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                 # process() must not synchronise
        try:
            for p, g in batches:
                for ev in evs:
                    ev.process(None, (p, g))
        finally:
            torch.cuda.set_sync_debug_mode(0)
        running = wf.running[:len(wf.results)].cpu().tolist()
        out = {}
        for ev in evs:
            out.update(ev.compute_metrics())
        return running, out, wf.summary()

    running, got, summary = validate()
    assert [c for c in calls if "wfm" in c] == ["dgtd_wfm", "dgtd_wfm_accumulate"] * len(batches)
    ref = R.Wrapper()
    for p, g in batches:
        ref.process(p.cpu().numpy(), g.cpu().numpy())
    assert len(running) == len(ref.results)
    for k, (a, b) in enumerate(zip(running, ref.results)):      # per-batch running means
        assert abs(a - b) <= WFM_TOL, (k, a, b)
    want = ref.compute_metrics()["WeightedFmeasure"]
    assert abs(got["WeightedFmeasure"] - want) <= WFM_TOL, (got, want)
    assert abs(summary["wFmeasure"] - ref.summary()["wFmeasure"]) <= WFM_TOL
    assert {"Smeasure", "MAE", "maxFm", "wFmeasure"} <= set(summary) and evs[0].summary() == summary
    again = validate()                                          # reset(): a second pass starts from nothing
    assert again == (running, got, summary)
    wf.reset()
    assert wf.compute_metrics() == {"WeightedFmeasure": 0.0} and "wFmeasure" not in wf.summary()
    alone = dgtd.runner.metrics.build_evaluators(cfg[1:], lambda m: None, sod_metrics="device")[0]
    alone.process(None, batches[0])
    assert set(alone.summary()) == {"wFmeasure"} and abs(alone.summary()["wFmeasure"] - ref.results[0]) <= WFM_TOL


VAL_YAML = """
train_cfg: {by_epoch: True, max_epochs: 1, val_interval: 1}
val_cfg: {sod_metrics: device}
model: {type: cod}
optim_wrapper:
  type: AmpOptimWrapper
  optimizer: {type: AdamW, lr: 0.0005, weight_decay: 0.1}
val_evaluator:
  - type: Emeasure
  - type: Fmeasure
  - type: Smeasure
  - type: WeightedFmeasure
  - type: MAE
"""


def test_runner_validate_with_all_five_evaluators(monkeypatch, tmp_path):
    import dgtd

    class Tiny(torch.nn.Module):
        """Stands in for cod's predict mode: (sigmoid map, label) from the batch dict's tensors."""

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, raw, image, label, depth, mode="predict"):
            return torch.sigmoid(self.w * (image[:, :1] - 0.5) * 4), label

    monkeypatch.setattr(dgtd.runner.config, "build_model", lambda cfg, dt: Tiny())
    r = dgtd.runner.Runner(dgtd.runner.load_config(VAL_YAML), device="cuda", compute_dtype=torch.float32, work_dir=str(tmp_path),
                           log=lambda m: None)
    rng = np.random.default_rng(3)
    loader = []
    for B in (2, 1):
        p, g = _case(int(rng.integers(1 << 30)), 2, 64, 64)
        loader.append({"input": p[:B].unsqueeze(1).repeat(1, 3, 1, 1).cuda(), "label": g[:B].unsqueeze(1).cuda(), "depth": None})
    out = r.validate(loader)
    assert set(out) == {"Emeasure", "Fmeasure", "Smeasure", "WeightedFmeasure", "MAE"}
    assert all(np.isfinite(v) for v in out.values())
    # the stand-in's sigmoid runs on the device; the helper gets the same map through the device so that both quantise one input
    ref2 = R.Wrapper()
    for b in loader:
        ref2.process(torch.sigmoid((b["input"][:, :1] - 0.5) * 4).cpu().numpy(), b["label"].cpu().numpy())
    assert abs(out["WeightedFmeasure"] - ref2.compute_metrics()["WeightedFmeasure"]) <= WFM_TOL
    assert r.validate(loader) == out


def test_chain_replays_inside_a_captured_graph():
    import dgtd
    B, H, W = 2, 96, 80
    pred, gt = _case(31, B, H, W)
    pred, gt = pred.cuda(), gt.cuda()
    state = torch.zeros(2, dtype=torch.float64, device="cuda")
    slot = torch.zeros(1, dtype=torch.float64, device="cuda")
    eager = dgtd.ops.weighted_fmeasure_rows(pred, gt)
    dgtd.ops.weighted_fmeasure_accumulate(eager, state, slot)
    eager_state, eager_slot = state.clone(), slot.clone()
    state.zero_()
    slot.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # one stream: memset node, five kernels, accumulate - a single chain
        rows = dgtd.ops.weighted_fmeasure_rows(pred, gt)
        dgtd.ops.weighted_fmeasure_accumulate(rows, state, slot)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rows, eager) and torch.equal(state, eager_state) and torch.equal(slot, eager_slot)
    _check_rows(pred, gt, rows, "graph")
