"""GPU: dgtd.ops.sod_metrics and the device S/E/F-measure evaluators against the NumPy restatement of py_sod_metrics
(tests/_sod_metrics_ref.py).  Curves, precision and recall depend only on integer counts and EPS and must be bit-identical; the
scalar metrics sum fp64 terms in another order than NumPy's pairwise sums and must agree to 1e-12."""
import numpy as np
import pytest
import torch

import _sod_metrics_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _smooth(rng, B, H, W, lo=4):
    """Random smooth maps in [0, 1]: a bilinear up-sampling of coarse noise through a sigmoid."""
    z = torch.from_numpy(rng.standard_normal((B, 1, lo, lo))).float() * 3
    return torch.sigmoid(torch.nn.functional.interpolate(z, size=(H, W), mode="bilinear", align_corners=False))[:, 0]


def _case(seed, B, H, W):
    rng = np.random.default_rng(seed)
    pred = _smooth(rng, B, H, W)
    mask = (_smooth(rng, B, H, W, lo=6) > 0.5).float()
    pred[0, :3, :5] = 0.0                                     # exact 0 and 1 in the prediction
    pred[0, -2:, -4:] = 1.0
    g = float(np.nextafter(np.float32(129 / 255), np.float32(0)))
    mask[1, 5:9, 7:20] = g                                    # gt just below the 129/255 boundary of gt > 128
    return pred, mask


def _check(pred, gt, got, name):
    p = pred.float().cpu().numpy()
    g = gt.cpu().numpy()
    for b in range(p.shape[0]):
        want = R.per_image(p[b], g[b])
        for k in ("fm_curve", "precision", "recall"):
            assert np.array_equal(getattr(got, k)[b].cpu().numpy(), want[k]), (name, b, k)
        em = got.em_curve[b].cpu().numpy()
        if R.square_is_pow(g[b]):
            assert np.array_equal(em, want["em_curve"]), (name, b)
        else:   # the package squares a Python float with the C library's pow, which is not always correctly rounded
            np.testing.assert_allclose(em, want["em_curve"], rtol=1e-15, atol=0, err_msg=f"{name} {b}")
        for k in ("mae", "sm", "adp_em", "adp_fm"):
            assert abs(float(getattr(got, k)[b]) - want[k]) <= TOL, (name, b, k, float(getattr(got, k)[b]), want[k])


@pytest.mark.parametrize("H,W", [(384, 384), (512, 512), (352, 480)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_ops_match_restatement(H, W, dtype):
    import dgtd
    pred, gt = _case(H * 7 + W, 4, H, W)
    pred = pred.to(dtype)
    got = dgtd.ops.sod_metrics(pred.cuda().unsqueeze(1), gt.cuda().unsqueeze(1))
    _check(pred, gt, got, f"{H}x{W} {dtype}")
    again = dgtd.ops.sod_metrics(pred.cuda(), gt.cuda())      # [B,H,W] layout too; two runs bit-identical
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_edge_cases():
    import dgtd
    H, W = 48, 40
    rng = np.random.default_rng(5)
    smooth = _smooth(rng, 1, H, W)[0]
    preds, gts = [], []
    # perfect binary prediction
    g = torch.zeros(H, W)
    g[10:30, 5:25] = 1
    preds.append(g.clone()); gts.append(g)
    # all-background and all-foreground gt
    preds.append(smooth); gts.append(torch.zeros(H, W))
    preds.append(smooth); gts.append(torch.ones(H, W))
    # constant prediction of exactly 0 and of exactly 1 (P = 0 / 1 exactly: no summation-order ties in the quadrant means)
    preds.append(torch.zeros(H, W)); gts.append(g)
    preds.append(torch.ones(H, W)); gts.append(g)
    # single foreground pixel in the last column: NaN S-measure terms -> 0
    g1 = torch.zeros(H, W)
    g1[17, W - 1] = 1
    preds.append(smooth); gts.append(g1)
    # centroid on the last row: bottom quadrants empty
    g2 = torch.zeros(H, W)
    g2[H - 1, 3:30] = 1
    preds.append(smooth); gts.append(g2)
    pred, gt = torch.stack(preds), torch.stack(gts)
    got = dgtd.ops.sod_metrics(pred.cuda(), gt.cuda())
    _check(pred, gt, got, "edge")
    assert float(got.sm[5]) == 0.0 and float(got.sm[6]) == 0.0


def test_cpu_tensors_refused():
    import dgtd
    with pytest.raises(dgtd._lib.DgtdError):
        dgtd.ops.sod_metrics(torch.rand(1, 8, 8), torch.rand(1, 8, 8))


def _batches(seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for B in (1, 3, 3, 1):
        p, g = _case(int(rng.integers(1 << 30)), max(B, 2), 96, 80)
        out.append((p[:B].unsqueeze(1), g[:B].unsqueeze(1)))
    return out


def test_evaluator_contract(monkeypatch):
    import dgtd
    cfg = [{"type": "Emeasure"}, {"type": "Fmeasure"}, {"type": "Smeasure"}]
    evs = dgtd.runner.metrics.build_evaluators(cfg, lambda m: None, sod_metrics="device")
    batches = [(p.cuda(), g.cuda()) for p, g in _batches()]
    calls = []
    real = dgtd._lib.call
    monkeypatch.setattr(dgtd._lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])

    def validate():
        for ev in evs:                                          # what Runner.validate does before a pass
            ev.results.clear()
            ev.reset()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for p, g in batches:
                for ev in evs:
                    ev.process(None, (p, g))
        finally:
            torch.cuda.set_sync_debug_mode(0)
        out = {}
        for ev in evs:
            out.update(ev.compute_metrics())
        return out, evs[0].summary()

    got, summary = validate()
    assert calls == ["dgtd_sod_metrics", "dgtd_sod_metrics_accumulate"] * len(batches)   # one chain per batch for all three
    ref = R.Wrappers()
    for p, g in batches:
        ref.process(p.cpu().numpy(), g.cpu().numpy())
    want = ref.compute_metrics()
    for k in ("Smeasure", "Emeasure", "Fmeasure"):
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    want_s = ref.summary()
    assert set(summary) == set(want_s)
    for k in want_s:
        assert abs(summary[k] - want_s[k]) <= TOL, (k, summary[k], want_s[k])
    again, summary2 = validate()
    assert again == got and summary2 == summary


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
  # - type: WeightedFmeasure
  - type: MAE
"""


def test_runner_validate_end_to_end(monkeypatch, tmp_path):
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
    assert set(out) == {"Emeasure", "Fmeasure", "Smeasure", "MAE"}
    assert all(np.isfinite(v) for v in out.values())
    assert r.validate(loader) == out
