"""CPU: the NumPy restatement of py_sod_metrics (tests/_sod_metrics_ref.py) anchored by hand, and the opt-in wiring of the device
S/E/F-measure evaluators into build_evaluators / Runner (built without touching a GPU)."""
import math

import numpy as np
import pytest

import _sod_metrics_ref as R

EPS = np.spacing(1)


def test_perfect_binary_prediction():
    N = 384 * 384
    rng = np.random.default_rng(0)
    gt = np.zeros((384, 384), np.float32)
    gt[100:260, 50:300] = 1.0
    gt[rng.random((384, 384)) < 0.01] = 1.0
    m = R.per_image(gt, gt)
    assert 1 - 1e-14 < m["sm"] < 1                             # 1 less the EPS terms of s_object / ssim (their sum depends on the mask)
    assert m["fm_curve"].max() == 1.0
    assert m["em_curve"].max() == pytest.approx(N / (N - 1 + EPS), rel=1e-15)     # every part aligned (enhanced value 1 - O(EPS))
    assert m["mae"] == 0.0


def test_hand_worked_4x4():
    # gt: 2x2 block top-left; pred: three of those four pixels plus one false positive -> TP 3, FP 1, FN 1
    gt = np.zeros((4, 4), np.float32)
    gt[:2, :2] = 1
    pred = np.zeros((4, 4), np.float32)
    pred[0, 0] = pred[0, 1] = pred[1, 0] = pred[2, 2] = 1
    m = R.per_image(pred, gt)
    assert m["mae"] == 2 / 16
    # F: P in {0, 1}, so every threshold above 0 sees TP 3 / 4 predicted / 4 positive; threshold 0 sees everything
    assert np.all(m["fm_curve"][:255] == pytest.approx(1.3 * 0.75 * 0.75 / (0.3 * 0.75 + 0.75)))
    assert m["fm_curve"][255] == pytest.approx(1.3 * 0.25 / (0.3 * 0.25 + 1.0))
    assert m["adp_fm"] == pytest.approx(0.75)                       # adaptive threshold 2 * 4/16 = 0.5
    # E at the adaptive threshold: parts (fgfg 3, fgbg 1, bgfg 1, bgbg 11), demeaned values +-(0.75, -0.25):
    # alignments 1, -0.6, -0.6, 1 -> enhanced 1, 0.04, 0.04, 1 -> (3 + 0.04 + 0.04 + 11) / 15
    assert m["adp_em"] == pytest.approx(14.08 / 15, abs=1e-14)
    assert m["em_curve"][0] == m["adp_em"]
    # S: object part by hand; the centroid (0.5, 0.5) rounds half to even -> (0, 0) -> X = Y = 1: the top-left quadrant holds one
    # pixel, its ssim divides 0 by 0 and the NaN score reports 0 (Python max(0, nan))
    S = R.Smeasure()
    P, G = R._prepare_data(R.quantise(pred), R.quantise(gt))
    fg = 2 * 0.75 / (0.75 ** 2 + 1 + 0.5 + EPS)
    bg_mean, bg_std = 11 / 12, math.sqrt(1 / 12)
    bg = 2 * bg_mean / (bg_mean ** 2 + 1 + bg_std + EPS)
    assert S.object(P, G) == pytest.approx(0.25 * fg + 0.75 * bg, abs=1e-15)
    assert S.centroid(G) == (1, 1)
    assert m["sm"] == 0


def test_degenerate_gt_branches():
    rng = np.random.default_rng(1)
    pred = rng.random((8, 12)).astype(np.float32)
    p8 = R.quantise(pred)
    P = p8 / 255
    P = (P - P.min()) / (P.max() - P.min())
    N = pred.size
    bg = R.per_image(pred, np.zeros_like(pred))
    assert bg["sm"] == pytest.approx(1 - P.mean(), abs=1e-15)
    assert bg["adp_fm"] == 0 and np.all(bg["fm_curve"] == 0) and np.all(bg["recall"] == 0)
    fgc = np.cumsum(np.flip(np.bincount((P * 255).astype(np.uint8).ravel(), minlength=256)))
    assert np.array_equal(bg["em_curve"], (N - fgc) / (N - 1 + EPS))
    fg = R.per_image(pred, np.ones_like(pred))
    assert fg["sm"] == pytest.approx(P.mean(), abs=1e-15)
    assert np.array_equal(fg["em_curve"], fgc / (N - 1 + EPS))
    assert fg["recall"][255] == 1.0


def test_constant_pred():
    gt = np.zeros((6, 6), np.float32)
    gt[1:4, 2:5] = 1
    m = R.per_image(np.full((6, 6), 0.5, np.float32), gt)
    c = 127 / 255                                             # (0.5 * 255) truncated, max == min so no normalisation
    assert m["mae"] == pytest.approx((9 * (1 - c) + 27 * c) / 36, abs=1e-15)
    assert m["adp_fm"] == 0 and m["adp_em"] == pytest.approx(9 / 35, abs=1e-14)    # threshold 2c > c: nothing predicted; 36 pixels at enhanced 1/4
    q = int(c * 255)                                          # the curves' second quantisation
    assert np.all(m["fm_curve"][:255 - q] == 0) and m["fm_curve"][255 - q] == pytest.approx(1.3 * 0.25 / (0.3 * 0.25 + 1.0))


def test_single_foreground_pixel_last_column():
    gt = np.zeros((5, 7), np.float32)
    gt[2, 6] = 1
    pred = np.linspace(0, 1, 35, dtype=np.float32).reshape(5, 7)
    m = R.per_image(pred, gt)
    assert m["sm"] == 0                                        # std with ddof=1 of one pixel and empty right quadrants: NaN -> 0
    assert np.isfinite(m["em_curve"]).all() and np.isfinite(m["fm_curve"]).all()


def test_wrapper_running_values():
    rng = np.random.default_rng(2)
    w = R.Wrappers()
    batches = [(rng.random((1, 10, 10)), (rng.random((1, 10, 10)) > 0.6)), (rng.random((3, 10, 10)), rng.random((3, 10, 10)) > 0.5)]
    for p, g in batches:
        w.process(p.astype(np.float32), g.astype(np.float32))
    out = w.compute_metrics()
    assert set(out) == {"Smeasure", "Emeasure", "Fmeasure", "MAE"}
    first = R.per_image(batches[0][0][0].astype(np.float32), batches[0][1][0].astype(np.float32))
    assert w.results["Smeasure"][0] == first["sm"]
    assert w.results["Fmeasure"][0] == first["fm_curve"].max()
    assert out["Smeasure"] == pytest.approx((w.results["Smeasure"][0] + w.results["Smeasure"][1]) / 2)
    assert set(w.summary()) == {"Smeasure", "MAE", "adpEm", "meanEm", "maxEm", "adpFm", "meanFm", "maxFm"}


# ---------------------------------------------------------------------------------------------------------------- evaluator wiring
VAL = [{"type": "Emeasure"}, {"type": "Fmeasure"}, {"type": "Smeasure"}, {"type": "MAE"}]


def test_build_evaluators_device_option():
    import dgtd
    logs = []
    ev = dgtd.runner.metrics.build_evaluators(VAL, logs.append, sod_metrics="device")
    assert [type(e).__name__ for e in ev] == ["Emeasure", "Fmeasure", "Smeasure", "MAE"]
    assert ev[0].acc is ev[1].acc is ev[2].acc                # one accumulator: one kernel chain per batch
    assert not logs
    assert all(e.compute_metrics()[e.name] == 0.0 for e in ev[:3])   # nothing processed yet: no device touched
    skipped = dgtd.runner.metrics.build_evaluators(VAL, logs.append)
    assert [type(e).__name__ for e in skipped] == ["MAE"]
    assert sum("skipped" in m for m in logs) == 3
    with pytest.raises(ValueError):
        dgtd.runner.metrics.build_evaluators(VAL, logs.append, sod_metrics="cpu")


def test_exported_metric_still_wins_in_device_mode():
    import dgtd
    R_ = dgtd.runner.registry

    class Emeasure:
        def __init__(self, prefix=None):
            self.prefix = prefix

    R_.REGISTRY["Emeasure"] = Emeasure
    try:
        ev = dgtd.runner.metrics.build_evaluators([{"type": "Emeasure", "prefix": "COD"}, {"type": "Smeasure"}], lambda m: None,
                                                  sod_metrics="device")
        assert isinstance(ev[0], Emeasure) and type(ev[1]).__name__ == "Smeasure"
    finally:
        R_.REGISTRY.pop("Emeasure", None)


RUNNER_YAML = """
train_cfg: {by_epoch: True, max_epochs: 1, val_interval: 1}
val_cfg: %s
model: {type: cod}
optim_wrapper:
  type: AmpOptimWrapper
  optimizer: {type: AdamW, lr: 0.0005, weight_decay: 0.1}
val_evaluator:
  - type: Emeasure
  - type: Fmeasure
  - type: Smeasure
  - type: MAE
"""


@pytest.mark.parametrize("val_cfg,kw,want", [("{sod_metrics: device}", None, ["Emeasure", "Fmeasure", "Smeasure", "MAE"]),
                                             ("{}", None, ["MAE"]), ("{}", "device", ["Emeasure", "Fmeasure", "Smeasure", "MAE"])])
def test_runner_reads_val_cfg(monkeypatch, tmp_path, val_cfg, kw, want):
    import torch
    import dgtd
    cfgmod = dgtd.runner.config
    monkeypatch.setattr(cfgmod, "build_model", lambda cfg, dt: torch.nn.Linear(4, 4))   # the evaluator wiring needs no real model
    cfg = dgtd.runner.load_config(RUNNER_YAML % val_cfg)
    logs = []
    extra = {} if kw is None else {"sod_metrics": kw}
    r = cfgmod.Runner(cfg, device="cpu", compute_dtype=torch.float32, work_dir=str(tmp_path), log=logs.append, **extra)
    assert [type(e).__name__ for e in r.evaluators] == want
    assert sum("skipped" in m for m in logs) == (3 if want == ["MAE"] else 0)
