"""CPU: the NumPy restatement of the weighted F-measure (tests/_wfm_ref.py) against what scipy recorded in tests/golden/wfm.npz
(tools/make_golden_wfm.py): nearest-foreground indices and distances exactly, the per-image Q to 1e-12 - and the wiring of the device
``WeightedFmeasure`` evaluator into build_evaluators (built without touching a GPU)."""
import os

import numpy as np
import pytest

import _wfm_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wfm.npz")
TOL = 1e-12          # the bound of test_sod_metrics_cpu.py for fp64 scalars: only the summation order of the 49 taps differs


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {n: {k: z[f"{k}_{n}"] for k in ("pred", "gt", "q", "idx", "dst") if f"{k}_{n}" in z.files} for n in z["names"].tolist()}


def test_fixture_covers_the_branches(golden):
    assert len(golden) >= 12 and os.path.getsize(GOLDEN) < 200 * 1024
    shapes = {c["gt"].shape for c in golden.values()}
    assert any(h != w for h, w in shapes) and all(max(s) <= 96 for s in shapes)
    fg = {n: (c["gt"] > 128) for n, c in golden.items()}
    assert any(m.all() for m in fg.values()) and any(not m.any() for m in fg.values())
    assert any(c["pred"].min() == c["pred"].max() for c in golden.values())


def test_transform_equals_scipy_on_fixture(golden):
    for name, c in golden.items():
        mask = c["gt"] > 128
        d2, index = R.edt_nearest(mask)
        if not mask.any():                                      # scipy is never asked: the package scores such an image 0
            assert (d2 == -1).all() and (index == -1).all(), name
            continue
        W = mask.shape[1]
        assert np.array_equal(index, c["idx"][0].astype(np.int32) * W + c["idx"][1]), name
        assert np.array_equal(np.sqrt(d2.astype(np.float64)), c["dst"]), name


def test_q_equals_scipy_formula_on_fixture(golden):
    for name, c in golden.items():
        got = R.step(c["pred"], c["gt"])
        assert abs(got - float(c["q"])) <= TOL, (name, got, float(c["q"]))
    assert R.step(golden["empty_gt"]["pred"], golden["empty_gt"]["gt"]) == 0.0
    assert 0.0 < float(golden["rectangles"]["q"]) < 1.0


def test_perfect_prediction_scores_one():
    gt = np.zeros((40, 52), np.uint8)
    gt[10:30, 5:25] = 255
    assert R.step(gt, gt) == pytest.approx(1.0, abs=1e-15)


def test_transform_equals_live_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    for k in range(300):
        H, W = int(rng.integers(1, 49)), int(rng.integers(1, 49))
        kind = k % 3
        if kind == 0:
            mask = rng.random((H, W)) < rng.choice([0.002, 0.02, 0.1, 0.5, 0.9])
        elif kind == 1:
            mask = np.zeros((H, W), bool)
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            mask[y0:y0 + int(rng.integers(1, H + 1)), x0:x0 + int(rng.integers(1, W + 1))] = True
        else:
            yy, xx = np.mgrid[:H, :W]
            p = int(rng.integers(1, 5))
            mask = ((yy // p + xx // p) % 2) == 0
        if not mask.any():
            mask[int(rng.integers(0, H)), int(rng.integers(0, W))] = True
        dst, idx = ndimage.distance_transform_edt(~mask, return_indices=True)
        d2, index = R.edt_nearest(mask)
        assert np.array_equal(index, idx[0] * W + idx[1]), (k, H, W)
        assert np.array_equal(np.sqrt(d2.astype(np.float64)), dst), (k, H, W)


def test_chunked_transform_equals_unchunked(monkeypatch):
    rng = np.random.default_rng(8)
    mask = rng.random((23, 41)) < 0.03
    want = R.edt_nearest(mask)
    monkeypatch.setattr(R, "_CHUNK", 41 * 7)                   # several x blocks and single-row blocks
    got = R.edt_nearest(mask)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_wrapper_running_values():
    rng = np.random.default_rng(2)
    w = R.Wrapper()
    batches = [(rng.random((1, 12, 10)), rng.random((1, 12, 10)) > 0.6), (rng.random((3, 12, 10)), rng.random((3, 12, 10)) > 0.5)]
    for p, g in batches:
        w.process(p.astype(np.float32), g.astype(np.float32))
    first = R.per_image(batches[0][0][0].astype(np.float32), batches[0][1][0].astype(np.float32))
    assert w.results[0] == first and len(w.results) == 2 and len(w.wfms) == 4
    assert w.compute_metrics()["WeightedFmeasure"] == pytest.approx((w.results[0] + np.mean(w.wfms)) / 2)
    assert w.summary()["wFmeasure"] == pytest.approx(np.mean(w.wfms))


# ---------------------------------------------------------------------------------------------------------------- evaluator wiring
VAL = [{"type": "Emeasure"}, {"type": "Fmeasure"}, {"type": "Smeasure"}, {"type": "WeightedFmeasure"}, {"type": "MAE"}]


def test_build_evaluators_builds_weighted_fmeasure():
    import dgtd
    logs = []
    ev = dgtd.runner.metrics.build_evaluators(VAL, logs.append, sod_metrics="device")
    assert [type(e).__name__ for e in ev] == ["Emeasure", "Fmeasure", "Smeasure", "WeightedFmeasure", "MAE"]
    assert [e.name for e in ev] == ["Emeasure", "Fmeasure", "Smeasure", "WeightedFmeasure", "MAE"]
    assert not logs
    assert isinstance(ev[3], dgtd.runner.sod_metrics.WeightedFmeasure)
    assert ev[0].acc is ev[1].acc is ev[2].acc is ev[3].acc and ev[0].acc.wfm is ev[3]
    assert ev[3].compute_metrics() == {"WeightedFmeasure": 0.0}          # nothing processed yet: no device touched
    assert ev[3].summary() == {} and ev[0].summary() == {}
    ev[3].reset()
    alone = dgtd.runner.metrics.build_evaluators([{"type": "WeightedFmeasure"}], logs.append, sod_metrics="device")
    assert [e.name for e in alone] == ["WeightedFmeasure"] and not logs


def test_weighted_fmeasure_still_skipped_by_default():
    import dgtd
    logs = []
    ev = dgtd.runner.metrics.build_evaluators(VAL, logs.append)
    assert [type(e).__name__ for e in ev] == ["MAE"]
    assert sum("WeightedFmeasure" in m and "skipped" in m for m in logs) == 1 and len(logs) == 4
    three = dgtd.runner.metrics.build_evaluators(VAL[:3], logs.append, sod_metrics="device")
    assert three[0].acc.wfm is None                             # summary() gains wFmeasure only when the evaluator is configured
