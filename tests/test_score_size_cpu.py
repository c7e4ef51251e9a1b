"""CPU: ``score_size`` parsing and every refusal of the own-size validation mode that needs no device, and the pairing errors of
runner.score_maps on a temporary folder."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

YAML = """
train_cfg: {by_epoch: True, max_epochs: 1, val_interval: 1}
val_cfg: %s
model: {type: cod}
optim_wrapper:
  type: AmpOptimWrapper
  optimizer: {type: AdamW, lr: 0.0005, weight_decay: 0.1}
val_evaluator:
%s
"""
SEFM = "  - type: Emeasure\n  - type: Fmeasure\n  - type: Smeasure\n  - type: MAE\n"


def make(monkeypatch, tmp_path, val_cfg, evaluators=SEFM, **kw):
    import dgtd
    cfgmod = dgtd.runner.config
    built = []
    monkeypatch.setattr(cfgmod, "build_model", lambda cfg, dt: (built.append(1), torch.nn.Linear(4, 4))[1])
    cfg = dgtd.runner.load_config(YAML % (val_cfg, evaluators))
    return (lambda: cfgmod.Runner(cfg, device="cpu", compute_dtype=torch.float32, work_dir=str(tmp_path), log=lambda m: None, **kw)), built


def test_score_size_is_read_from_the_yaml_and_the_keyword(monkeypatch, tmp_path):
    import dgtd
    mk, _ = make(monkeypatch, tmp_path, "{sod_metrics: device}")
    r = mk()
    assert r.score_size == "network" and type(r.evaluators[3]) is dgtd.runner.metrics.MAE          # the default is today's wiring
    mk, _ = make(monkeypatch, tmp_path, "{sod_metrics: device, score_size: original}")
    r = mk()
    assert r.score_size == "original"
    assert [type(e).__name__ for e in r.evaluators] == ["Emeasure", "Fmeasure", "Smeasure", "MAE"]
    assert type(r.evaluators[3]) is dgtd.runner.sod_metrics.MAE and r.evaluators[3].acc is r.evaluators[0].acc   # one shared accumulator
    mk, _ = make(monkeypatch, tmp_path, "{sod_metrics: device}", score_size="original")
    assert mk().score_size == "original"
    mk, _ = make(monkeypatch, tmp_path, "{sod_metrics: device, score_size: network}")
    assert mk().score_size == "network"


@pytest.mark.parametrize("val_cfg,evaluators,kw,match", [
    ("{sod_metrics: device, score_size: orignal}", SEFM, {}, "score_size must be one of"),
    ("{sod_metrics: device}", SEFM, {"score_size": "full"}, "score_size must be one of"),
    ("{score_size: original}", SEFM, {}, "requires sod_metrics: device"),
    ("{sod_metrics: skip, score_size: original}", SEFM, {}, "requires sod_metrics: device"),
    ("{sod_metrics: device, score_size: original}", SEFM + "  - type: meanIntersectionOverUnion\n", {}, "network size only"),
    ("{sod_metrics: device, score_size: original}", SEFM + "  - type: BinaryMIoU\n", {}, "network size only"),
    ("{sod_metrics: device, score_size: original}", SEFM + "  - type: WeightedFmeasure\n", {}, "network size only"),
])
def test_bad_values_and_combinations_fail_before_the_model_is_built(monkeypatch, tmp_path, val_cfg, evaluators, kw, match):
    mk, built = make(monkeypatch, tmp_path, val_cfg, evaluators, **kw)
    with pytest.raises(ValueError, match=match):
        mk()
    assert built == []


def test_build_evaluators_checks_the_same_things():
    import dgtd
    be = dgtd.runner.metrics.build_evaluators
    with pytest.raises(ValueError, match="score_size must be one of"):
        be([{"type": "Smeasure"}], lambda m: None, sod_metrics="device", score_size="big")
    with pytest.raises(ValueError, match="requires sod_metrics: device"):
        be([{"type": "Smeasure"}], lambda m: None, score_size="original")
    with pytest.raises(ValueError, match="network size only"):
        be([{"type": "WeightedFmeasure"}], lambda m: None, sod_metrics="device", score_size="original")
    assert [type(e).__name__ for e in be([{"type": "MAE"}], lambda m: None, sod_metrics="device", score_size="original")] == ["MAE"]


@pytest.mark.parametrize("batch", [{"input": torch.zeros(1, 3, 4, 4), "label": None, "depth": None},
                                   {"input": torch.zeros(1, 3, 4, 4), "label": None, "depth": None, "size": [(4, 4)]},
                                   {"input": torch.zeros(1, 3, 4, 4), "label": None, "depth": None, "gt8": torch.zeros(16, dtype=torch.uint8)}])
def test_a_batch_without_gt8_or_size_names_the_loader_flag(monkeypatch, tmp_path, batch):
    mk, _ = make(monkeypatch, tmp_path, "{sod_metrics: device, score_size: original}")
    r = mk()
    with pytest.raises(ValueError, match=r"DeviceLoader\(with_gt8=True\)"):
        r.validate([batch])


def write(folder, stem, shape, ext=".png"):
    os.makedirs(folder, exist_ok=True)
    Image.fromarray(np.zeros(shape, np.uint8)).save(os.path.join(folder, stem + ext))


def test_score_maps_pairing_errors(tmp_path):
    import dgtd
    pred, gt = str(tmp_path / "pred"), str(tmp_path / "gt")
    for stem in ("a", "b", "c", "d"):
        write(gt, stem, (5, 7))
    write(pred, "a", (5, 7))
    write(pred, "c", (5, 7), ".jpg")
    write(pred, "zz", (5, 7))                                   # a map without a ground truth is not scored and no error
    with pytest.raises(FileNotFoundError, match="b, d"):
        dgtd.runner.score_maps(pred, gt)
    write(pred, "b", (5, 7))
    write(pred, "d", (7, 5))                                    # transposed: same pixel count, another size
    with pytest.raises(ValueError, match=r"d\.png is 7x5 .* is 5x7") as e:
        dgtd.runner.score_maps(pred, gt)
    assert "refuses" in str(e.value)
    os.makedirs(tmp_path / "empty")
    with pytest.raises(FileNotFoundError, match="no image files"):
        dgtd.runner.score_maps(pred, str(tmp_path / "empty"))
