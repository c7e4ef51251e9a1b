"""GPU: validation at each image's own size (``val_cfg: {score_size: original}``): DeviceLoader(with_gt8=True) delivers the packed GT
planes, Runner.validate scores the bytes of ops.predict_maps against them through dgtd_sod_metrics_ragged, the same pass can write the
PNGs, and runner.score_maps scores such a folder again.  A ``Tiny`` model stands in for cod (as in tests/test_sod_metrics_gpu.py)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _sod_metrics_ref as R
from _rgbd_folder import SIZES7, write_folder

pytestmark = pytest.mark.gpu
TOL = 1e-12
S = 64
STEMS = [f"{i:03d}" for i in range(len(SIZES7))]

YAML = """
train_cfg: {by_epoch: True, max_epochs: 1, val_interval: 0}
val_dataloader:
  batch_size: 3
  num_workers: 2
  sampler: {type: DefaultSampler, shuffle: False}
  dataset: {type: SOD_TEST, data_dir: %(root)s, depth_dir: depth, split: test, image_size: 64}
model: {type: cod, img_size: 64}
optim_wrapper:
  type: AmpOptimWrapper
  optimizer: {type: AdamW, lr: 0.0005, weight_decay: 0.1}
val_cfg: %(val_cfg)s
val_evaluator:
  - type: Emeasure
  - type: Fmeasure
  - type: Smeasure
  - type: MAE
"""


class Tiny(torch.nn.Module):
    """Stands in for cod: a logit map from the batch's image; mode='predict' is (sigmoid, label), mode='tensor' the logits."""
    img_size = S

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))

    def forward(self, raw, image, label, depth, mode="predict"):
        logits = (self.w * (image[:, :1] * 1.5 + image[:, 1:2])).contiguous()
        return logits if mode == "tensor" else (torch.sigmoid(logits), label)


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("sod7")
    return root, write_folder(root, "RGB", "depth", sizes=SIZES7)


def make_runner(dgtd, root, tmp_path, monkeypatch, val_cfg="{sod_metrics: device}"):
    monkeypatch.setattr(dgtd.runner.config, "build_model", lambda cfg, dt: Tiny())
    return dgtd.runner.Runner(dgtd.runner.load_config(YAML % {"root": str(root), "val_cfg": val_cfg}), device="cuda", compute_dtype=torch.float32,
                              work_dir=str(tmp_path / "work"), log=lambda *a: None, seed=0)


def test_loader_delivers_the_gt_planes_packed_at_their_own_size(dgtd, folder, tmp_path, monkeypatch):
    root, arrays = folder
    r = make_runner(dgtd, root, tmp_path, monkeypatch)
    ds = r.build_dataset("val")
    sampler = dgtd.runner.DefaultSampler(len(ds), shuffle=False)
    for prefetch in (True, False):
        loader = dgtd.runner.DeviceLoader(ds, sampler, 3, "cuda", num_workers=2, prefetch=prefetch, with_gt8=True)
        try:
            held = list(loader)                                    # every batch of the epoch is held, then compared
        finally:
            loader.close()
        torch.cuda.synchronize()
        assert [len(b["raw"]) for b in held] == [3, 3, 1]
        i = 0
        for b in held:
            assert set(b) == {"raw", "input", "label", "depth", "size", "gt8"}
            offsets, total = dgtd._lib.predict_maps_layout(b["size"])
            assert b["gt8"].dtype == torch.uint8 and b["gt8"].is_cuda and b["gt8"].shape == (total,)
            host = b["gt8"].cpu().numpy()
            for (h, w), off in zip(b["size"], offsets):
                assert (h, w) == SIZES7[i]
                assert np.array_equal(host[off:off + h * w].reshape(h, w), arrays[i][1]), (prefetch, i)
                i += 1
        assert i == len(SIZES7)
    plain = dgtd.runner.DeviceLoader(ds, sampler, 3, "cuda", num_workers=2)
    try:
        assert all(set(b) == {"raw", "input", "label", "depth"} for b in plain)
    finally:
        plain.close()


def restated_pass(dgtd, r, arrays, minmax=False):
    """(compute_metrics, summary, {stem: bytes}) of the restated wrappers over ops.predict_maps bytes copied back and the GT arrays."""
    ds = r.build_dataset("val")
    loader = dgtd.runner.DeviceLoader(ds, dgtd.runner.DefaultSampler(len(ds), shuffle=False), 3, "cuda", num_workers=2, with_sizes=True)
    w, maps, i = R.Wrappers(), {}, 0
    r.model.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                logits = r.model(batch["raw"], batch["input"], batch["label"], batch["depth"], mode="tensor")
                packed, offsets = dgtd.ops.predict_maps(logits, batch["size"], minmax=minmax)
                host = packed.cpu().numpy()
                for (h, wd), off in zip(batch["size"], offsets):
                    p8 = host[off:off + h * wd].reshape(h, wd).copy()
                    maps[STEMS[i]] = p8
                    for m in (w.S, w.E, w.F, w.M):
                        m.step(p8, arrays[i][1])
                    i += 1
                w.results["Smeasure"].append(w.S.get_results()["sm"])
                w.results["Emeasure"].append(w.E.get_results()["em"]["curve"].max())
                w.results["Fmeasure"].append(w.F.get_results()["fm"]["curve"].max())
                w.results["MAE"].append(w.M.get_results()["mae"])
    finally:
        loader.close()
        r.model.train()
    return w.compute_metrics(), w.summary(), maps


def test_validate_config_at_the_original_size_matches_the_restatement(dgtd, folder, tmp_path, monkeypatch):
    root, arrays = folder
    r = make_runner(dgtd, root, tmp_path, monkeypatch, "{sod_metrics: device, score_size: original}")
    assert r.score_size == "original"
    got = r.validate_config()
    summary = r.evaluators[0].summary()
    want, want_s, _ = restated_pass(dgtd, r, arrays)
    assert set(got) == set(want) == {"Emeasure", "Fmeasure", "Smeasure", "MAE"}
    for k in want:
        print(k, got[k], want[k])
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    assert set(summary) == set(want_s)
    for k in want_s:
        assert abs(summary[k] - want_s[k]) <= TOL, (k, summary[k], want_s[k])
    assert r.validate_config() == got                                        # a second pass after reset() returns the same dict
    net = make_runner(dgtd, root, tmp_path, monkeypatch).validate_config()    # the same weights and data, scored at the network size
    assert set(net) == set(got) and all(net[k] != got[k] for k in got)


def test_one_pass_writes_the_folder_and_scores_it(dgtd, folder, tmp_path, monkeypatch):
    root, arrays = folder
    out_dir = tmp_path / "maps"
    r = make_runner(dgtd, root, tmp_path, monkeypatch, "{sod_metrics: device, score_size: original, save_maps: {out_dir: %s, normalize: minmax}}" % out_dir)
    calls = []
    real = dgtd._lib.call
    monkeypatch.setattr(dgtd._lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    got = r.validate_config()
    monkeypatch.setattr(dgtd._lib, "call", real)
    assert calls.count("dgtd_predict_maps") == 3 and calls.count("dgtd_sod_metrics_ragged") == 3       # one of each per batch: shared bytes
    summary = r.evaluators[0].summary()
    want, want_s, maps = restated_pass(dgtd, r, arrays, minmax=True)
    assert sorted(os.listdir(out_dir)) == [s + ".png" for s in STEMS]
    for stem, (h, w) in zip(STEMS, SIZES7):
        with Image.open(os.path.join(out_dir, stem + ".png")) as im:
            assert im.mode == "L" and im.size == (w, h)
            assert np.array_equal(np.asarray(im), maps[stem]), stem          # the PNGs hold the scored bytes
    for k in want:
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    again = dgtd.runner.score_maps(str(out_dir), os.path.join(str(root), "GT"), batch=4, workers=2)
    assert again == summary                                                  # the same bytes in the same order: equal, not close
    assert dgtd.runner.score_maps(str(out_dir), os.path.join(str(root), "GT")) == summary


def test_default_is_what_it_was(dgtd, folder, tmp_path, monkeypatch):
    root, _ = folder
    r = make_runner(dgtd, root, tmp_path, monkeypatch)
    assert r.score_size == "network"
    calls, keys = [], []
    real = dgtd._lib.call
    monkeypatch.setattr(dgtd._lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    process = r.evaluators[0].process
    monkeypatch.setattr(r.evaluators[0], "process", lambda batch, out: (keys.append(set(batch)), process(batch, out))[1])
    r.validate_config()
    metric_calls = [c for c in calls if "sod_metrics" in c or "predict_maps" in c]
    assert metric_calls == ["dgtd_sod_metrics", "dgtd_sod_metrics_accumulate"] * 3
    assert keys == [{"raw", "input", "label", "depth"}] * 3
