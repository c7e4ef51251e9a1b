"""GPU: Runner.predict / predict_config -> runner.predict.MapWriter: one PNG per image of a folder dataset, named by the image's stem,
at the GT's own size, holding exactly the bytes of ops.predict_maps applied to cod.forward(mode='tensor') of the same batch."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from _rgbd_folder import SIZES7, write_folder

pytestmark = pytest.mark.gpu
S = 64
SIZES5 = SIZES7[:4] + [(64, 64)]      # five images of different sizes; batch 2 leaves a partial last batch

YAML = """
train_cfg: {by_epoch: True, max_epochs: 1, val_interval: 0}
train_dataloader:
  batch_size: 2
  num_workers: 2
  sampler: {type: DefaultSampler, shuffle: True}
  dataset: {type: SOD_TRAIN, data_dir: %(root)s, depth_dir: depth, split: train, image_size: 64}
val_dataloader:
  batch_size: 2
  num_workers: 2
  sampler: {type: DefaultSampler, shuffle: False}
  dataset: {type: SOD_TEST, data_dir: %(root)s, depth_dir: depth, split: test, image_size: 64}
model: {type: cod, img_size: 64, drop_path_rate: 0.0}
optim_wrapper:
  type: AmpOptimWrapper
  optimizer: {type: AdamW, lr: 0.0005, weight_decay: 0.1}
val_evaluator:
  - type: MAE
%(extra)s
"""


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    root = tmp_path_factory.mktemp("sod5")
    write_folder(root, "RGB", "depth", sizes=SIZES5, names=["ant", "bee.v2", "cat", "dog", "eel"])
    return root


def make_runner(dgtd, root, tmp_path, extra=""):
    torch.manual_seed(0)
    return dgtd.runner.Runner(dgtd.runner.load_config(YAML % {"root": str(root), "extra": extra}), device="cuda", compute_dtype=torch.float32,
                              work_dir=str(tmp_path / "work"), log=lambda *a: None, seed=0)


def expected_maps(dgtd, r, minmax=False):
    """{stem: uint8 [H, W]} from the op applied to mode='tensor' of the same batches, with the weights the model holds now."""
    ds = r.build_dataset("val")
    loader = dgtd.runner.DeviceLoader(ds, dgtd.runner.DefaultSampler(len(ds), shuffle=False), 2, "cuda", num_workers=2, with_sizes=True)
    want, was = {}, r.model.training
    r.model.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                assert set(batch) == {"raw", "input", "label", "depth", "size"}
                logits = r.model(batch["raw"], batch["input"], batch["label"], batch["depth"], mode="tensor")
                assert logits.shape == (len(batch["raw"]), 1, S, S)
                packed, offsets = dgtd.ops.predict_maps(logits, batch["size"], minmax=minmax)
                host = packed.cpu().numpy()
                for raw, (h, w), off in zip(batch["raw"], batch["size"], offsets):
                    want[os.path.splitext(os.path.basename(raw))[0]] = host[off:off + h * w].reshape(h, w).copy()
    finally:
        loader.close()
        r.model.train(was)
    return want


def check_folder(out_dir, paths, want):
    stems = ["ant", "bee.v2", "cat", "dog", "eel"]
    assert [os.path.basename(p) for p in paths] == [s + ".png" for s in stems]
    assert sorted(os.listdir(out_dir)) == sorted(s + ".png" for s in stems)       # five PNGs, no *.tmp left behind
    for stem, (h, w) in zip(stems, SIZES5):
        with Image.open(os.path.join(out_dir, stem + ".png")) as im:
            assert im.mode == "L" and im.size == (w, h), stem                     # the GT's own (W, H)
            assert np.array_equal(np.asarray(im), want[stem]), stem


def test_predict_config_writes_one_png_per_image_at_its_own_size(dgtd, root, tmp_path, monkeypatch):
    r = make_runner(dgtd, root, tmp_path)
    # the four keys of today with the default, and mode='predict' before the call
    ds = r.build_dataset("val")
    plain = dgtd.runner.DeviceLoader(ds, dgtd.runner.DefaultSampler(len(ds), shuffle=False), 2, "cuda", num_workers=2)
    try:
        first = next(iter(plain))
    finally:
        plain.close()
    assert set(first) == {"raw", "input", "label", "depth"}
    r.model.eval()
    with torch.no_grad():
        before = r.model(first["raw"], first["input"], first["label"], first["depth"], mode="predict")
        logits = r.model(first["raw"], first["input"], first["label"], first["depth"], mode="tensor")
    assert logits.shape == (2, 1, S, S) and logits.dtype == before[0].dtype
    assert torch.allclose(logits.sigmoid(), before[0], rtol=0.0, atol=1e-6)       # tensor = logit(predict) up to sigmoid's rounding
    r.model.train()
    # one entry call and one device-to-host copy per batch, counted at their boundaries
    L, W = dgtd._lib, dgtd.runner.MapWriter
    calls, copies = [], []
    real_call, real_copy = L.call, W._to_host
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(W, "_to_host", staticmethod(lambda pinned, packed: (copies.append(packed.numel()), real_copy(pinned, packed))[1]))
    out_dir = tmp_path / "maps"
    paths = r.predict_config("val", out_dir=str(out_dir))
    monkeypatch.undo()
    assert calls.count("dgtd_predict_maps") == 3 and len(copies) == 3             # batches of 2, 2 and 1
    assert r.model.training and r._device_loaders == {}
    check_folder(out_dir, paths, expected_maps(dgtd, r))
    r.model.eval()
    with torch.no_grad():
        after = r.model(first["raw"], first["input"], first["label"], first["depth"], mode="predict")
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])  # predict mode is what it was
    # validate's loader still yields the four keys after predict_config asked the same runner for sizes
    assert "size" not in next(iter(r.loader(r.build_dataset("val"), "val")))
    r.close()


def test_predict_without_sizes_writes_at_the_models_size(dgtd, root, tmp_path):
    r = make_runner(dgtd, root, tmp_path)
    data = dgtd.runner.SyntheticRGBD(S, 2, length=3)
    batches = list(dgtd.runner.batches(data, dgtd.runner.DefaultSampler(3, shuffle=False), 2, "cuda"))
    paths = r.predict(batches, str(tmp_path / "synthetic"))
    assert [os.path.basename(p) for p in paths] == ["0.png", "1.png", "2.png"]
    for p in paths:
        with Image.open(p) as im:
            assert im.mode == "L" and im.size == (S, S)


def test_with_ema_the_maps_come_from_the_averaged_weights(dgtd, root, tmp_path):
    extra = ("custom_hooks:\n  - {type: EMAHook, momentum: 0.5}\n"
             "val_cfg: {save_maps: {out_dir: %s, normalize: minmax}}\n" % str(tmp_path / "ema_maps"))
    r = make_runner(dgtd, root, tmp_path, extra)
    r.fit()                                                                       # three steps: the average now differs from the weights
    raw = {k: v.clone() for k, v in r.model.state_dict().items()}
    paths = r.predict_config()                                                    # out_dir and min-max from val_cfg.save_maps
    assert all(torch.equal(v, raw[k]) for k, v in r.model.state_dict().items())   # the raw weights are back in place
    with_raw = expected_maps(dgtd, r, minmax=True)
    r.swap_ema()
    try:
        with_avg = expected_maps(dgtd, r, minmax=True)
    finally:
        r.swap_ema()
    assert any(not np.array_equal(with_raw[k], with_avg[k]) for k in with_raw)    # the two sets of weights give different maps
    check_folder(tmp_path / "ema_maps", paths, with_avg)
