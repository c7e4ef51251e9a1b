"""CPU: the folder datasets of runner/datasets.py (the reference's twig/dataset classes), their host path against the numpy
restatement of the transform chain, the flip coin, the job layout of dgtd_preprocess_batch, and the Runner building them from YAML."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import preprocess_cpu as pc
from _rgbd_folder import SIZES7, write_folder


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    return m


@pytest.fixture(scope="module")
def D(dgtd):
    return dgtd.runner.datasets


# (class, image dir, default size, prefix, split to build with)
TABLE = [("SOD_TRAIN", "RGB", 384, (), "train"), ("COD10K_CAMO_TRAIN", "Imgs", 384, (), "train"), ("SOD_TEST", "RGB", 384, (), "test"),
         ("COD10K_TEST", "Image", 384, (), "test"), ("COD_TEST", "Image", 704, (), "val"), ("CHAMELEON", "Image", 704, (), "test"),
         ("NC4K", "Image", 704, ("train",), "test")]


@pytest.mark.parametrize("name,image_dir,size,prefix,split", TABLE, ids=[t[0] for t in TABLE])
def test_every_class_finds_its_directories_sorted(dgtd, D, tmp_path, name, image_dir, size, prefix, split):
    names = ["b", "a", "c"]                                   # written out of order: the lists come back sorted
    write_folder(tmp_path, image_dir, "dep", prefix, sizes=[(8, 9), (5, 6), (7, 7)], names=names)
    cls = dgtd.runner.registry.get(name)
    assert cls is getattr(D, name)
    if name == "COD10K_TEST":
        assert cls.SKIP == 3381
        cls = type("COD10K_TEST_SHORT", (cls,), {"SKIP": 0})
    ds = cls(str(tmp_path), "dep", split)
    assert len(ds) == 3 and ds.image_size == size
    base = os.path.join(str(tmp_path), *prefix)
    assert ds.images == [os.path.join(base, image_dir, n + ".png") for n in "abc"]
    assert ds.gts == [os.path.join(base, "GT", n + ".png") for n in "abc"]
    assert ds.depth == [os.path.join(base, "dep", n + ".png") for n in "abc"]
    rgb, gt, dep, flip = ds.decode(0)
    assert rgb.shape == (5, 6, 3) and gt.shape == (5, 6) and dep.shape == (5, 6) and all(a.dtype == np.uint8 for a in (rgb, gt, dep))
    assert ds[1]["raw"] == ds.images[1]                      # raw is the path in every class


def test_cod10k_test_slices_the_sorted_lists_before_filtering(D, tmp_path):
    write_folder(tmp_path, "Image", "dep", sizes=[(6, 6)] * 5, gt_sizes={3: (6, 7)})
    cls = type("COD10K_TEST_2", (D.COD10K_TEST,), {"SKIP": 2})
    ds = cls(str(tmp_path), "dep", "test")
    assert [os.path.basename(p) for p in ds.images] == ["002.png", "004.png"]          # [2:], then 003 filtered out
    assert [os.path.basename(p) for p in ds.depth] == ["002.png", "004.png"]
    with pytest.raises(FileNotFoundError):
        D.COD10K_TEST(str(tmp_path / "nowhere"), "dep", "test")


def test_split_errors(D, tmp_path):
    write_folder(tmp_path, "RGB", "dep", sizes=[(6, 6)])
    write_folder(tmp_path, "Imgs", "dep", sizes=[(6, 6)])
    for split in ("train", "test", "val", "anything"):       # the reference's train classes take `if True:`
        assert len(D.SOD_TRAIN(str(tmp_path), "dep", split)) == 1
        assert len(D.COD10K_CAMO_TRAIN(str(tmp_path), "dep", split)) == 1
    for cls in (D.SOD_TEST, D.COD10K_TEST, D.COD_TEST, D.CHAMELEON, D.NC4K):
        with pytest.raises(ValueError):
            cls(str(tmp_path), "dep", "train")
        with pytest.raises(NotImplementedError):
            cls(str(tmp_path), "dep", "predict")
    assert len(D.SOD_TEST(str(tmp_path), "dep", "val")) == 1 and len(D.SOD_TEST(str(tmp_path), "dep", "test")) == 1


def test_size_mismatch_drops_the_whole_triple_and_unequal_lists_raise(D, tmp_path):
    write_folder(tmp_path / "a", "RGB", "dep", sizes=[(6, 6), (8, 8), (6, 9), (5, 5)], gt_sizes={1: (8, 7)})
    ds = D.SOD_TRAIN(str(tmp_path / "a"), "dep", "train")
    want = ["000.png", "002.png", "003.png"]
    for lst in (ds.images, ds.gts, ds.depth):                 # the depth list stays in step (the reference's does not)
        assert [os.path.basename(p) for p in lst] == want
    assert ds.decode(1)[2].shape == (6, 9)
    os.remove(ds.depth[0])
    with pytest.raises(ValueError, match="dep") as e:
        D.SOD_TRAIN(str(tmp_path / "a"), "dep", "train")
    assert "RGB" in str(e.value) and "GT" in str(e.value)


def test_image_size_argument(D, tmp_path):
    write_folder(tmp_path, "RGB", "dep", sizes=[(6, 6)])
    mk = lambda s: D.SOD_TRAIN(str(tmp_path), "dep", "train", s)
    assert mk(None).image_size == 384 and mk(64).image_size == 64 and mk([96, 96]).image_size == 96 and mk((32, 32)).image_size == 32
    for bad in (50, [64, 96], 0, [64]):
        with pytest.raises(ValueError):
            mk(bad)


@pytest.fixture(scope="module")
def folder7(tmp_path_factory):
    root = tmp_path_factory.mktemp("sod7")
    return str(root), write_folder(root, "RGB", "depth", jpeg=4)


@pytest.mark.parametrize("S", [64, 32])
def test_getitem_equals_the_numpy_restatement_bit_for_bit(D, folder7, S):
    """Down-scales, an up-scale ((20,30) -> 64), a 1-pixel-high image and a decoded JPEG; flipped and not."""
    root, arrays = folder7
    for cls, split in ((D.SOD_TRAIN, "train"), (D.SOD_TEST, "test")):
        ds = cls(root, "depth", split, S)
        assert len(ds) == len(SIZES7)
        flips = []
        for i, (rgb, gt, dep) in enumerate(arrays):
            r, g, d, flip = ds.decode(i, 0)
            assert np.array_equal(r, rgb) and np.array_equal(g, gt) and np.array_equal(d, dep)
            flips.append(flip)
            it = ds[i]
            assert set(it) == {"raw", "input", "label", "depth"} and it["raw"] == ds.images[i]
            for key, arr, c in (("input", rgb, 3), ("label", gt, 1), ("depth", dep, 1)):
                t = it[key]
                assert t.shape == (c, S, S) and t.dtype == torch.float32 and t.device.type == "cpu" and torch.isfinite(t).all()
                assert np.array_equal(t.numpy(), pc.preprocess(arr, S, normalize=(key == "input"), flip=flip)), (i, key)
            assert 0.0 <= float(it["label"].min()) and float(it["label"].max()) <= 1.0
            assert 0.0 <= float(it["depth"].min()) and float(it["depth"].max()) <= 1.0
            lo, hi = (0 - 0.485) / 0.229, (1 - 0.406) / 0.225
            assert lo - 1e-5 <= float(it["input"].min()) and float(it["input"].max()) <= hi + 1e-5
        if cls is D.SOD_TEST:                                                     # test classes never flip
            assert not any(flips)
            assert not any(ds.flip(i, e) for i in range(len(ds)) for e in range(8))


def test_flip_coin(D, folder7):
    root, arrays = folder7
    coin = D.flip_coin
    assert [coin(0, 0, i) for i in range(64)] == [coin(0, 0, i) for i in range(64)]               # a pure function
    assert any(coin(0, 0, i) != coin(0, 1, i) for i in range(64))                                  # changes with the epoch
    assert any(coin(0, 0, i) != coin(1, 0, i) for i in range(64))                                  # and with the seed
    for seed, epoch in ((0, 0), (0, 1), (3, 7), (1234, 49)):
        share = sum(coin(seed, epoch, i) for i in range(1000)) / 1000.0
        assert 0.4 <= share <= 0.6, (seed, epoch, share)       # binomial sd 0.016: six deviations wide
    # no rank enters: both ranks of a 2-rank sampler that draw the same index see the same sample
    import dgtd
    ds = D.SOD_TRAIN(root, "depth", "train", 32)
    ds.seed = 5
    seen = {}
    for rank in (0, 1):
        s = dgtd.runner.DefaultSampler(len(ds), shuffle=True, seed=5, rank=rank, world=2)
        s.set_epoch(2)
        for i in s:
            f = ds.decode(i, s.epoch)[3]
            assert seen.setdefault(i, f) == f and f == coin(5, 2, i)
    assert len(seen) == len(ds)
    # one coin for image, GT and depth; a flipped sample is the unflipped one mirrored BEFORE the resize
    ds.set_epoch(2)
    flipped = [i for i in range(len(ds)) if coin(5, 2, i)]
    plain = [i for i in range(len(ds)) if not coin(5, 2, i)]
    assert flipped and plain
    for i in flipped[:2]:
        rgb, gt, dep = arrays[i]
        it = ds[i]
        assert np.array_equal(it["input"].numpy(), pc.preprocess(np.ascontiguousarray(rgb[:, ::-1]), 32, True, flip=False))
        assert np.array_equal(it["label"].numpy(), pc.preprocess(np.ascontiguousarray(gt[:, ::-1]), 32, False, flip=False))
        assert np.array_equal(it["depth"].numpy(), pc.preprocess(np.ascontiguousarray(dep[:, ::-1]), 32, False, flip=False))
    i = plain[0]
    assert np.array_equal(ds[i]["input"].numpy(), pc.preprocess(arrays[i][0], 32, True, flip=False))


def test_job_layout_is_aligned_disjoint_and_covered(dgtd):
    """Pure host arithmetic: no library call (LIB_PATH is not even consulted)."""
    L = dgtd._lib
    import ctypes
    assert ctypes.sizeof(L.PreprocessJob) == 64
    assert [L.resize_ksize(i, o) for i, o in ((30, 64), (64, 64), (65, 64), (128, 64), (400, 64), (1, 48))] == [3, 3, 5, 5, 15, 3]
    for i, o in ((97, 64), (131, 64), (300, 64), (400, 384), (7, 7), (1000, 3)):
        assert L.resize_ksize(i, o) == int(math.ceil(max(i / o, 1.0))) * 2 + 1                     # Pillow's form
    shapes = [(97, 131, 3), (20, 30, 1), (1, 7, 1), (50, 33, 3), (300, 400, 1)]
    for S in (64, 48):
        lay = L.preprocess_batch_layout(shapes, S)
        planes = [(o, h * w * c) for o, (h, w, c) in zip(lay["src"], shapes)]
        regions = []
        for j, (h, w, c) in enumerate(shapes):
            regions += [(lay["mid"][j], h * S * c), (lay["tab_h"][j], S * (2 + L.resize_ksize(w, S)) * 4),
                        (lay["tab_v"][j], S * (2 + L.resize_ksize(h, S)) * 4)]
        for group, total in ((planes, lay["planes_bytes"]), (regions, lay["workspace_bytes"])):
            assert all(o % 16 == 0 and n > 0 for o, n in group)
            srt = sorted(group)
            assert all(a + n <= b for (a, n), (b, _) in zip(srt, srt[1:]))                          # no overlap
            assert srt[0][0] == 0 and srt[-1][0] + srt[-1][1] <= total <= srt[-1][0] + srt[-1][1] + 15
        table = (L.PreprocessJob * len(shapes))()
        L.fill_preprocess_jobs(table, shapes, lay, [j % 2 for j in range(5)], [c == 3 for _, _, c in shapes], [0 if c == 3 else 1 for _, _, c in shapes],
                               [0, 0, 1, 1, 2])
        assert [(t.H, t.W, t.C, t.flip, t.normalize, t.out_sel, t.batch) for t in table][3] == (50, 33, 3, 1, 1, 0, 1)
        assert [t.src_off for t in table] == lay["src"] and [t.tab_v_off for t in table] == lay["tab_v"]
    for bad in ([(0, 5, 3)], [(5, 5, 2)], []):
        with pytest.raises(L.DgtdError):
            L.preprocess_batch_layout(bad, 64)


# ---------------------------------------------------------------------------------------------------------------- the runner on CPU
YAML = """
train_cfg: {by_epoch: True, max_epochs: 1}
train_dataloader:
  batch_size: 2
  num_workers: 2
  sampler: {type: DefaultSampler, shuffle: True}
  dataset: {type: %s, data_dir: %s, depth_dir: depth, split: train, image_size: %d}
val_dataloader:
  batch_size: 1
  dataset: {type: SOD_TEST, data_dir: %s, depth_dir: depth, split: test, image_size: 32}
model: {type: ds_tiny, img_size: 32}
optim_wrapper:
  optimizer: {type: AdamW, lr: 0.01, weight_decay: 0.0}
"""


class Tiny(torch.nn.Module):
    def __init__(self, img_size=32, compute_dtype=torch.float32):
        super().__init__()
        self.img_size = img_size
        self.conv = torch.nn.Conv2d(4, 1, 3, padding=1)
        self.seen = []

    def forward(self, raw, input, label, depth, mode="loss"):
        x, l, d = (torch.stack(list(t)) if isinstance(t, (list, tuple)) else t for t in (input, label, depth))
        self.seen.append((list(raw), x.clone(), l.clone(), d.clone()))
        y = self.conv(torch.cat([x, d], 1))
        return {"loss": ((y - l) ** 2).mean()} if mode == "loss" else (y.sigmoid(), l)


@pytest.fixture
def tiny_registered(dgtd):
    dgtd.runner.register_model(Tiny, name="ds_tiny")
    yield
    dgtd.runner.registry.REGISTRY.pop("ds_tiny", None)
    dgtd.runner.config.MODEL_REGISTRY.pop("ds_tiny", None)


def test_runner_builds_datasets_from_yaml_and_fits_on_cpu(dgtd, D, tiny_registered, tmp_path):
    write_folder(tmp_path / "data", "RGB", "depth", sizes=SIZES7[:4])
    root = str(tmp_path / "data")
    mk = lambda typ="SOD_TRAIN", size=32: dgtd.runner.Runner(dgtd.runner.load_config(YAML % (typ, root, size, root)), device="cpu",
                                                             compute_dtype=torch.float32, work_dir=str(tmp_path / "work"), log=lambda m: None, seed=4)
    r = mk()
    ds = r.build_dataset("train")
    assert isinstance(ds, D.SOD_TRAIN) and len(ds) == 4 and ds.image_size == 32 and ds.seed == 4
    assert isinstance(r.build_dataset("val"), D.SOD_TEST)
    losses = r.fit()                                           # 4 images, batch 2, one epoch, through batches(...)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    raw, x, l, d = r.model.seen[0]
    s = dgtd.runner.DefaultSampler(4, shuffle=True, seed=4)
    first = list(s)[:2]
    assert raw == [ds.images[i] for i in first]
    assert torch.equal(x, torch.stack([ds[i]["input"] for i in first])) and torch.equal(d, torch.stack([ds[i]["depth"] for i in first]))
    assert os.path.exists(tmp_path / "work" / "epoch_1.pth")
    with pytest.raises(KeyError, match="SOD_TRAIN"):           # the message lists what IS registered
        mk("NO_SUCH_SET").build_dataset("train")
    with pytest.raises(ValueError, match="img_size"):
        mk(size=64).fit()
    # SyntheticRGBD still builds through the same registry
    cfg = dgtd.runner.load_config(YAML % ("SOD_TRAIN", root, 32, root))
    cfg["train_dataloader"]["dataset"] = {"type": "SyntheticRGBD", "size": 32, "batch": 2, "device": "cpu", "length": 4}
    r2 = dgtd.runner.Runner(cfg, device="cpu", compute_dtype=torch.float32, work_dir=str(tmp_path / "w2"), log=lambda m: None)
    assert isinstance(r2.build_dataset("train"), dgtd.runner.SyntheticRGBD) and len(r2.fit()) == 2
