"""GPU: runner.data.DeviceLoader (decode threads -> one pinned upload -> dgtd_preprocess_batch) against the datasets' host path
``ds[i]`` (PIL resize + ToTensor / Normalize), bit for bit, and the Runner training / validating from the YAML's dataset blocks."""
import math

import pytest
import torch

from _rgbd_folder import SIZES7, write_folder

pytestmark = pytest.mark.gpu
S = 64


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


@pytest.fixture(scope="module")
def folder(dgtd, tmp_path_factory):
    """Seven triples of different sizes (one image a JPEG) and the host path's tensors for epochs 0 and 1, computed once."""
    root = tmp_path_factory.mktemp("sod7")
    write_folder(root, "RGB", "depth", jpeg=4)
    ds = dgtd.runner.datasets.SOD_TRAIN(str(root), "depth", "train", S)
    assert len(ds) == len(SIZES7)
    host = {}
    for epoch in (0, 1):
        ds.set_epoch(epoch)
        host[epoch] = [ds[i] for i in range(len(ds))]
    flips = {e: [ds.flip(i, e) for i in range(len(ds))] for e in (0, 1)}
    assert all(any(f) and not all(f) for f in flips.values()) and flips[0] != flips[1]      # mixed within a batch, changing with the epoch
    return ds, host


def _check(batch, host, indices, dataset, dtype=torch.float32):
    assert batch["raw"] == [dataset.images[i] for i in indices]
    for key, c in (("input", 3), ("label", 1), ("depth", 1)):
        t = batch[key]
        assert t.shape == (len(indices), c, S, S) and t.dtype == dtype and t.is_cuda and t.is_contiguous()
        assert torch.equal(t.cpu(), torch.stack([host[i][key] for i in indices]).to(dtype)), key


@pytest.mark.parametrize("prefetch", [True, False])
def test_batches_equal_the_host_path_over_two_epochs(dgtd, folder, prefetch):
    ds, host = folder
    sampler = dgtd.runner.DefaultSampler(len(ds), shuffle=True, seed=1)
    loader = dgtd.runner.DeviceLoader(ds, sampler, 3, "cuda", torch.float32, num_workers=4, prefetch=prefetch)
    assert loader.num_threads == 4 and len(loader) == 3
    ptrs = None
    try:
        for epoch in (0, 1):
            sampler.set_epoch(epoch)
            order = list(sampler)
            got = list(loader)                                    # every batch of the epoch is held and compared AFTER the epoch ended
            torch.cuda.synchronize()
            assert [len(b["raw"]) for b in got] == [3, 3, 1]      # the last partial batch is yielded
            for k, b in enumerate(got):
                _check(b, host[epoch], order[3 * k:3 * k + 3], ds)
            now = [st.pinned.data_ptr() for st in loader.sets]    # both staging sets were used (3 batches) and are reused
            assert ptrs is None or now == ptrs
            ptrs = now
        assert len({b["input"].data_ptr() for b in got}) == 3     # the outputs are fresh tensors per batch, not views of a reused set
    finally:
        loader.close()


def test_drop_last_16_bit_and_the_thread_cap(dgtd, folder):
    ds, host = folder
    sampler = dgtd.runner.DefaultSampler(len(ds), shuffle=False)
    loader = dgtd.runner.DeviceLoader(ds, sampler, 3, "cuda", torch.bfloat16, num_workers=64, drop_last=True)
    try:
        assert loader.num_threads == 16 and len(loader) == 2
        got = list(loader)
        assert len(got) == 2
        for k, b in enumerate(got):
            _check(b, host[0], [3 * k, 3 * k + 1, 3 * k + 2], ds, torch.bfloat16)
    finally:
        loader.close()
    with pytest.raises(dgtd._lib.DgtdError):
        dgtd.runner.DeviceLoader(ds, sampler, 3, "cpu")
    with pytest.raises(TypeError):
        dgtd.runner.DeviceLoader(dgtd.runner.SyntheticRGBD(S, 2, length=4), sampler, 2, "cuda")


def test_one_entry_call_per_batch_and_nothing_per_sample(dgtd, folder):
    """The library's own call records: an epoch of three batches is three dgtd_preprocess_batch calls (three launches each,
    csrc/preprocess_batch.hip) over exactly the planes' bytes, and no per-sample dgtd_preprocess call."""
    ds, host = folder
    L = dgtd._lib
    loader = dgtd.runner.DeviceLoader(ds, dgtd.runner.DefaultSampler(len(ds), shuffle=False), 3, "cuda", num_workers=2)
    L.profile_native(True)
    try:
        got = list(loader)
        rec = L.profile_native_summary()
    finally:
        L.profile_native(False)
        loader.close()
    assert len(got) == 3 and sorted(rec) == ["dgtd_preprocess_batch[3x->64]", "dgtd_preprocess_batch[9x->64]"]
    assert rec["dgtd_preprocess_batch[9x->64]"]["calls"] == 2 and rec["dgtd_preprocess_batch[3x->64]"]["calls"] == 1
    want = sum(h * w * 5 for h, w in SIZES7) + 4 * 5 * len(SIZES7) * S * S          # uint8 planes in, fp32 batch tensors out
    assert sum(v["amount"] for v in rec.values()) == want


def test_two_ranks_cover_the_dataset_with_round_up_repetition(dgtd, folder):
    ds, host = folder
    raws = []
    for rank in (0, 1):
        sampler = dgtd.runner.DefaultSampler(len(ds), shuffle=False, rank=rank, world=2)
        loader = dgtd.runner.DeviceLoader(ds, sampler, 3, "cuda", num_workers=2)
        try:
            order, got = list(sampler), list(loader)
        finally:
            loader.close()
        assert order == ([0, 2, 4, 6] if rank == 0 else [1, 3, 5, 0])               # 7 -> 8 by repeating the start
        for k, b in enumerate(got):
            _check(b, host[0], order[3 * k:3 * k + 3], ds)
        raws.append([r for b in got for r in b["raw"]])
    assert set(raws[0]) | set(raws[1]) == set(ds.images) and raws[1][-1] == ds.images[0]
    assert len(raws[0]) == len(raws[1]) == 4


YAML = """
train_cfg: {by_epoch: True, max_epochs: 1, val_interval: 1}
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
"""


def test_runner_fits_and_validates_from_yaml(dgtd, tmp_path):
    write_folder(tmp_path / "data", "RGB", "depth", sizes=SIZES7[:4], jpeg=1)
    logs = []
    torch.manual_seed(0)
    r = dgtd.runner.Runner(dgtd.runner.load_config(YAML % {"root": str(tmp_path / "data")}), device="cuda", compute_dtype=torch.float32,
                           work_dir=str(tmp_path / "work"), log=logs.append, seed=3)
    seen, step = [], r.train_step
    r.train_step = lambda batch: (seen.append(batch), step(batch))[1]
    losses = r.fit()
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert sum(isinstance(m, str) and " val " in m and "MAE" in m for m in logs) == 1
    assert torch.is_tensor(seen[0]["input"]) and seen[0]["input"].shape == (2, 3, S, S)      # stacked by DeviceLoader, not a list from batches(...)
    assert r._device_loaders == {}                                # fit() closed the loaders (and their decode threads) it opened
    ds = r.build_dataset("train")                                 # the host path of the very first batch the runner trained on
    ds.set_epoch(0)
    sampler = dgtd.runner.DefaultSampler(4, shuffle=True, seed=3)
    first = list(sampler)[:2]
    assert seen[0]["raw"] == [ds.images[i] for i in first]
    for key in ("input", "label", "depth"):
        assert torch.equal(seen[0][key].cpu(), torch.stack([ds[i][key] for i in first])), key
    metrics = r.validate_config()
    assert set(metrics) == {"MAE"} and math.isfinite(metrics["MAE"]) and 0.0 <= metrics["MAE"] <= 1.0
    r.cfg["train_dataloader"]["dataset"]["image_size"] = 96      # a size the model was not built for: refused before the first step
    steps = len(seen)
    with pytest.raises(ValueError, match="img_size"):
        r.fit()
    assert len(seen) == steps and r._device_loaders == {}
