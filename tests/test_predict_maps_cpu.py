"""CPU: the float64 restatement behind the prediction-map tests (tests/_predict_ref.py) against torch, the packing helper, the job
struct, the ``val_cfg.save_maps`` parser and ``MapWriter``'s file handling (no device)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _predict_ref as R


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    return m


def test_restatement_equals_torch_interpolate_in_float64():
    worst = 0.0
    for S in (32, 64):
        plane = torch.from_numpy(R.logits(1, S, seed=S)[0]).double()
        for (H, W) in R.target_sizes(S):
            want = F.interpolate(plane[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0].numpy()
            got = R.resize(plane.numpy(), H, W, coords=np.float64)
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"restatement vs F.interpolate(float64): max |diff| {worst:.2e}")
    assert worst <= 1e-12


def test_fp32_taps_are_the_float64_taps_up_to_coordinate_rounding():
    """The two ``coords`` variants differ only by the fp32 rounding of src (three roundings at magnitude <= in): the maps differ by at
    most that times the largest neighbour difference, per axis."""
    for S in (32, 64):
        plane = R.logits(1, S, seed=S)[0]
        step = max(float(np.abs(np.diff(plane, axis=0)).max()), float(np.abs(np.diff(plane, axis=1)).max()))
        for (H, W) in R.target_sizes(S):
            d = np.abs(R.resize(plane, H, W, np.float32) - R.resize(plane, H, W, np.float64)).max()
            assert d <= 2 * (4 * R.U * S) * step, (S, H, W, d)


def test_identity_size_is_the_source():
    plane = R.logits(1, 32, seed=5)[0]
    for coords in (np.float32, np.float64):
        assert np.array_equal(R.resize(plane, 32, 32, coords), plane.astype(np.float64))


def test_quantisation_rule_is_save_image():
    v = torch.linspace(0.0, 1.0, 1 << 20, dtype=torch.float64)
    want = v.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(R.quantise(255.0 * v.numpy()), want)
    assert R.quantise(np.array([np.nan, -3.0, 300.0, 254.5, 254.49])).tolist() == [0, 0, 255, 255, 254]


def test_accepts_is_exact_outside_the_tie_band():
    v = np.array([10.2, 10.4999, 10.5001, 10.5, np.nan, 0.0, 255.0])
    assert R.accepts(np.array([10, 10, 11, 11, 0, 0, 255]), v, 1e-3).all()
    assert R.accepts(np.array([10, 11, 10, 10, 0, 0, 255]), v, 1e-3).tolist() == [True, True, True, True, True, True, True]
    assert R.accepts(np.array([11, 9, 12, 9, 1, 1, 254]), v, 1e-3).tolist() == [False] * 7
    assert R.eps_plain(16.0) < 1e-3 and R.eps_minmax(16.0, 0.5) < 5e-3


def test_tie_share_of_the_test_inputs_is_small():
    worst = 0.0
    for S in (32, 64):
        plane = R.logits(1, S, seed=S)[0]
        for (H, W) in R.target_sizes(S):
            if H * W >= 100:
                worst = max(worst, R.tie_share(R.levels(plane, H, W)[0], 1e-3))
    print(f"worst tie share at eps = 1e-3: {worst:.4f}")
    assert worst <= 0.05


def test_layout_is_aligned_tight_and_in_order(dgtd):
    L = dgtd._lib
    sizes = [(1, 1), (1, 7), (32, 32), (33, 47), (5, 67), (3, 1), (16, 16)]
    offsets, total = L.predict_maps_layout(sizes)
    end = 0
    for (h, w), off in zip(sizes, offsets):
        assert off % 16 == 0 and end <= off < end + 16           # aligned, behind the previous map, no more than the padding apart
        end = off + h * w
    assert total == end                                          # tight: nothing behind the last map
    assert L.predict_maps_layout([(4, 4)]) == ([0], 16)
    for bad in ([], [(0, 3)], [(3, (1 << 24) + 1)]):
        with pytest.raises(L.DgtdError):
            L.predict_maps_layout(bad)


def test_predict_job_is_32_bytes(dgtd):
    J = dgtd._lib.PredictJob
    assert ctypes.sizeof(J) == 32
    assert (J.out_off.offset, J.H.offset, J.W.offset, J.batch.offset, J.reserved.offset) == (0, 8, 12, 16, 20)


def test_save_maps_parser(dgtd):
    parse = dgtd.runner.predict.parse_save_maps
    assert parse(None) is None
    assert parse({"out_dir": "maps"}) == {"out_dir": "maps", "minmax": False}
    assert parse({"out_dir": "maps", "normalize": "minmax"}) == {"out_dir": "maps", "minmax": True}
    assert parse({"normalize": "none"}) == {"out_dir": None, "minmax": False}
    with pytest.raises(KeyError):
        parse({"out_dirs": "maps"})
    with pytest.raises(ValueError):
        parse({"out_dir": "maps", "normalize": "min-max"})
    with pytest.raises(TypeError):
        parse({"out_dir": 3})
    with pytest.raises(TypeError):
        parse("maps")


def test_runner_rejects_a_misspelt_save_maps_before_building_the_model(dgtd, monkeypatch):
    built = []
    monkeypatch.setattr(dgtd.runner.config, "build_model", lambda *a, **k: built.append(1))
    cfg = {"model": {"type": "cod"}, "val_cfg": {"save_maps": {"out_dir": "maps", "normalise": "minmax"}}}
    with pytest.raises(KeyError, match="normalise"):
        dgtd.runner.Runner(cfg, device="cpu")
    assert built == []


def test_map_writer_names_files_by_stem_and_replaces_atomically(dgtd, tmp_path):
    from PIL import Image
    L = dgtd._lib
    sizes = [(5, 7), (3, 1), (16, 16)]
    raws = ["/data/RGB/a_01.jpg", "b.png", "deep/dir/c.v2.png"]
    offsets, total = L.predict_maps_layout(sizes)
    rng = np.random.default_rng(0)
    packed = rng.integers(0, 256, total, dtype=np.uint8)
    out = tmp_path / "maps"
    (out).mkdir()
    (out / "b.png").write_bytes(b"stale")                         # an earlier file under the same name is replaced
    w = dgtd.runner.MapWriter(str(out), workers=2)
    w.put(w.stages[0], packed, [(dgtd.runner.predict.map_path(str(out), r), h, wd, off) for r, (h, wd), off in zip(raws, sizes, offsets)])
    paths = w.close()
    assert [os.path.basename(p) for p in paths] == ["a_01.png", "b.png", "c.v2.png"]
    assert sorted(os.listdir(out)) == ["a_01.png", "b.png", "c.v2.png"]          # no *.tmp left behind
    for p, (h, wd), off in zip(paths, sizes, offsets):
        with Image.open(p) as im:
            assert im.mode == "L" and im.size == (wd, h)
            assert np.array_equal(np.asarray(im), packed[off:off + h * wd].reshape(h, wd))


def test_map_writer_close_raises_the_first_encode_error_and_leaves_no_tmp(dgtd, tmp_path):
    w = dgtd.runner.MapWriter(str(tmp_path / "maps"), workers=1)
    packed = np.zeros(16, np.uint8)
    w.put(w.stages[0], packed, [(str(tmp_path / "maps" / "missing_dir" / "x.png"), 4, 4, 0), (str(tmp_path / "maps" / "ok.png"), 4, 4, 0)])
    with pytest.raises(OSError):
        w.close()
    assert os.listdir(tmp_path / "maps") == ["ok.png"]
