"""Input pipeline (twig/dataset/sod_train.py:31-54): the numpy restatement against vectors produced by real Pillow
and against the Pillow installed here (CPU), and the HIP kernels against the restatement, bit-exactly (GPU)."""
import os

import numpy as np
import pytest
import torch

from oracle import preprocess_cpu as pc
from oracle.make_golden import GOLDEN_DIR, PREPROCESS_CASES


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN_DIR, "preprocess.npz"))


@pytest.mark.parametrize("case", PREPROCESS_CASES, ids=[c[0] for c in PREPROCESS_CASES])
def test_oracle_resize_matches_pillow_vectors(G, case):
    name, h, w, c, s = case
    x = G[name + ".in"]
    xi = x[:, :, 0] if c == 1 else x
    assert np.array_equal(pc.resize_bilinear_u8(xi, s), G[name + ".resized"])
    assert np.array_equal(pc.resize_bilinear_u8(np.ascontiguousarray(xi[:, ::-1]), s), G[name + ".resized_flip"])


def test_oracle_matches_installed_pillow_and_totensor_normalize():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for (h, w, c, s) in [(61, 45, 3, 32), (40, 40, 1, 64), (128, 96, 3, 96)]:
        x = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        xi = x[:, :, 0] if c == 1 else x
        ref = np.asarray(Image.fromarray(xi).resize((s, s), Image.BILINEAR))
        assert np.array_equal(pc.resize_bilinear_u8(xi, s), ref)
        t = torch.from_numpy(ref if c == 3 else ref[:, :, None]).permute(2, 0, 1).float().div(255)       # ToTensor
        if c == 3:
            t = (t - torch.tensor(pc.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(pc.IMAGENET_STD).view(3, 1, 1)   # Normalize
        assert np.array_equal(pc.preprocess(xi, s, normalize=(c == 3)), t.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,c,s", [(97, 131, 3, 64), (20, 30, 3, 48), (50, 33, 1, 40), (90, 64, 3, 64), (480, 640, 3, 512), (300, 400, 1, 384)])
@pytest.mark.parametrize("flip", [False, True])
def test_hip_pipeline_bit_exact(h, w, c, s, flip):
    import dgtd
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    xi = x[:, :, 0] if c == 1 else x
    want = pc.preprocess(xi, s, normalize=(c == 3), flip=flip)
    got = dgtd.runner.device_preprocess(torch.from_numpy(xi.copy()).cuda(), s, normalize=(c == 3), flip=flip)
    assert got.shape == (c, s, s) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)


# shapes at which the shared device bodies can still go wrong for a job passed by value
EDGE_SHAPES = [(1, 1, 3, 4),        # one-pixel plane
               (1, 7, 1, 64),       # one row, up-scale
               (33, 2, 3, 16),      # two columns, down-scale in H only
               (3, 200, 1, 16),     # 12.5x down-scale, ksize = 27
               (10, 10, 1, 300),    # 2S = 600 table threads: three blocks of the coefficient kernel, the axis boundary inside one
               (5, 7, 2, 6), (9, 4, 4, 8),   # the channel counts only the single entry accepts
               (64, 64, 3, 64)]     # identity resize, with Normalize


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,c,s", EDGE_SHAPES)
@pytest.mark.parametrize("flip", [False, True])
def test_hip_single_entry_edge_shapes_bit_exact(h, w, c, s, flip):
    import dgtd
    x = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, c), dtype=np.uint8)
    xi = x[:, :, 0] if c == 1 else x
    want = pc.preprocess(xi, s, normalize=(c == 3), flip=flip)
    got = dgtd.runner.device_preprocess(torch.from_numpy(xi.copy()).cuda(), s, normalize=(c == 3), flip=flip)
    assert got.shape == (c, s, s) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.gpu
def test_hip_four_channel_normalize_through_the_c_entry():
    import ctypes
    import dgtd
    L = dgtd._lib
    h, w, c, s = 9, 4, 4, 8
    x = np.random.default_rng(94).integers(0, 256, (h, w, c), dtype=np.uint8)
    mean, std = np.array([0.485, 0.456, 0.406, 0.25], np.float32), np.array([0.229, 0.224, 0.225, 0.5], np.float32)
    want = (pc.preprocess(x, s, normalize=False) - mean[:, None, None]) / std[:, None, None]
    assert want.dtype == np.float32
    img = torch.from_numpy(x).cuda()
    out = torch.full((c, s, s), float("nan"), device="cuda")
    ws = torch.empty(L.load().dgtd_preprocess_workspace(h, w, c, s), dtype=torch.uint8, device="cuda")
    L.call("dgtd_preprocess", L.ptr(img), L.ptr(out), (ctypes.c_float * 4)(*mean), (ctypes.c_float * 4)(*std), L.ptr(ws), h, w, c, s, 0,
           L.dtype_code(out), L.stream_ptr())
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,c,s", [(97, 131, 3, 64), (20, 30, 1, 48)])
def test_hip_single_entry_stays_inside_its_workspace(h, w, c, s):
    import ctypes
    import dgtd
    L = dgtd._lib
    x = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, c), dtype=np.uint8)
    want = pc.preprocess(x[:, :, 0] if c == 1 else x, s, normalize=(c == 3))
    nbytes = L.load().dgtd_preprocess_workspace(h, w, c, s)
    assert nbytes > 0
    img = torch.from_numpy(x).cuda()
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((c, s, s), float("nan"), device="cuda")
    mean = (ctypes.c_float * 3)(*pc.IMAGENET_MEAN) if c == 3 else None
    std = (ctypes.c_float * 3)(*pc.IMAGENET_STD) if c == 3 else None
    L.call("dgtd_preprocess", L.ptr(img), L.ptr(out), mean, std, L.ptr(ws), h, w, c, s, 0, L.dtype_code(out), L.stream_ptr())
    tail = ws[nbytes:]
    assert tail.numel() == 256 and bool((tail == 0xA5).all())
    assert not torch.isnan(out).any()
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.gpu
def test_device_sample_shares_the_flip():
    import dgtd
    rng = np.random.default_rng(3)
    rgb, gt, dep = (rng.integers(0, 256, sh, dtype=np.uint8) for sh in ((70, 90, 3), (70, 90), (70, 90)))
    out = dgtd.runner.device_sample(torch.from_numpy(rgb).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(dep).cuda(), 64, flip=True,
                                    out_dtype=torch.bfloat16)
    assert out["input"].shape == (3, 64, 64) and out["label"].shape == (1, 64, 64) and out["depth"].dtype == torch.bfloat16
    want = torch.from_numpy(pc.preprocess(gt, 64, normalize=False, flip=True)).bfloat16()
    assert torch.equal(out["label"].cpu(), want)
