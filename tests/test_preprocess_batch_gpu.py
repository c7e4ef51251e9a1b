"""GPU: dgtd_preprocess_batch (csrc/preprocess_batch.hip) - a batch of planes of differing sizes in three launches - against the
single-image entry of the same file (torch.equal per plane: the job read from the device table and the job passed by value reach the
same device code) and, as the independent check, the numpy restatement of the transform chain, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import preprocess_cpu as pc

pytestmark = pytest.mark.gpu

MIXED = [(97, 131, 3), (20, 30, 1), (1, 7, 1), (50, 33, 3), (300, 400, 1)]       # (20,30) -> 64 is the up-scale
#         input[0]      label[0]     depth[0]    input[1]     label[1]            depth[1] is written by no job
SLOTS = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)]
FLIPS = [True, False, True, False, True]
GAP = 256
CANARY = 0xA5


@pytest.fixture(scope="module")
def dgtd():
    import dgtd as m
    m._lib.load()
    return m


def _planes(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]


class Call:
    """Buffers of one dgtd_preprocess_batch call; the workspace carries a canary gap between job 1's and job 2's regions and 256
    trailing canary bytes, the outputs start as NaN."""

    def __init__(self, dgtd, planes, slots, flips, S, B, dtype=torch.float32):
        L = dgtd._lib
        self.L, self.S, self.B, self.n = L, S, B, len(planes)
        shapes = [p.shape for p in planes]
        self.lay = lay = L.preprocess_batch_layout(shapes, S)
        for key in ("mid", "tab_h", "tab_v"):                     # open a gap in front of job 2
            lay[key] = [o + (GAP if j >= 2 else 0) for j, o in enumerate(lay[key])]
        self.gap_at = lay["mid"][2] - GAP if self.n > 2 else None
        self.ws_bytes = lay["workspace_bytes"] + (GAP if self.n > 2 else 0)
        self.table = (L.PreprocessJob * self.n)()
        L.fill_preprocess_jobs(self.table, shapes, lay, flips, [s[2] == 3 for s in shapes], [s for s, _ in slots], [b for _, b in slots])
        host = np.zeros(lay["planes_bytes"], np.uint8)
        for p, off in zip(planes, lay["src"]):
            host[off:off + p.size] = p.reshape(-1)
        self.planes = torch.from_numpy(host).cuda()
        self.ws = torch.full((self.ws_bytes + 256,), CANARY, dtype=torch.uint8, device="cuda")
        self.out = [torch.full((B, c, S, S), float("nan"), dtype=dtype, device="cuda") for c in (3, 1, 1)]
        self.mean, self.std = (ctypes.c_float * 3)(*pc.IMAGENET_MEAN), (ctypes.c_float * 3)(*pc.IMAGENET_STD)

    def run(self, njobs=None, planes_bytes=None, ws_bytes=None):
        """Returns (status, message); uploads the table as it stands."""
        L = self.L
        dev_table = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8).cuda()
        rc = L.load().dgtd_preprocess_batch(self.planes.data_ptr(), self.planes.numel() if planes_bytes is None else planes_bytes,
                                            dev_table.data_ptr(), ctypes.addressof(self.table), self.n if njobs is None else njobs,
                                            L.ptr(self.out[0]), L.ptr(self.out[1]), L.ptr(self.out[2]), self.B, self.S, self.mean, self.std,
                                            self.ws.data_ptr(), self.ws_bytes if ws_bytes is None else ws_bytes, L.dtype_code(self.out[0]),
                                            L.stream_ptr())
        torch.cuda.synchronize()
        return rc, L.load().dgtd_last_error().decode()

    def canaries_intact(self):
        tail = self.ws[self.ws_bytes:]
        ok = bool((tail == CANARY).all()) and tail.numel() == 256
        if self.gap_at is not None:
            ok = ok and bool((self.ws[self.gap_at:self.gap_at + GAP] == CANARY).all())
        return ok

    def untouched(self):
        return all(bool(torch.isnan(o).all()) for o in self.out)


@pytest.fixture(scope="module")
def mixed(dgtd):
    """The mixed batch run once in fp32; its planes, the call and the per-plane numpy reference are shared, none is modified."""
    planes = _planes(MIXED, 11)
    call = Call(dgtd, planes, SLOTS, FLIPS, 64, 2)
    rc, msg = call.run()
    assert rc == 0, msg
    ref = [pc.preprocess(p[:, :, 0] if p.shape[2] == 1 else p, 64, normalize=(p.shape[2] == 3), flip=f) for p, f in zip(planes, FLIPS)]
    return planes, call, ref


def test_mixed_sizes_equal_the_single_image_entry_and_the_restatement(dgtd, mixed):
    planes, call, ref = mixed
    assert call.L.load().dgtd_preprocess_batch_workspace(ctypes.addressof(call.table), call.n, 64) == call.lay["workspace_bytes"]
    for p, (sel, b), flip, want in zip(planes, SLOTS, FLIPS, ref):
        got = call.out[sel][b]
        one = dgtd.runner.device_preprocess(torch.from_numpy(p).cuda(), 64, normalize=(p.shape[2] == 3), flip=flip)
        assert got.dtype == torch.float32 and torch.equal(got, one), p.shape
        assert np.array_equal(got.cpu().numpy(), want), p.shape


def test_output_coverage_and_workspace_canaries(mixed):
    _, call, _ = mixed
    # The issue words this as "no NaN remains after the call".  Its own list of five planes fills five of the six slots of a batch
    # of two, so the check is made per slot and is stricter than the wording: every targeted slot is free of NaN, and the one slot
    # no job targets must still be all NaN (the kernels write nothing but what the jobs name).
    for sel, b in SLOTS:
        assert not torch.isnan(call.out[sel][b]).any()           # every element of a targeted slot is written
    assert torch.isnan(call.out[2][1]).all()                     # and nothing outside them: no job targets depth[1]
    assert call.canaries_intact()


def test_other_size_single_sample(dgtd):
    planes = _planes([(97, 131, 3), (97, 131, 1), (40, 60, 1)], 5)
    call = Call(dgtd, planes, [(0, 0), (1, 0), (2, 0)], [True] * 3, 48, 1)
    rc, msg = call.run()
    assert rc == 0, msg
    for p, (sel, _) in zip(planes, [(0, 0), (1, 0), (2, 0)]):
        one = dgtd.runner.device_preprocess(torch.from_numpy(p).cuda(), 48, normalize=(p.shape[2] == 3), flip=True)
        want = pc.preprocess(p[:, :, 0] if p.shape[2] == 1 else p, 48, normalize=(p.shape[2] == 3), flip=True)
        assert torch.equal(call.out[sel][0], one) and np.array_equal(call.out[sel][0].cpu().numpy(), want)
        assert not torch.isnan(call.out[sel]).any()
    assert call.canaries_intact()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_outputs_are_the_fp32_result_cast(dgtd, mixed, dtype):
    planes, call32, _ = mixed
    call = Call(dgtd, planes, SLOTS, FLIPS, 64, 2, dtype)
    rc, msg = call.run()
    assert rc == 0, msg
    for sel, b in SLOTS:
        assert call.out[sel].dtype == dtype and torch.equal(call.out[sel][b], call32.out[sel][b].to(dtype))
    assert torch.isnan(call.out[2][1]).all() and call.canaries_intact()


def test_refusals_return_the_error_and_launch_nothing(dgtd, mixed):
    planes = mixed[0]
    L = dgtd._lib

    def fresh():
        return Call(dgtd, planes, SLOTS, FLIPS, 64, 2)

    c = fresh()
    c.table[1].C = 2
    rc, msg = c.run()
    assert rc == 2 and "job 1" in msg and "C=2" in msg and c.untouched() and c.canaries_intact()
    for field in ("src_off", "mid_off", "tab_h_off", "tab_v_off"):
        c = fresh()
        setattr(c.table[3], field, getattr(c.table[3], field) + 8)
        rc, msg = c.run()
        assert rc == 2 and "job 3" in msg and "aligned" in msg and c.untouched(), field
    c = fresh()
    rc, msg = c.run(planes_bytes=c.lay["src"][4] + 300 * 400 - 1)          # the last plane ends one byte past the size passed in
    assert rc == 2 and "job 4" in msg and "outside" in msg and c.untouched()
    c = fresh()
    c.table[0].src_off = 1 << 40
    rc, msg = c.run()
    assert rc == 2 and "job 0" in msg and "outside" in msg and c.untouched()
    c = fresh()
    rc, msg = c.run(ws_bytes=c.lay["tab_v"][4] + 16)                       # the last table does not fit
    assert rc == 2 and "job 4" in msg and "workspace" in msg and c.untouched() and c.canaries_intact()
    c = fresh()
    c.table[0].H = c.table[0].W = 2 ** 31 - 1                              # H*W*C would wrap int64: the sides are bounded first
    rc, msg = c.run()
    assert rc == 2 and "job 0" in msg and "bad sizes" in msg and c.untouched()
    c = fresh()
    c.table[2].batch = 2
    rc, msg = c.run()
    assert rc == 2 and "batch index" in msg and c.untouched()
    c = fresh()
    assert L.PREPROCESS_BATCH_MAX_JOBS == 65535
    rc, msg = c.run(njobs=L.PREPROCESS_BATCH_MAX_JOBS + 1)                 # refused before the table is read
    assert rc == 2 and "65535" in msg and c.untouched()
    with pytest.raises(L.DgtdError, match="65535"):
        L.call("dgtd_preprocess_batch", c.planes.data_ptr(), c.planes.numel(), c.planes.data_ptr(), ctypes.addressof(c.table), 0, None, None, None,
               2, 64, c.mean, c.std, c.ws.data_ptr(), c.ws_bytes, 0, L.stream_ptr())
