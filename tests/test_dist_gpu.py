"""GPU, 2 processes sharing the one MI355X over gloo: exercises the CUDA side of GradReducer that the CPU test cannot —
post-accumulate hooks on the autograd thread, bucket gather, the side HIP stream with event fences, working-weight refresh —
and checks both ranks end up with identical, averaged gradients and identical weights after an optimizer step.
(RCCL itself needs one GPU per rank, which only the driver's multi-GPU node has.)"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
        import dgtd
        torch.cuda.set_device(0)
        dgtd.dist.init_process_group("gloo")
        torch.manual_seed(rank)                     # replicas start different; broadcast must fix that
        net = torch.nn.Sequential(dgtd.nn.Linear(64, 256), dgtd.nn.LayerNorm(256, eps=1e-6), torch.nn.GELU(),
                                  dgtd.nn.Linear(256, 64), dgtd.nn.LayerNorm(64, eps=1e-6), dgtd.nn.Linear(64, 1)).cuda()
        dgtd.dist.broadcast_parameters(net)
        red = dgtd.dist.GradReducer(net, bucket_bytes=32 << 10, exclude_prefixes=(), working_dtype=torch.bfloat16)
        assert len(red.buckets) >= 2 and red.comm_stream is not None
        opt = dgtd.runner.build_optimizer(net, lr=1e-2, custom_keys={})
        g = torch.Generator().manual_seed(7)
        x = torch.randn(2, 128, 64, generator=g)[rank].cuda()
        y = torch.randn(2, 128, 1, generator=g)[rank].cuda()
        for _ in range(3):
            red.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = net(x)
            ((out.float() - y) ** 2).mean().backward()
            red.finish()
            grads = [p.grad.detach().float().cpu().numpy().copy() for p in net.parameters()]
            opt.step()
            red.refresh_working()
        torch.cuda.synchronize()
        weights = [p.detach().float().cpu().numpy().copy() for p in net.parameters()]
        q.put((rank, grads, weights))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc(), None))
        raise


def test_reducer_streams_and_hooks_two_ranks_one_gpu():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, g, w = q.get(timeout=300)
        assert not isinstance(g, str), f"rank {r}: {g}"
        res[r] = (g, w)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b) and np.isfinite(a).all() and np.abs(a).sum() > 0   # same averaged gradient on both ranks
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, b)                                                      # replicas stay in lock-step


# ------------------------------------------------------------------------------------------------ the real model, two ranks
def _flat_grads(net):
    """All parameter gradients of ``net`` as ONE fp32 vector on the GPU, in named_parameters order, + [(name, numel)]."""
    items = [(n, p.grad) for n, p in net.named_parameters() if p.grad is not None]
    return torch.cat([g.detach().float().reshape(-1) for _, g in items]), [(n, g.numel()) for n, g in items]


def _fingerprint(flat):
    """Order-sensitive exact integer fingerprint of an fp32 vector (bit pattern, not value): equal on two ranks <=> same tensor, up to
    2^-64 collisions.  Also the count of non-finite elements."""
    bits = flat.contiguous().view(torch.int32).to(torch.int64)
    w = (torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 65521) + 1
    return [int(bits.sum().item()), int((bits * w).sum().item()), int((~torch.isfinite(flat)).sum().item())]


def _cod_worker(rank, world, port, q, tmpdir):
    """One rank of a 2-rank job on the shared GPU: the real dgtd.nn.cod at 64x64, bf16 working copies, reducer + FlatAdamW, run twice
    in the same process group (starting a fresh model each time):
      'eager' = hooks gather + all-reduce buckets during backward (overlap on the side stream);
      'split' = GraphedTrainStep, graph A | bucketed all-reduce | graph B (gloo cannot be captured).
    The ranks compare their gradients / weights with each other through exact fingerprints (all_gather_object); rank 0 leaves its
    gradient vector in ``tmpdir`` for the comparison with the single-process reference (458 MB per mode: a file, not a pickle)."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
        os.environ["DGTD_GEMM_TUNE"] = "0"     # the library GEMM plan = the heuristic's first answer in every process (see _reference_worker)
        import copy
        import time
        torch.set_num_threads(4)               # three processes build a 114 M-parameter model at once: 3 x 16 spinning OpenMP threads on
        t0, marks = time.perf_counter(), []    # 16 cores made that take 116 s instead of 8
        mark = lambda what: marks.append((what, round(time.perf_counter() - t0, 1)))
        import dgtd
        from oracle import filler
        mark("imports")
        torch.cuda.set_device(0)
        dgtd.dist.init_process_group("gloo")
        S, B = 64, 2
        x, d, l = (t.cuda() for t in filler.synthetic_batch(B, S, seed=100 + rank))     # every rank its own samples
        batch = {"raw": None, "input": x, "label": l, "depth": d}
        base = dgtd.nn.cod(drop_path_rate=0.0, compute_dtype=torch.bfloat16)
        filler.fill_module(base)                # values from the parent's shared file (oracle/filler.py), seconds instead of 20
        mark("model built + filled")
        out = {}
        for mode in ("eager", "split"):
            net = copy.deepcopy(base).cuda().train()
            dgtd.dist.broadcast_parameters(net)
            red = dgtd.dist.GradReducer(net, bucket_bytes=16 << 20, working_dtype=torch.bfloat16)
            assert red.world == 2 and red.comm16 and len(red.buckets) >= 4 and red.comm_stream is not None
            opt = dgtd.runner.FlatAdamW(red, lr=1e-4, graph_safe=True)
            mark(f"{mode}: replica + broadcast + reducer + optimizer")
            losses, grads, names = [], None, None
            if mode == "eager":
                for _ in range(2):
                    red.zero_grad()
                    loss = net(None, x, l, d, mode="loss")["loss"]
                    loss.backward()
                    red.finish()
                    if grads is None:
                        torch.cuda.synchronize()
                        grads, names = _flat_grads(net)
                    opt.step()
                    losses.append(loss.item())
            else:
                stepper = dgtd.runner.GraphedTrainStep(net, red, opt, warmup=1, comm="split")
                stepper.capture(batch)
                assert stepper.mode == "split" and stepper.graph_opt is not None
                for _ in range(2):
                    losses.append(stepper(batch).item())
                    if grads is None:
                        torch.cuda.synchronize()
                        grads, names = _flat_grads(net)
                stepper.release()
            torch.cuda.synchronize()
            mark(f"{mode}: steps")
            weights = torch.cat([p.detach().float().reshape(-1) for p in net.parameters()])
            mine = {"grads": _fingerprint(grads), "weights": _fingerprint(weights), "n_grads": len(names)}
            both = [None, None]
            torch.distributed.all_gather_object(both, mine)
            bn = net.hitnet.Translayer2_1.bn.running_mean.detach().cpu().numpy().copy()
            if rank == 0:
                np.save(os.path.join(tmpdir, f"grads_{mode}.npy"), grads.cpu().numpy())
            out[mode] = {"both": both, "losses": losses, "bn": bn, "names": names if rank == 0 else None}
            del net, red, opt, grads, weights
            torch.distributed.barrier()
            mark(f"{mode}: fingerprints + file")
        out["timing"] = marks
        q.put((rank, out, None))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc(), None))
        raise


def _reference_worker(q, tmpdir):
    """world 1, same weights, own process: the gradient of the MEAN of the two ranks' losses = the mean of the per-rank gradients, each
    rank's batch through its own forward (BatchNorm statistics are per rank in the reference: plain BatchNorm2d, cod.py:362).
    Own process + DGTD_GEMM_TUNE=0 like the ranks: the library GEMM plans are otherwise picked by TIMING candidates once per process,
    two processes can pick differently, and bf16 gradients computed through differently-rounded GEMMs differ by several percent
    (measured 4-6 % pooled) - the bf16 noise floor of this model, not a property of the reducer."""
    try:
        os.environ["DGTD_GEMM_TUNE"] = "0"
        import copy
        torch.set_num_threads(4)
        import dgtd
        from oracle import filler
        S, B = 64, 2
        base = dgtd.nn.cod(drop_path_rate=0.0, compute_dtype=torch.bfloat16)
        filler.fill_module(base)
        acc, names, losses = None, None, []
        for rank in range(2):
            net = copy.deepcopy(base).cuda().train()
            red = dgtd.dist.GradReducer(net, bucket_bytes=16 << 20, working_dtype=torch.bfloat16)
            x, d, l = (t.cuda() for t in filler.synthetic_batch(B, S, seed=100 + rank))
            red.zero_grad()
            loss = net(None, x, l, d, mode="loss")["loss"]
            loss.backward()
            red.finish()
            torch.cuda.synchronize()
            g, names = _flat_grads(net)
            acc = g / 2 if acc is None else acc + g / 2
            losses.append(loss.item())
            del net, red
        np.save(os.path.join(tmpdir, "grads_ref.npy"), acc.cpu().numpy())
        q.put(("ref", {"losses": losses, "names": names}, None))
    except Exception:
        import traceback
        q.put(("ref", "ERROR: " + traceback.format_exc(), None))
        raise


def test_real_model_two_ranks_one_gpu():
    """the product's own modules (16-bit working copies, O,H,W,I gradient views, deferred weight gradients flushed
    from inside the hooks, 16-bit all-reduce payload) under a 2-rank reducer: both ranks hold the same averaged gradient, it equals the
    single-process mean of the per-rank gradients within the bf16 budget, replicas stay in lock-step after AdamW, BN statistics stay
    per rank - once with hook-driven overlap ("eager"), once through the captured split step ("split"); one process group, one reference."""
    import shutil
    import tempfile
    import dgtd
    from oracle import filler
    filler.fill_module(dgtd.nn.cod(drop_path_rate=0.0, compute_dtype=torch.bfloat16))    # generate once here (the later model tests of
    filler.save_disk_cache()                                                             # this session reuse it), share it with the children
    world, port = 2, _free_port()
    tmpdir = tempfile.mkdtemp(prefix="dgtd_2rank_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_cod_worker, args=(r, world, port, q, tmpdir)) for r in range(world)]
        procs.append(ctx.Process(target=_reference_worker, args=(q, tmpdir)))
        for p in procs:
            p.start()
        res = {}
        for _ in range(world + 1):
            r, payload, _ = q.get(timeout=900)
            assert not isinstance(payload, str), f"rank {r}: {payload}"
            res[r] = payload
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
        print("rank 0 timeline (s):", res[0]["timing"])
        want = np.load(os.path.join(tmpdir, "grads_ref.npy"), mmap_mode="r")
        lref, names = res["ref"]["losses"], res["ref"]["names"]
        den = float(np.dot(want.astype(np.float64), want.astype(np.float64)))
        for mode in ("eager", "split"):
            r0, r1 = res[0][mode], res[1][mode]
            assert r0["names"] == names and len(names) > 800
            f0, f1 = r0["both"]
            assert f0 == r1["both"][0] and f1 == r1["both"][1]                   # both ranks saw the same pair of reports
            assert f0["grads"] == f1["grads"] and f0["grads"][2] == 0, (mode, f0, f1)      # the all-reduced gradient is the same (finite) tensor on both ranks
            assert f0["weights"] == f1["weights"] and f0["weights"][2] == 0, (mode, f0, f1)   # replicas in lock-step after two optimizer steps
            assert f0["n_grads"] == f1["n_grads"] == len(names)
            assert not np.array_equal(r0["bn"], r1["bn"])                        # BatchNorm statistics are per rank (no SyncBN in the reference)
            l0, l1 = r0["losses"], r1["losses"]
            assert abs(l0[0] - lref[0]) < 2e-2 * abs(lref[0]) and abs(l1[0] - lref[1]) < 2e-2 * abs(lref[1]), (mode, l0, l1, lref)
            # element-level agreement with the single-process mean gradient: the bf16 payload rounding
            got = np.load(os.path.join(tmpdir, f"grads_{mode}.npy"), mmap_mode="r")
            assert got.shape == want.shape
            e2 = (got.astype(np.float64) - want.astype(np.float64)) ** 2
            num = float(e2.sum())
            rel = (num / den) ** 0.5
            ends = np.cumsum([n for _, n in names])
            shares = np.add.reduceat(e2, np.concatenate(([0], ends[:-1]))) / max(num, 1e-300)
            top = [(names[k][0], round(float(shares[k]), 3)) for k in np.argsort(-shares)[:4]]
            print(f"[{mode}] 2-rank vs single-process mean gradient: pooled rel L2 {rel:.4f} (budget 0.005); largest shares of the error: {top}")
            assert rel < 0.005, (mode, rel, top)      # measured 0.002 - 0.003
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


def test_bench_control_flow_two_ranks_one_gpu(tmp_path):
    """`bench.py --gpus N` had never run with N > 1 - rank 0 alone entered the instrumented pass (eager steps
    with bucketed all-reduces) while the others went to the barrier.  Two gloo ranks on the one GPU run the whole script at a small
    size with --full: graph capture (split mode: gloo cannot be captured), timed steps, the instrumented pass on EVERY rank, one JSON
    line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DGTD_DIST_BACKEND="gloo", DGTD_GEMM_CANDIDATES="2", OMP_NUM_THREADS="4")    # two ranks on one box's cores
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--size", "64", "--batch", "2", "--full", "--profile-steps", "1"]
    p = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=1100)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["parallelism"] == "dp2" and out["config"]["global_batch"] == 4
    assert out["config"]["hip_graph"] and out["config"]["graph_mode"] == "split", out["config"]
    assert out["config"]["allreduce_payload"].startswith("16-bit")
    assert out["value"] > 0 and out["roofline"] is not None and out["entries"], out
    assert np.isfinite(out["config"]["final_loss"])
