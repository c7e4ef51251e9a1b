"""No GPU: the switch of the own weight-gradient kernel and its three C entry points in the ctypes table."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _own_wgrad_in_fresh_interpreter(value):
    env = dict(os.environ)
    env.pop("DGTD_OWN_WGRAD", None)
    if value is not None:
        env["DGTD_OWN_WGRAD"] = value
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", "import dgtd; print(dgtd.ops._native.OWN_WGRAD)"], env=env, cwd=ROOT, capture_output=True,
                         text=True, check=True)
    return out.stdout.strip().splitlines()[-1]


def test_own_wgrad_is_off_unless_the_environment_turns_it_on():
    assert _own_wgrad_in_fresh_interpreter(None) == "False"
    assert _own_wgrad_in_fresh_interpreter("1") == "True"


def test_wgrad_entry_points_are_in_the_ctypes_table():
    import dgtd
    sig = dgtd._lib.SIGNATURES
    for name in ("dgtd_gemm_wgrad_supported", "dgtd_gemm_wgrad_workspace", "dgtd_gemm_wgrad_batched"):
        assert name in sig, name
    assert len(sig["dgtd_gemm_wgrad_batched"][1]) == 13
    assert len(sig["dgtd_gemm_wgrad_workspace"][1]) == 4


def test_token_chunks_respect_the_cap_and_the_gate():
    """host logic only (no launch): the workspace size encodes the chunk count S; a chunk is at most 4096 tokens, unsupported shapes
    get no workspace, and the gate refuses what the kernel cannot tile"""
    import dgtd
    L = dgtd._lib.load()
    BF16, F16, F32 = dgtd._lib.BF16, dgtd._lib.F16, dgtd._lib.F32
    for batch, M, N, K in [(1, 64, 64, 64), (1, 1024, 320, 128), (2, 8192, 128, 128), (27, 8192, 2048, 512), (3, 131072, 512, 128), (3, 2048, 4096, 1024)]:
        assert L.dgtd_gemm_wgrad_supported(M, N, K, BF16) == 1 and L.dgtd_gemm_wgrad_supported(M, N, K, F16) == 1
        ws = L.dgtd_gemm_wgrad_workspace(batch, M, N, K)
        assert ws > 0 and ws % (batch * N * K * 4) == 0
        S = ws // (batch * N * K * 4)
        assert 1 <= S <= M // 64 and S * 4096 >= M, (batch, M, N, K, S)
    assert L.dgtd_gemm_wgrad_workspace(1, 64, 64, 64) == 64 * 64 * 4                  # one k-step: one chunk
    assert L.dgtd_gemm_wgrad_workspace(2, 8192, 128, 128) >= 2 * 2 * 128 * 128 * 4    # the cap alone forces two chunks
    for M, N, K, dt in [(96, 64, 64, BF16), (64, 96, 64, BF16), (64, 64, 96, BF16), (0, 64, 64, BF16), (64, 64, 64, F32), (1 << 22, 1024, 64, BF16)]:
        assert L.dgtd_gemm_wgrad_supported(M, N, K, dt) == 0, (M, N, K, dt)
    assert L.dgtd_gemm_wgrad_workspace(1, 96, 64, 64) == 0
