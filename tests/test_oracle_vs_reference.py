"""CPU: the oracle restatement against the reference's own outputs, stored by oracle/make_golden.py (tests/golden/ref32.npz: the
reference model at 32x32; tests/golden/msda.npz: the reference's ms_deform_attn_core_pytorch).  Self-contained: the vectors were
generated once from the reference, which the tests never read."""
import os

import numpy as np
import torch

from oracle import cod_cpu, filler
from oracle.make_golden import GOLDEN_DIR, grad_projection, grad_samples

# same-machine runs are bit-exact; a different host CPU may pick other oneDNN kernels (as tests/test_oracle_golden.py)
RTOL, ATOL = 2e-5, 2e-5


def test_keys_forward_backward_bit_exact():
    S = 32
    g = np.load(os.path.join(GOLDEN_DIR, "ref32.npz"))
    mine = cod_cpu.cod(S).train()
    sm = mine.state_dict()
    assert list(sm.keys()) == g["keys"].tolist() or set(sm) == set(g["keys"].tolist())
    shapes = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert all("x".join(map(str, v.shape)) == shapes[k] for k, v in sm.items())
    filler.fill_module(mine)
    x, d, l = filler.synthetic_batch(2, S)
    lb = mine(None, x, l, list(d), mode="loss")["loss"]
    assert abs(float(g["train.loss"]) - lb.item()) < 1e-5
    lb.backward()
    gm = dict(mine.named_parameters())
    assert sorted(gm) == sorted(g["train.grad_names"].tolist())
    for k, norm, samp, proj in zip(g["train.grad_names"].tolist(), g["train.grad_norms"], g["train.grad_samples"], g["train.grad_proj"]):
        q = gm[k].grad
        assert (norm < 0) == (q is None), k
        if q is None:
            continue
        np.testing.assert_allclose(q.double().norm().item(), norm, rtol=2e-4, atol=1e-7, err_msg=k)
        # a transposed / permuted / sign-flipped gradient keeps its norm but not its samples or its +-1 projection
        np.testing.assert_allclose(grad_samples(q), samp, rtol=1e-2, atol=1e-2 * norm / max(q.numel(), 1) ** 0.5, err_msg=k)
        assert abs(grad_projection(q) - proj) <= 1e-2 * norm + 1e-7, k
    mine.eval()
    with torch.no_grad():
        x_hp, P1, P2 = mine.hitnet(x, d)
    np.testing.assert_allclose(x_hp.numpy(), g["eval.x_hp"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(torch.stack(P1).numpy(), g["eval.P1"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(P2.numpy(), g["eval.P2"], rtol=RTOL, atol=ATOL)


def test_msda_restatement_vs_live_reference_function():
    """oracle/ms_deform_attn_cpu.py against the outputs of the reference's ms_deform_attn_core_pytorch
    (twig/ops/functions/ms_deform_attn_func.py:49-71) stored in tests/golden/msda.npz, at the tolerance of the former live comparison."""
    from oracle import ms_deform_attn_cpu as mc
    G = np.load(os.path.join(GOLDEN_DIR, "msda.npz"))
    for name, (N, M, D, Lq, shapes, P) in mc.CASES.items():
        value, shp, loc, attn, _ = mc.case_inputs(name, N, M, D, Lq, shapes, P)
        np.testing.assert_allclose(mc.ms_deform_attn(value, shp, loc, attn).numpy(), G[f"{name}.out"], rtol=1e-11, atol=1e-15, err_msg=name)
