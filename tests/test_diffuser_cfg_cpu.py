"""CPU: the yardstick and the plumbing of the configurable texture diffuser.  The oracle with its constants patched is what the GPU
tests of the ``diffuser`` option compare against, so it is pinned to the reference's own MessagePassing here; the YAML ``model:``
block must carry the option to the model class unchanged."""
import pytest
import torch

from oracle import cod_cpu, ref_loader


@pytest.mark.parametrize("grid,m", [(12, 1), (12, 9), (12, -1), (20, 3), (7, 2)])
def test_patched_oracle_equals_reference_message_passing(monkeypatch, grid, m):
    """The reference's MessagePassing(24, 64, k=7, max_step=m) on a grid x grid state is bit-identical to the oracle's with
    DIFFUSE_STEPS patched (max_step < 0 means max(h, w) = grid steps, cod.py:1203).  k stays 7: the reference pins padding=3 (cod.py:1204)."""
    if not ref_loader.reference_available():
        pytest.skip("reference tree not present")
    ref = ref_loader.load_reference_cod()
    monkeypatch.setattr(cod_cpu, "DIFFUSE_STEPS", grid if m < 0 else m)
    torch.manual_seed(grid * 100 + m)
    theirs = ref.MessagePassing(24, 64, k=7, max_step=m)
    ours = cod_cpu.MessagePassing(24, 64)
    ours.load_state_dict(theirs.state_dict())
    x = torch.randn(2, 24, grid, grid)
    w = torch.rand(2, 24 * 49, grid, grid)
    with torch.no_grad():
        assert torch.equal(theirs(x, w), ours(x, w))


YAML = """
model:
  type: {type}
  win_size: 8
  diffuser:
    grid: 22
    k: 5
    max_step: 6
"""


def test_yaml_model_block_carries_the_diffuser_option():
    import dgtd
    from dgtd.runner import config, registry
    seen = {}

    class Stub:
        def __init__(self, **kw):
            seen.update(kw)

    registry.register_model(Stub, name="diffuser_cfg_stub")
    try:
        cfg = config.load_config(YAML.format(type="diffuser_cfg_stub"))
        assert cfg["model"]["diffuser"] == {"grid": 22, "k": 5, "max_step": 6}
        model = config.build_model(cfg, compute_dtype=torch.float32)
    finally:
        config.MODEL_REGISTRY.pop("diffuser_cfg_stub", None)
        registry.REGISTRY.pop("diffuser_cfg_stub", None)
    assert isinstance(model, Stub)
    assert seen == {"win_size": 8, "diffuser": {"grid": 22, "k": 5, "max_step": 6}, "compute_dtype": torch.float32}
    assert dgtd.nn.modules.diffuser_kwargs(seen["diffuser"]) == {"grid": 22, "k": 5, "max_step": 6}
    assert dgtd.nn.modules.diffuser_kwargs({"latent_dim": 16}) == {"diffuser_latent": 16}
    assert dgtd.nn.modules.diffuser_kwargs(None) == {}


def test_unknown_diffuser_key_is_a_type_error():
    import dgtd
    from dgtd.runner import config
    with pytest.raises(TypeError, match="steps"):
        dgtd.nn.cod(img_size=64, diffuser={"grid": 9, "steps": 2})
    cfg = config.load_config("model:\n  type: cod\n  diffuser:\n    gird: 22\n")
    with pytest.raises(TypeError, match="gird"):
        config.build_model(cfg, compute_dtype=torch.float32)


def test_modules_size_their_parameters_from_the_option():
    """State-dict keys never change; three tensors change shape.  The pure predicate and the step rule, no device needed."""
    import dgtd
    M, O = dgtd.nn.modules, dgtd.ops.diffuser
    assert M.ShapePropWeightRegressor(3, 24).reg.weight.shape == (24 * 49, 3, 1, 1)
    assert M.ShapePropWeightRegressor(3, 16, k=5).reg.weight.shape == (16 * 25, 3, 1, 1)
    mp = M.MessagePassing(16, img_size=64, k=5, max_step=-1)
    assert (mp.k, mp.size, mp.max_step) == (5, 25, -1) and mp.conv.weight.shape == (3, 16, 1, 1)
    x, w = torch.randn(1, 16, 6, 6), torch.rand(1, 16 * 25, 6, 6)
    assert mp(x, w).shape == (1, 3, 64, 64)
    assert O.uses_generic(12, 7, 4, 24) is False
    assert all(O.uses_generic(*c) for c in [(13, 7, 4, 24), (12, 9, 4, 24), (12, 7, 0, 24), (12, 7, 4, 28)])
    assert O.resolve_steps(-1, 22) == 22 and O.resolve_steps(0, 22) == 0 and O.resolve_steps(6, 22) == 6
