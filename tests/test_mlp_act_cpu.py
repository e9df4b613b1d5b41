"""transformer.act other than gelu on the host side (no GPU): every accepted ACT2FN name maps to its kernel kind and beta, other
names (and different encoder / decoder activations) raise, the module builds, its state dict matches the reference's
(tests/golden/mlp_act_fwd_bwd.npz, scripts/make_mlp_act_goldens.py) and the engine's flat layout matches its parameters."""
import hashlib

import pytest

from conftest import load_npz
from helpers import build_model, model_config, tiny_config
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K
from multi_modal_foundation_model_amd.engine import EngineConfig, ParamLayout

MODS = [("ap", 12), ("behavior", 2)]
WANT = {"gelu": (L.MLP_GELU, 1.0), "relu": (L.MLP_RELU, 1.0), "silu": (L.MLP_SIGMOID, 1.0), "swish": (L.MLP_SIGMOID, 1.0),
        "quick_gelu": (L.MLP_SIGMOID, 1.702), "gelu_new": (L.MLP_GELU_TANH, 1.0), "gelu_pytorch_tanh": (L.MLP_GELU_TANH, 1.0),
        "gelu_fast": (L.MLP_GELU_TANH, 1.0)}


@pytest.mark.parametrize("name", sorted(WANT))
def test_accepted_names_map_to_kind_and_beta(name):
    assert K.mlp_act(name) == WANT[name]
    assert EngineConfig.from_model_config(model_config(act=name), MODS).act == WANT[name]
    fwd, grad = K.GEMM_ACTS[WANT[name][0]]
    assert grad == fwd + (2 if fwd == L.ACT_GELU else 1)


def test_default_config_is_gelu():
    assert EngineConfig.from_model_config(model_config(), MODS).act == (L.MLP_GELU, 1.0)
    assert L.MLP_GELU == 0          # a zero-initialised mmfm_mlp_desc means GELU


@pytest.mark.parametrize("name", ["tanh", "gelu_10", "mish", "leaky_relu", "Relu"])
def test_unknown_names_raise_listing_the_accepted_ones(name):
    with pytest.raises(NotImplementedError) as e:
        EngineConfig.from_model_config(model_config(act=name), MODS)
    for ok in WANT:
        assert ok in str(e.value)
    with pytest.raises(NotImplementedError):
        build_model(tiny_config(act=name), 12, 2, seed=7)


def test_encoder_decoder_act_must_match():
    mc = model_config(act="relu")
    mc["decoder"]["transformer"]["act"] = "silu"
    with pytest.raises(NotImplementedError):
        EngineConfig.from_model_config(mc, MODS)


def test_embedder_act_other_than_softsign_still_raises():
    mc = model_config(act="silu")
    mc["encoder"]["embedder"]["act"] = "relu"
    with pytest.raises(NotImplementedError):
        EngineConfig.from_model_config(mc, MODS)


@pytest.mark.parametrize("name", sorted(WANT))
def test_mlp_module_constructs(name):
    from multi_modal.mm_utils import MLP
    m = MLP(32, 64, name, True, 0.0)
    assert (m.act_kind, m.act_beta) == WANT[name]
    assert [k for k, _ in m.named_parameters()] == ["up_proj.weight", "up_proj.bias", "down_proj.weight", "down_proj.bias"]


@pytest.mark.parametrize("act", ["relu", "silu", "quick_gelu", "gelu_new"])
def test_state_dict_matches_reference_fixture(act):
    """Keys, order, shapes and initial values (sha256 of the fp32 bytes) of the reference's state dict under the same seed."""
    _, meta = load_npz("mlp_act_fwd_bwd.npz")
    model = build_model(tiny_config(act=act), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    want = meta["init"][act]
    sd = model.state_dict()
    assert list(sd) == [e["key"] for e in want]
    for e in want:
        v = sd[e["key"]]
        assert list(v.shape) == e["shape"] and str(v.dtype) == e["dtype"], e["key"]
        assert hashlib.sha256(v.numpy().tobytes()).hexdigest()[:16] == e["sha256"], e["key"]
        assert float(v.double().sum()) == e["sum"], e["key"]
    assert [k for k, _ in model.named_parameters()] == meta["params"][act]


@pytest.mark.parametrize("act", ["relu", "silu", "gelu_new"])
def test_param_layout_matches_named_parameters(act):
    mc = tiny_config(act=act, n_enc=2, n_dec=2)
    model = build_model(mc, 12, 2, seed=7)
    layout = ParamLayout(EngineConfig.from_model_config(mc, MODS))
    named = dict(model.named_parameters())
    assert set(layout.entries) == set(named)
    for name, p in named.items():
        assert layout.entries[name][1] == tuple(p.shape), name
    gelu = ParamLayout(EngineConfig.from_model_config(tiny_config(n_enc=2, n_dec=2), MODS))
    assert layout.entries == gelu.entries and layout.segments == gelu.segments
