"""use_scalenorm: true on the host side (no GPU): the engine accepts the switch, its flat parameter layout matches the module's
parameters (each ScaleNorm's 0-dim `.scale` included), and the module's state dict - keys, order, initial values - matches the
reference's (tests/golden/scalenorm_fwd_bwd.npz, scripts/make_scalenorm_goldens.py)."""
import hashlib
import math

import pytest
import torch

from conftest import load_npz
from helpers import build_model, model_config, tiny_config
from multi_modal_foundation_model_amd.engine import EngineConfig, ParamLayout

MODS = [("ap", 12), ("behavior", 2)]


def test_engine_config_accepts_use_scalenorm():
    cfg = EngineConfig.from_model_config(model_config(scalenorm=True), MODS)
    assert cfg.norm == "scalenorm"
    assert EngineConfig.from_model_config(model_config(), MODS).norm == "layernorm"
    mc = model_config(scalenorm=True)
    mc["decoder"]["transformer"]["use_scalenorm"] = False
    with pytest.raises(NotImplementedError):
        EngineConfig.from_model_config(mc, MODS)


@pytest.mark.parametrize("kw", [dict(), dict(n_enc=2, n_dec=3)])
def test_param_layout_matches_named_parameters(kw):
    mc = tiny_config(scalenorm=True, **kw)
    model = build_model(mc, 12, 2, seed=7)
    layout = ParamLayout(EngineConfig.from_model_config(mc, MODS))
    named = dict(model.named_parameters())
    assert set(layout.entries) == set(named)
    for name, p in named.items():
        off, shape = layout.entries[name]
        assert shape == tuple(p.shape), name
        if name.endswith(".scale"):
            assert shape == () and off % 8 == 0, name
    scales = [n for n in named if n.endswith(".scale")]
    assert len(scales) == 2 * mc.encoder.transformer.n_layers + 4 * mc.decoder.transformer.n_layers
    assert "encoder_norm.weight" in layout.entries and "decoder_norm.bias" in layout.entries       # stay LayerNorm (mm.py:72,77)
    # every parameter inside one DDP segment, and each `.scale` in the slot (order) the LayerNorm layout gives that norm's weight
    for name, (off, shape) in layout.entries.items():
        n = int(math.prod(shape))
        assert any(s <= off and off + n <= e for _, s, e in layout.segments), name
    ln_layout = ParamLayout(EngineConfig.from_model_config(tiny_config(**kw), MODS))
    assert [s[0] for s in ln_layout.segments] == [s[0] for s in layout.segments]
    want = []
    for k in sorted(ln_layout.entries, key=lambda k: ln_layout.entries[k][0]):
        base, leaf = k.rsplit(".", 1)
        if base.rsplit(".", 1)[-1] in ("ln1", "ln2", "query_norm", "context_norm"):
            if leaf == "weight":
                want.append(base + ".scale")
        else:
            want.append(k)
    assert sorted(layout.entries, key=lambda k: layout.entries[k][0]) == want


@pytest.mark.parametrize("variant", ["base", "pad", "sep", "deep"])
def test_state_dict_matches_reference_fixture(variant):
    """Keys, order, shapes and initial values (sha256 of the fp32 bytes) of the reference's state dict under the same seed."""
    _, meta = load_npz("scalenorm_fwd_bwd.npz")
    model = build_model(tiny_config(scalenorm=True, **meta["variants"][variant]), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    want = meta["init"][variant]
    sd = model.state_dict()
    assert list(sd) == [e["key"] for e in want]
    for e in want:
        v = sd[e["key"]]
        assert list(v.shape) == e["shape"] and str(v.dtype) == e["dtype"], e["key"]
        assert hashlib.sha256(v.numpy().tobytes()).hexdigest()[:16] == e["sha256"], e["key"]
        assert float(v.double().sum()) == e["sum"], e["key"]
        if e["key"].endswith(".scale"):
            assert v.shape == () and v.dtype == torch.float32 and float(v) == pytest.approx(meta["H"] ** 0.5)
    assert sum(e["key"].endswith(".scale") for e in want) == (12 if variant == "deep" else 6)
