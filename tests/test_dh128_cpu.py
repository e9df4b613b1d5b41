"""Head dim 128, host side (no GPU): EngineConfig and the flat parameter layout for the two scale-ups of BASELINE configs[4]
(hidden 1024 / 8 heads, hidden 512 / 4 heads) and the fixture's hidden 256 / 2 heads, the head-dim check of EngineConfig.from_model_config,
the default config unchanged, and the reference fixture's shape (tests/golden/dh128_*, scripts/make_dh128_goldens.py)."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import load_json, load_npz
from helpers import build_model, model_config
from multi_modal_foundation_model_amd.engine import HEAD_DIMS, EngineConfig, ParamLayout

MODS = [("ap", 12), ("behavior", 2)]
# EngineConfig.from_model_config(model_config(), [("ap", 668), ("behavior", 2)]) before head dim 128 existed, field for field
PARENT_DEFAULT = {'hidden': 256, 'heads': 8, 'inter': 512, 'n_enc': 5, 'n_dec': 5, 'max_F': 100, 'mult': 2, 'n_modality': 2, 'embed_scale': 1.0,
                  'embed_dropout': 0.2, 'dropout': 0.4, 'sep_mask': False, 'causal_mask': False, 'mods': [('ap', 668), ('behavior', 2)],
                  'loss_kind': {'ap': 0, 'behavior': 1}, 'loss_param': {}, 'loss_flags': {}, 'norm': 'layernorm', 'act': (0, 1.0),
                  'enc_attn_bias': True, 'enc_mlp_bias': True, 'dec_attn_bias': True, 'dec_mlp_bias': True}


@pytest.mark.parametrize("H,heads,inter", [(1024, 8, 2048), (512, 4, 1024), (256, 2, 512)])
def test_engine_config_and_layout_at_head_dim_128(H, heads, inter):
    """The config builds, and the ParamLayout key set equals the model's state-dict keys (one layer a side keeps the model small)."""
    mc = model_config(H=H, heads=heads, inter=inter, n_enc=1, n_dec=1, max_F=8)
    cfg = EngineConfig.from_model_config(mc, MODS)
    assert (cfg.hidden, cfg.heads, cfg.inter) == (H, heads, inter) and cfg.hidden // cfg.heads == 128
    model = build_model(mc, 12, 2, seed=0)
    layout = ParamLayout(cfg)
    named = dict(model.named_parameters())
    assert set(layout.entries) == set(named)
    assert set(layout.entries) <= set(model.state_dict())
    for name, p in named.items():
        assert layout.entries[name][1] == tuple(p.shape), name


@pytest.mark.parametrize("H,heads,what", [(256, 3, "not a multiple"), (96, 2, "head dim 48")])
def test_head_dims_outside_the_built_set_raise_when_the_config_is_read(H, heads, what):
    with pytest.raises(ValueError, match=what) as e:
        EngineConfig.from_model_config(model_config(H=H, heads=heads, inter=2 * H, n_enc=1, n_dec=1), MODS)
    assert "(8, 16, 32, 64, 128)" in str(e.value), "the message names the accepted head dims"
    assert HEAD_DIMS == (8, 16, 32, 64, 128)


def test_every_built_head_dim_is_accepted():
    for dh in HEAD_DIMS:
        assert EngineConfig.from_model_config(model_config(H=2 * dh, heads=2, inter=4 * dh, n_enc=1, n_dec=1), MODS).heads == 2


def test_default_engine_config_is_the_parents():
    c = EngineConfig.from_model_config(model_config(), [("ap", 668), ("behavior", 2)])
    assert dataclasses.asdict(c) == PARENT_DEFAULT
    assert [f.name for f in dataclasses.fields(EngineConfig)] == list(PARENT_DEFAULT)


def test_fixtures_hold_the_issue_cases_and_stay_small():
    z, meta = load_npz("dh128_fwd_bwd.npz")
    assert (meta["H"], meta["heads"], meta["inter"], meta["n_enc"], meta["n_dec"], meta["T"], meta["B"], meta["n_ap"], meta["n_beh"]) == \
        (256, 2, 512, 1, 1, 20, 3, 12, 2)
    assert meta["cases"] == {"dense": dict(causal=False, sep=False), "causal": dict(causal=True, sep=False),
                             "causal_sep": dict(causal=True, sep=True)}
    for case in meta["cases"]:
        assert all(f"{case}/grad/{k}" in z.files and f"{case}/grad_stat/{k}" in z.files for k in meta["params"])
        assert float(z[f"{case}/loss"]) > 0
    assert all(f"init/{k}" in z.files for k, _ in meta["state"])
    g = load_json("dh128_curve.json")
    assert len(g["loss"]) == len(g["objective"]) == 50 and g["H"] // g["heads"] == 128 and len(g["final_norm"]) == g["n_state_keys"]
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert all(os.path.getsize(os.path.join(gold, f)) < 2 ** 20 for f in ("dh128_fwd_bwd.npz", "dh128_curve.json"))


def test_mirror_state_dict_is_the_references_at_head_dim_128():
    """Keys, order, shapes and the initial values (stored elements bit for bit, fp64 sums) of the API mirror's state dict."""
    z, meta = load_npz("dh128_fwd_bwd.npz")
    mc = model_config(H=meta["H"], heads=meta["heads"], inter=meta["inter"], n_enc=meta["n_enc"], n_dec=meta["n_dec"], max_F=meta["max_F"],
                      dropout=0.0, emb_dropout=0.0)
    model = build_model(mc, meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == meta["state"]
    assert [k for k, _ in model.named_parameters()] == meta["params"]
    n = meta["sample"]
    for k, v in model.state_dict().items():
        f = v.numpy().reshape(-1)
        np.testing.assert_array_equal(f if f.size <= n else f[::f.size // n][:n], z[f"init/{k}"], err_msg=k)
        assert float(v.double().sum()) == pytest.approx(float(z[f"init_stat/{k}"][0]), rel=1e-9, abs=1e-9), k
