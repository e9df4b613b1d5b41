"""transformer.attention_bias / transformer.mlp_bias = false, host side (no GPU): the flat parameter layout and the API mirror's
state dict against the reference's (tests/golden/linear_bias_fwd_bwd.npz, scripts/make_linear_bias_goldens.py), the default layout
unchanged, EngineConfig from a YAML-shaped config with mixed switches."""
import dataclasses

import numpy as np
import pytest
import torch

import plan_sig
from conftest import load_json, load_npz
from helpers import build_model, model_config, tiny_config
from multi_modal_foundation_model_amd.engine import EngineConfig, ParamLayout, _align

MODS = [("ap", 12), ("behavior", 2)]
CASES = ("FT", "TF", "FF", "FF_TT")
ATTN = ("query", "key", "value", "out_proj")
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("linear_bias_fwd_bwd.npz")
    return _Z


def case_config(meta, case, **kw):
    (ea, em), (da, dm) = meta["switches"][case]
    return tiny_config(attn_bias=(ea, da), mlp_bias=(em, dm), **kw)


def governed(name, cfg):
    """True where `name` is a bias the config switches off."""
    side = name.split(".")[0]
    if side not in ("encoder", "decoder") or not name.endswith(".bias"):
        return False
    ab, mb = (cfg.enc_attn_bias, cfg.enc_mlp_bias) if side == "encoder" else (cfg.dec_attn_bias, cfg.dec_mlp_bias)
    parts = name.split(".")
    if parts[2] in ("attn", "cross_attn") and parts[3] in ATTN:
        return not ab
    if parts[2] == "mlp":
        return not mb
    return False


def test_fixture_covers_the_issue_cases():
    z, meta = fixture()
    assert meta["switches"] == {"FT": [[False, True], [False, True]], "TF": [[True, False], [True, False]],
                                "FF": [[False, False], [False, False]], "FF_TT": [[False, False], [True, True]]}
    assert sorted(meta["cases"]) == sorted(f"{c}/{o}" for c in CASES for o in ("encoding", "decoding", "token_masking"))


@pytest.mark.parametrize("case", CASES)
def test_layout_and_state_dict_match_reference_fixture(case):
    """Keys, order and shapes of the mirror's state dict equal the reference's; the layout holds exactly the model's parameters; the
    initial values are the reference's bit for bit (nn.Linear(bias=False) draws no bias: the stream behind it shifts)."""
    z, meta = fixture()
    mc = case_config(meta, case)
    model = build_model(mc, meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["state"][case]
    assert [k for k, _ in model.named_parameters()] == meta["params"][case]
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), z[f"{case}/init/{k}"], err_msg=k)
    cfg = EngineConfig.from_model_config(mc, MODS)
    layout = ParamLayout(cfg)
    named = dict(model.named_parameters())
    assert set(layout.entries) == set(named)
    for name, p in named.items():
        assert layout.entries[name][1] == tuple(p.shape), name
    # what went away is exactly the governed biases (and the fused aliases over them); everything else keeps its bias
    full = ParamLayout(dataclasses.replace(cfg, enc_attn_bias=True, enc_mlp_bias=True, dec_attn_bias=True, dec_mlp_bias=True))
    assert set(full.entries) - set(layout.entries) == {n for n in full.entries if governed(n, cfg)}
    assert set(full.alias) - set(layout.alias) == {n for n in full.alias if governed(n.replace(".qkv.", ".query.").replace(".kv.", ".key."), cfg)}
    for keep in ("decoder_proj_context.bias", "encoder_norm.bias", "decoder.0.ln1.bias", "decoder_embeddings.ap.out.bias",
                 "encoder_embeddings.ap.embedder.token_embed.bias"):
        assert keep in layout.entries


@pytest.mark.parametrize("case", CASES)
def test_layout_is_dense(case):
    """No slot is left where a bias was: entries are disjoint, ascending, 8-aligned, and each gap is only the alignment padding
    (the buffer ends on a multiple of 64), so the buffer's size is the aligned sum of its entries."""
    _, meta = fixture()
    layout = ParamLayout(EngineConfig.from_model_config(case_config(meta, case, n_enc=2, n_dec=2), MODS))
    end = 0
    for name, (off, shape) in layout.entries.items():
        assert off == _align(end), name
        end = off + int(np.prod(shape))
    assert layout.n == _align(end, 64)
    assert layout.n == _align(sum(_align(int(np.prod(s))) for _, s in layout.entries.values()), 64)
    starts = [s for _, s, _ in layout.segments]
    assert starts == sorted(starts) and layout.segments[-1][2] <= layout.n
    for a, names in ((k, v) for k, v in layout.alias.items()):
        off, shape = names
        first = a.replace(".qkv.", ".query.").replace(".kv.", ".key.")
        assert layout.entries[first][0] == off


def test_all_switches_true_is_the_parent_layout():
    """A config that never mentions the new fields (their defaults) and one built from the YAML's `true` give one layout."""
    yaml_cfg = EngineConfig.from_model_config(tiny_config(n_enc=2, n_dec=2), MODS)
    assert (yaml_cfg.enc_attn_bias, yaml_cfg.enc_mlp_bias, yaml_cfg.dec_attn_bias, yaml_cfg.dec_mlp_bias) == (True,) * 4
    fields = {f.name: getattr(yaml_cfg, f.name) for f in dataclasses.fields(EngineConfig) if not f.name.endswith("_bias")}
    omitted = EngineConfig(**fields)
    a, b = ParamLayout(yaml_cfg), ParamLayout(omitted)
    assert a.entries == b.entries and a.alias == b.alias and a.segments == b.segments and a.n == b.n
    assert list(a.entries) == list(b.entries)
    # ... and it still is the layout of the 254-key default model: every linear has its bias
    lins = [n[:-len(".weight")] for n, (_, s) in a.entries.items() if n.endswith(".weight") and len(s) == 2 and "_embed" not in n and "mod_emb" not in n]
    assert lins and all(l + ".bias" in a.entries for l in lins)


def test_engine_config_from_mixed_yaml_needs_no_device():
    mc = model_config(attn_bias=(False, True), mlp_bias=(True, False))
    c = EngineConfig.from_model_config(mc, [("ap", 668), ("behavior", 2)])
    assert (c.enc_attn_bias, c.enc_mlp_bias, c.dec_attn_bias, c.dec_mlp_bias) == (False, True, True, False)
    lay = ParamLayout(c)
    assert "encoder.0.attn.query.bias" not in lay.entries and "encoder.0.attn.qkv.bias" not in lay.alias
    assert "encoder.0.mlp.up_proj.bias" in lay.entries and "decoder.0.mlp.down_proj.bias" not in lay.entries
    assert "decoder.0.cross_attn.kv.bias" in lay.alias and "decoder.0.attn.out_proj.bias" in lay.entries
    # the default YAML leaves both on
    d = EngineConfig.from_model_config(model_config(), [("ap", 668), ("behavior", 2)])
    assert (d.enc_attn_bias, d.enc_mlp_bias, d.dec_attn_bias, d.dec_mlp_bias) == (True,) * 4


def test_reference_state_dict_round_trips():
    """A reference state dict without the bias keys loads strictly; one WITH them is refused for a bias-free model."""
    z, meta = fixture()
    model = build_model(case_config(meta, "FF"), meta["n_ap"], meta["n_beh"], seed=1)
    ref = {k: torch.from_numpy(z[f"FF/init/{k}"]) for k, _ in meta["state"]["FF"]}
    model.load_state_dict(ref, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k
    full = build_model(tiny_config(), meta["n_ap"], meta["n_beh"], seed=1)
    with pytest.raises(RuntimeError):
        model.load_state_dict(full.state_dict(), strict=True)


@pytest.mark.parametrize("case", CASES)
def test_ddp_buckets_cover_every_parameter(case):
    """The DDP wrapper reduces contiguous segment ranges of the flat gradient buffer: with biases gone the ranges still tile the
    buffer, in backward order, and every entry lies in exactly one bucket."""
    from multi_modal_foundation_model_amd.ddp import GradBuckets
    _, meta = fixture()
    cfg = EngineConfig.from_model_config(case_config(meta, case, n_enc=2, n_dec=2), MODS)
    layout = ParamLayout(cfg)
    b = GradBuckets(layout, cfg, bucket_bytes=16 << 10).buckets
    assert len(b) >= 3 and b[-1][1] == 0
    for (_, lo, hi), (_, lo2, hi2) in zip(b, b[1:]):
        assert hi2 == lo
    for name, (off, shape) in layout.entries.items():
        assert sum(lo <= off and off + int(np.prod(shape)) <= hi for _, lo, hi in b) == 1, name


@pytest.mark.parametrize("pin", list(plan_sig.LAYOUTS))
def test_param_layout_is_the_recorded_one(pin):
    """entries (names, order, offsets, shapes), aliases, segments and n of the YAML model's flat buffer - default, ScaleNorm, bias-free
    per side - are what tests/golden/param_layout.json recorded (scripts/make_plan_goldens.py --layout) before ParamLayout was
    rewritten over engine.block_linears."""
    assert plan_sig.layout_record(plan_sig.LAYOUTS[pin]) == load_json("param_layout.json")[pin]
