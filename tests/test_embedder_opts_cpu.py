"""embedder.act / pos / bias, host side (no GPU): the activation names and their mmfm_gemm code pairs, EngineConfig's per-side values and
what stays an error without `embedder_opts=True`, the API mirror's state dict against the reference's
(tests/golden/embedder_opts_fwd_bwd.npz, scripts/make_embedder_goldens.py), the flat parameter layout, and the default model's layout
and descriptors, which must be what they were."""
import dataclasses

import numpy as np
import pytest

import plan_sig as S
from conftest import load_json
from embedder_opts import CASES, OBJECTIVES, case_config, fixture
from helpers import build_model, model_config, tiny_config
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K
from multi_modal_foundation_model_amd.engine import PER_SIDE_EMBED, EngineConfig, ParamLayout, Sides
from side_config import sides

MODS = [("ap", 12), ("behavior", 2)]
# name -> (forward code, gradient code) of include/mmfm.h
WANT = {"softsign": (2, 4), "identity": (12, 13), "linear": (12, 13), "relu": (14, 15), "gelu": (16, 17), "silu": (18, 19), "swish": (18, 19),
        "quick_gelu": (20, 21), "gelu_new": (22, 23), "gelu_pytorch_tanh": (22, 23), "gelu_fast": (22, 23), "tanh": (24, 25)}
# case -> (encoder, decoder) values of (embed_act, embed_pos, embed_bias, embed_scale)
DEF = ("softsign", True, True, 1.0)
SIDE_WANT = {"IDENTITY": ("identity", True, True, 1.0), "RELU": ("relu", True, True, 1.0), "GELU": ("gelu", True, True, 1.0),
             "SILU": ("silu", True, True, 1.0), "QUICK_GELU": ("quick_gelu", True, True, 1.0), "GELU_NEW": ("gelu_new", True, True, 1.0),
             "TANH": ("tanh", True, True, 1.0), "POS_OFF": ("softsign", False, True, 1.0), "BIAS_OFF": ("softsign", True, False, 1.0),
             "POS_BIAS_OFF": ("softsign", False, False, 1.0), "ASYM": (("tanh", False, False, 32 ** 0.5), DEF),
             "SCALE": ("silu", True, True, 0.7)}


def test_fixture_covers_the_issue_cases():
    z, meta = fixture()
    assert tuple(meta["switches"]) == CASES
    assert sorted(meta["cases"]) == sorted(f"{c}/{o}" for c in CASES for o in OBJECTIVES)
    assert (meta["B"], meta["T"], meta["n_ap"], meta["n_beh"], meta["H"], meta["model_seed"], meta["data_seed"]) == (2, 8, 12, 2, 32, 7, 3)
    for c in meta["full_grad_cases"]:
        assert sum(k.startswith(f"{c}/token_masking/grad/") for k in z.files) == len(meta["params"][c])
    assert set(load_json("embedder_opts_curve.json")) == {"ASYM", "GELU"}


def test_every_accepted_name_maps_to_its_code_pair():
    assert K.EMBED_ACTS == WANT
    for name, pair in WANT.items():
        assert K.embed_act(name) == pair
        if name != "softsign":
            assert pair[0] % 2 == 0 and pair[1] == pair[0] + 1 and 12 <= pair[0] <= 24
    assert (L.ACT_EMB_IDENTITY, L.ACT_EMB_TANH_GRAD) == (12, 25)


def test_unknown_name_raises_listing_the_accepted_ones():
    with pytest.raises(NotImplementedError) as e:
        K.embed_act("mish")
    assert all(name in str(e.value) for name in WANT)
    with pytest.raises(NotImplementedError, match="gelu_pytorch_tanh"):
        EngineConfig.from_model_config(sides(enc_emb=dict(act="mish")), MODS, per_side=True, embedder_opts=True)
    with pytest.raises(NotImplementedError, match="quick_gelu"):
        build_model(sides(dec_emb=dict(act="leaky_relu"), H=32, heads=4, inter=64, n_enc=1, n_dec=1, max_F=8), 12, 2, seed=0)


@pytest.mark.parametrize("case", CASES)
def test_engine_config_holds_each_sides_values(case):
    cfg = EngineConfig.from_model_config(case_config(case), MODS, per_side=True, embedder_opts=True)
    want = SIDE_WANT[case]
    enc_w, dec_w = want if isinstance(want[0], tuple) else (want, want)
    for side, w in (("encoder", enc_w), ("decoder", dec_w)):
        sc = cfg.side(side)
        assert (sc.embed_act, sc.embed_pos, sc.embed_bias, sc.embed_scale) == w, side
    for k in PER_SIDE_EMBED:
        e, d = getattr(cfg.side("encoder"), k), getattr(cfg.side("decoder"), k)
        assert getattr(cfg, k) == (e if e == d else Sides(e, d)) and isinstance(getattr(cfg, k), Sides) == (e != d), k


@pytest.mark.parametrize("emb,match", [(dict(act="gelu"), "softsign"), (dict(pos=False), "embedder_opts"), (dict(bias=False), "embedder_opts")])
@pytest.mark.parametrize("side", ["enc_emb", "dec_emb"])
@pytest.mark.parametrize("per_side", [False, True])
def test_without_the_keyword_all_three_keys_raise(emb, match, side, per_side):
    mc = sides(**{side: emb})
    with pytest.raises(NotImplementedError, match=match):
        EngineConfig.from_model_config(mc, MODS, per_side=per_side)
    cfg = EngineConfig.from_model_config(mc, MODS, per_side=per_side, embedder_opts=True)
    sc = cfg.side("encoder" if side == "enc_emb" else "decoder")
    assert (sc.embed_act, sc.embed_pos, sc.embed_bias) == (emb.get("act", "softsign"), emb.get("pos", True), emb.get("bias", True))


def test_constructor_takes_one_value_or_sides():
    base = EngineConfig.from_model_config(tiny_config(), MODS, per_side=True, embedder_opts=True)
    assert base == EngineConfig.from_model_config(tiny_config(), MODS) and (base.embed_act, base.embed_pos, base.embed_bias) == DEF[:3]
    one = {f.name: getattr(base, f.name) for f in dataclasses.fields(EngineConfig)}
    a = EngineConfig(**one, embed_act="tanh", embed_pos=False, embed_bias=(True, True))
    b = EngineConfig(**one, embed_act=Sides("tanh", "tanh"), embed_pos=[False, False])
    assert a == b != base and a.side("decoder").embed_act == "tanh" and a.embed_bias is True
    c = EngineConfig(**one, embed_act=("tanh", "softsign"), embed_pos=Sides(False, True))
    assert c.embed_act == Sides("tanh", "softsign") and c != a
    assert (c.side("encoder").embed_pos, c.side("decoder").embed_pos, c.side("decoder").embed_act) == (False, True, "softsign")


@pytest.mark.parametrize("case", CASES)
def test_layout_and_state_dict_match_reference_fixture(case):
    """Keys, order and shapes of the mirror's state dict equal the reference's - no pos_embed key under pos: false, no token_embed.bias
    under bias: false; the initial values are the reference's bit for bit (the construction order is the RNG contract); the layout holds
    exactly the model's parameters at their shapes."""
    z, meta = fixture()
    mc = case_config(case)
    model = build_model(mc, meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["state"][case]
    assert [k for k, _ in model.named_parameters()] == meta["params"][case]
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), z["init/" + meta["init"][case][k]], err_msg=k)
    sw = meta["switches"][case]
    for side in ("encoder", "decoder"):
        emb = sw[side].get("embedder", {})
        for mod in ("ap", "behavior"):
            p = f"{side}_embeddings.{mod}.embedder."
            assert (p + "pos_embed.weight" in sd) == emb.get("pos", True) and (p + "token_embed.bias" in sd) == emb.get("bias", True)
    layout = ParamLayout(EngineConfig.from_model_config(mc, MODS, per_side=True, embedder_opts=True))
    named = dict(model.named_parameters())
    assert set(layout.entries) == set(named)
    for name, p in named.items():
        assert layout.entries[name][1] == tuple(p.shape), name
    offs = sorted((off, int(np.prod(shape))) for off, shape in layout.entries.values())
    assert all(a + n <= b for (a, n), (b, _) in zip(offs, offs[1:])) and offs[-1][0] + offs[-1][1] <= layout.n


def test_default_layout_and_descriptors_are_what_they_were():
    """The YAML model's layout read with embedder_opts=True is the pinned one (tests/golden/param_layout.json), and mmfm_gemm_desc has the
    fields it had: the new behaviour rides on act codes and NULL pointers."""
    want = load_json("param_layout.json")["default"]
    lay = ParamLayout(EngineConfig.from_model_config(model_config(), [("ap", 668), ("behavior", 2)], per_side=True, embedder_opts=True))
    got = dict(entries=[[k, off, list(shape)] for k, (off, shape) in lay.entries.items()],
               alias=[[k, off, list(shape)] for k, (off, shape) in lay.alias.items()], segments=[list(s) for s in lay.segments], n=lay.n)
    assert got == want == S.layout_record({})
    assert [n for n, _ in L.GemmDesc._fields_] == ["dtype", "c_f32", "A", "B", "C", "M", "N", "K", "lda", "ldb", "ldc", "a_kcontig", "b_kcontig",
                                                   "splits", "kchunk", "slab_stride", "bias", "pre_out", "act", "act_scale", "gradmul_pre", "drop",
                                                   "residual", "ldr", "colsum"]
    import ctypes
    assert ctypes.sizeof(L.GemmDesc) == 152
