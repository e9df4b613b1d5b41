"""embedder.act / pos / bias on the MI355X, whole models: the fp32 engine against the reference's own forward / backward and 50-step curves
(tests/golden/embedder_opts_*, scripts/make_embedder_goldens.py); the bf16 engine against an fp64 restatement (the tokeniser written here,
the rest oracle/mm_oracle.py) at the tiny size and at the default widths; one dropout-on step without position tables against the same
restatement fed the step's own masks; checkpoint resume and hipGraph replay of a non-default embedder model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_json
from embedder_opts import CASES, OBJECTIVES, case_config, fixture
from helpers import build_model
from model_checks import (bf16_stats, check_fixture_case, engine_step_and_oracle, graph_replay_matches_eager, resume_roundtrip,
                          run_curve)
from oracle import mm_oracle as O
from side_config import sides

pytestmark = pytest.mark.gpu
K_TANH = (2.0 / np.pi) ** 0.5


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """Loss, counts (exact), predictions, every gradient norm and (the full-gradient cases / token_masking) every gradient tensor; the
    quantities and tolerances of test_side_config_model_gpu.py::test_tiny_forward_backward_vs_reference_fixture."""
    z, meta = fixture()
    check_fixture_case(build_model(case_config(case), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"]), z, meta, case, objective)


@pytest.mark.parametrize("case", ["ASYM", "GELU"])
def test_loss_curve_tiny_50_steps_vs_reference_fixture(case):
    g = load_json("embedder_opts_curve.json")[case]
    model = build_model(case_config(case), g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    assert len(model.state_dict()) == g["n_state_keys"]
    losses = run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- the fp64 restatement
def act_ref(name, u):
    if name == "softsign":
        return u / (1 + u.abs())
    if name in ("identity", "linear"):
        return u
    if name == "relu":
        return torch.relu(u)
    if name == "gelu":
        return F.gelu(u)
    if name in ("silu", "swish", "quick_gelu"):
        return u * torch.sigmoid((1.702 if name == "quick_gelu" else 1.0) * u)
    if name in ("gelu_new", "gelu_pytorch_tanh", "gelu_fast"):
        return 0.5 * u * (1 + torch.tanh(K_TANH * (u + 0.044715 * u ** 3)))
    assert name == "tanh", name
    return torch.tanh(u)


def embed_ref(mc):
    """The tokeniser of the reference (encoder_embeddings.py:44-61 and its decoder twin) restated for a model config `mc`, with the
    signature of oracle.mm_oracle.embed: the side's act, scale, pos and bias come from its own `embedder` section."""
    def embed(sd, p, inputs, ts, mod_idx, cfg, training, gen=None, dropout_fn=None, site_key=None):
        e = mc[p.split("_", 1)[0]]["embedder"]
        scale = cfg.hidden ** 0.5 if e["scale"] is None else e["scale"]
        x = F.linear(inputs, sd[p + ".token_embed.weight"], sd[p + ".token_embed.bias"] if e["bias"] else None)
        x = F.linear(act_ref(e["act"], x) * scale, sd[p + ".projection.weight"], sd[p + ".projection.bias"])
        B, T, _ = inputs.shape
        emb = sd[p + ".mod_emb.weight"][mod_idx][None, None, :].expand(B, T, -1).clone()
        if e["pos"]:
            emb = emb + sd[p + ".pos_embed.weight"][ts]
        return O.dropout(x, e["dropout"], training, dropout_fn, site_key), emb
    return embed


ASYM = dict(enc_emb=dict(act="tanh", pos=False, bias=False, scale=None))
BF16_MODELS = {"softsign": {}, "ASYM": ASYM, "GELU": dict(enc_emb=dict(act="gelu"), dec_emb=dict(act="gelu"))}
# (B, T, n_ap, model_config keywords): the tiny size; the default widths (H 256, 668 neurons: the K = 668 / 1336 tokeniser GEMMs)
BF16_SIZES = {"tiny": (2, 8, 12, dict(H=32, heads=4, inter=64, n_enc=1, n_dec=1, max_F=8)), "default_widths": (4, 100, 668, dict(n_enc=1, n_dec=1))}


@pytest.mark.parametrize("size", list(BF16_SIZES))
@pytest.mark.parametrize("name", list(BF16_MODELS))
def test_bf16_step_vs_fp64_restatement(name, size):
    """One bf16 training step (dropout 0) against the fp64 restatement at the bound tests/model_checks.py::check_bf16 holds the
    softsign model to: loss within 2e-2, worst gradient cosine > 0.995 (> 0.98 under 256 elements), worst norm error < 5e-2.  `softsign`
    is the default model in the same run, the yardstick for what the saved bf16 pre-activation of the other activations costs."""
    B, T, n_ap, kw = BF16_SIZES[size]
    mc = sides(dropout=0.0, emb_dropout=0.0, **BF16_MODELS[name], **kw)
    batch = O.synth_batch(B, T, n_ap, 2, seed=6)
    out, named, ref, grads, eng = engine_step_and_oracle(mc, n_ap, 2, batch, "token_masking", "bf16", 3, embed=embed_ref(mc))
    st = bf16_stats(out, named, ref, grads)
    print(f"bf16 {name} {size}: {st}")
    if name != "softsign":      # the forward stores z, the backward reads it: the plan's buffers say so
        want_z = {"ASYM": {"encoder/z/0", "encoder/z/1"}, "GELU": {f"{s}/z/{m}" for s in ("encoder", "decoder") for m in (0, 1)}}[name]
        assert {k for k in eng._last["b"] if "/z/" in k and not k.startswith("d/")} == want_z
    assert st["loss"] < 2e-2, st
    assert st["cos_big"] > 0.995 and st["cos_small"] > 0.98, st
    assert st["norm"] < 5e-2, st


# ---------------------------------------------------------------------------------------------- dropout, resume, graph replay
def test_fp32_dropout_step_without_position_tables():
    """fp32, tiny, dropout 0.4 / embedder dropout 0.2, pos: false on both sides and a bias-free relu tokeniser on the decoder: the keep
    masks are read off the kernels (tests/dropout_refs.py) and fed to the fp64 restatement; loss, predictions and every gradient at the
    bounds of test_dropout_step_gpu.py::test_fp32_dropout_step_vs_oracle_fed_the_steps_masks."""
    kw = dict(H=32, heads=4, inter=64, n_enc=1, n_dec=1, max_F=8, dropout=0.4, emb_dropout=0.2)
    mc = sides(enc_emb=dict(pos=False), dec_emb=dict(pos=False, bias=False, act="relu"), **kw)
    batch = O.synth_batch(3, 8, 12, 2, seed=4, pad=[0, 3, 1])
    out, named, ref, grads, eng = engine_step_and_oracle(mc, 12, 2, batch, "token_masking", "fp32", 0, embed=embed_ref(mc))
    assert len(eng.dropout_sites(3, 8)) == 4 + 3 + 5
    assert not any("pos_embed" in k for k in named) and "decoder_embeddings.ap.embedder.token_embed.bias" not in named
    assert out.loss.item() == pytest.approx(ref["loss"].item(), rel=2e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(ref["mod_n_examples"][m])
        assert out.mod_loss[m].item() == pytest.approx(ref["mod_loss"][m].item(), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), ref["mod_preds"][m].detach().cpu().numpy(), rtol=1e-4, atol=2e-5)
    for k, g in named.items():
        r = grads[k].cpu().numpy()
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(r).max(), err_msg=k)


def test_asym_case_resume_from_train_state_is_bit_identical(tmp_path):
    """The ASYM tiny model in fp32: 6 steps in one go == 3 steps, save_model + save_train_state, fresh objects restored from the files
    (load_train_state), 3 more steps."""
    def after_save(ck):
        keys = list(ck["model"].state_dict())
        assert "encoder_embeddings.ap.embedder.pos_embed.weight" not in keys and "decoder_embeddings.ap.embedder.pos_embed.weight" in keys
        assert "encoder_embeddings.ap.embedder.token_embed.bias" not in keys

    def after_restore(m2, opt2, sch2):
        enc, dec = (m2._engine.cfg.side(s) for s in ("encoder", "decoder"))
        assert (enc.embed_act, enc.embed_pos, enc.embed_bias, dec.embed_act, dec.embed_pos, dec.embed_bias) == ("tanh", False, False, "softsign", True, True)

    resume_roundtrip(tmp_path, case_config("ASYM", n_enc=2, n_dec=2), B=2, after_save=after_save, after_restore=after_restore)


def test_asym_case_graph_replay_gives_the_eager_losses(monkeypatch):
    """The ASYM tiny model, 5 optimiser steps in fp32: with hipGraph replay (the plan runs eagerly once, is captured on the second step and
    replayed from the third) the losses are the ones of MMFM_GRAPH=0, bit for bit."""
    g = load_json("embedder_opts_curve.json")["ASYM"]
    graph_replay_matches_eager(monkeypatch, lambda: build_model(case_config("ASYM"), g["n_ap"], g["n_beh"], seed=g["model_seed"]), g)
