"""The grouped context side of cross-attention in the step plan (MMFM_CTX_GROUP): one mmfm_rowgemm_groups launch writes every
decoder layer's keys / values, one at the head of the bridge segment sums their dX products behind one norm backward.

A d_model-256 / inter-512 model with 2 + 2 layers, B = 4, T = 12, bf16, dropout 0.1, one training step with the switch on against the
switch off: the forward is bit-identical, so is every gradient that does not pass through d/ctx, and both runs meet the fp64 oracle at
the bounds of tests/model_checks.py::check_bf16."""
import pytest
import torch

from helpers import build_model, model_config
from model_checks import bf16_stats, check_bf16, cosine, engine_step_and_oracle, to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

B, T, N_AP, N_BEH, N_DEC = 4, 12, 12, 2, 2
GROUPS = "mmfm_rowgemm_groups"


def names(entries):
    return [fn.__name__ for fn, _, _ in entries]


def bwd_names(plan):
    return [n for _, seg in plan["bwd"] for n in names(seg)]


@pytest.fixture(scope="module")
def runs():
    """The step with MMFM_CTX_GROUP = 0 and = 1: (output, gradients, oracle output, oracle gradients, engine) each."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for mode in ("0", "1"):
            mp.setenv("MMFM_CTX_GROUP", mode)
            mc = model_config(n_enc=2, n_dec=N_DEC, dropout=0.1)
            out[mode] = engine_step_and_oracle(mc, N_AP, N_BEH, O.synth_batch(B, T, N_AP, N_BEH, seed=6), "token_masking", "bf16", 3)
    finally:
        mp.undo()
    return out


def test_plan_launches(runs):
    p0, p1 = runs["0"][4]._last, runs["1"][4]._last
    assert GROUPS not in names(p0["fwd"]) and GROUPS not in bwd_names(p0)
    assert names(p1["fwd"]).count(GROUPS) == 1 and bwd_names(p1).count(GROUPS) == 1
    assert len(p1["fwd"]) == len(p0["fwd"]) - (N_DEC - 1)
    assert len(bwd_names(p1)) == len(bwd_names(p0)) - (N_DEC - 1)
    # the segments and their order stay; the grouped dX launch heads the bridge segment
    assert [s for s, _ in p1["bwd"]] == [s for s, _ in p0["bwd"]]
    bridge = dict(p1["bwd"])["bridge"]
    assert names(bridge)[0] == GROUPS
    for seg, entries in p1["bwd"]:
        if seg != "bridge":
            assert GROUPS not in names(entries)
    assert {f"d/kvc/{i}" for i in range(N_DEC)} <= set(p1["b"]) and "d/kvc" not in p1["b"] and "d/kvc" in p0["b"]


def test_forward_bit_identical(runs):
    (o0, _, _, _, e0), (o1, _, _, _, e1) = runs["0"], runs["1"]
    assert torch.equal(o0.loss, o1.loss)
    for m in ("ap", "behavior"):
        assert torch.equal(o0.mod_preds[m], o1.mod_preds[m]), m
    b0, b1 = e0._last["b"], e1._last["b"]
    # every buffer the forward writes (d/: gradients, ws/: workspaces; */keep: keep-bit tiles, allocated with a tail no kernel writes,
    # and enc_out, which only the un-fused encoder_norm writes)
    fwd = lambda b: [k for k in b if not k.startswith(("d/", "ws/")) and not k.endswith("/keep") and k != "enc_out"]
    fwd_keys = fwd(b0)
    assert set(fwd_keys) == set(fwd(b1))
    assert any(k.endswith("/kvc") for k in fwd_keys) and "dec0/cn/xh" in fwd_keys
    for k in fwd_keys:
        assert torch.equal(b0[k], b1[k]), k


def test_gradients_off_the_context_path_bit_identical(runs):
    """d/ctx reaches the encoder, its norm, decoder_proj_context and the encoder's tokenisers (with the modality rows they share); every
    other gradient - the decoder's layers, norm, heads and tokenisers - sees the same bits in both plans."""
    g0, g1 = runs["0"][1], runs["1"][1]
    off = [k for k in g0 if k.startswith(("decoder.", "decoder_norm", "decoder_embeddings.")) and "mod_emb" not in k]
    assert len(off) > 40 and any("cross_attn.key" in k for k in off) and any("context_norm" in k for k in off)
    for k in off:
        assert torch.equal(g0[k], g1[k]), k
    on = [k for k in g0 if k.startswith(("encoder.", "encoder_norm", "decoder_proj_context"))]
    assert on and all(float(g1[k].abs().max()) > 0 for k in on if not k.endswith("key.bias"))


@pytest.mark.parametrize("mode", ["0", "1"])
def test_step_vs_oracle(runs, mode):
    out, named, ref, grads, _ = runs[mode]
    check_bf16(bf16_stats(out, named, ref, grads), f"MMFM_CTX_GROUP={mode}")


def test_threshold_keeps_small_plans(monkeypatch):
    """With the switch unset this size is far below the row threshold: the per-layer launches."""
    monkeypatch.delenv("MMFM_CTX_GROUP", raising=False)
    model = build_model(model_config(n_enc=2, n_dec=N_DEC, dropout=0.1), N_AP, N_BEH, seed=3)
    model.compute_dtype = "bf16"
    model.cuda()
    plan = model.engine()._plan(B, T, True, True)
    assert GROUPS not in names(plan["fwd"]) and GROUPS not in bwd_names(plan)
    ctx = [keep[0] for fn, _, keep in plan["fwd"] if fn.__name__ == "mmfm_rowgemm" and keep[0].ln and keep[0].N == 512]
    assert len(ctx) == N_DEC


def test_scalenorm_bias_free_decoder(monkeypatch):
    """ScaleNorm everywhere, attention without biases, a bias-free decoder MLP, SiLU: the grouped launches take the ScaleNorm prologue /
    backward and NULL biases.  (The fp64 oracle has no ScaleNorm: the per-layer plan is the reference.)  Forward and the gradients off the
    context path bit-identical; the encoder's gradients, which differ by the bf16 roundings of d/ctx only, at a cosine above 0.9999."""
    mc_kw = dict(n_enc=2, n_dec=N_DEC, dropout=0.1, scalenorm=True, attn_bias=False, mlp_bias=(True, False), act="silu")
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MMFM_CTX_GROUP", mode)
        model = build_model(model_config(**mc_kw), N_AP, N_BEH, seed=3)
        model.compute_dtype, model.engine_seed = "bf16", 77
        model.cuda().train()
        torch.manual_seed(5)
        out = model(to_dev(O.make_mod_dict(O.synth_batch(B, T, N_AP, N_BEH, seed=6), "token_masking")))
        out.loss.backward()
        torch.cuda.synchronize()
        res[mode] = (out.loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}, model._engine._last)
    (l0, g0, p0), (l1, g1, p1) = res["0"], res["1"]
    assert names(p1["fwd"]).count(GROUPS) == 1 and bwd_names(p1).count(GROUPS) == 1 and GROUPS not in names(p0["fwd"])
    grouped = [keep[0] for fn, _, keep in p1["fwd"] if fn.__name__ == GROUPS][0]
    assert grouped.ln == 2 and grouped.groups == N_DEC and not grouped.bias[0]
    assert torch.equal(l0, l1) and bool(torch.isfinite(l1))
    for i in range(N_DEC):
        assert torch.equal(p0["b"][f"dec{i}/kvc"], p1["b"][f"dec{i}/kvc"])
    for k in g0:
        if k.startswith(("decoder.", "decoder_norm")):
            assert torch.equal(g0[k], g1[k]), k
        elif k.startswith(("encoder.", "encoder_norm", "decoder_proj_context")) and float(g0[k].abs().max()) > 0:
            assert cosine(g0[k], g1[k]) > 0.9999, k
