"""Encoder and decoder sections of the model config that differ, on the MI355X, whole models: the fp32 engine against the reference's own
forward / backward and 50-step curves (tests/golden/side_config_*, scripts/make_side_config_goldens.py); a bf16 model whose encoder runs
the row-owner MLP kernels (8 heads, inter 512) and whose decoder the un-fused GEMMs (4 heads = dh 64, inter 1024, relu) against the fp32
engine and against the un-fused kernels, with the launches read off the plan; dropout per side; checkpoint resume and hipGraph replay."""
import numpy as np
import pytest
import torch

from conftest import load_json
from helpers import build_model
from model_checks import (check_fixture_case, cosine, fixture_batch, graph_replay_matches_eager, resume_roundtrip, run_curve,
                          to_dev)
from oracle import mm_oracle as O
from side_config import CASES, OBJECTIVES, case_config, fixture, sides

pytestmark = pytest.mark.gpu
B, T, N_AP, N_BEH = 4, 100, 48, 2          # the bf16 tests' batch: R = 800 rows of H = 256
MIXED = dict(dec=dict(n_heads=4, inter_size=1024, act="relu"), n_enc=2, n_dec=2)      # on the YAML's encoder: 8 heads, inter 512, gelu


def attn_descs(plan, which="fwd"):
    """The attention descriptors of the forward in launch order: every encoder layer's self-attention, then per decoder layer its
    self-attention and its cross-attention."""
    entries = plan["fwd"] if which == "fwd" else [e for _, seg in plan["bwd"] for e in seg]
    return [keep[0] for fn, _, keep in entries if fn.__name__ == ("mmfm_attn_fwd" if which == "fwd" else "mmfm_attn_bwd")]


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """Loss, counts (exact), predictions, every gradient norm and (ALL / token_masking) every gradient tensor; the tolerances of
    test_linear_bias_model_gpu.py::test_tiny_forward_backward_vs_reference_fixture."""
    z, meta = fixture()
    check_fixture_case(build_model(case_config(case), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"]), z, meta, case, objective)


def test_drop0_control_is_the_unmixed_model():
    """DROP0 names dropout 0 on both sides, which the tiny config has anyway: config, parameters, loss and gradients are the un-mixed
    model's, bit for bit."""
    from helpers import tiny_config
    z, meta = fixture()
    batch = fixture_batch(z)
    res = []
    for mc in (case_config("DROP0"), tiny_config()):
        model = build_model(mc, meta["n_ap"], meta["n_beh"], seed=meta["model_seed"]).cuda().train()
        torch.manual_seed(11)
        out = model(to_dev(O.make_mod_dict(batch, "token_masking")))
        out.loss.backward()
        res.append((model._engine.cfg, out.loss.item(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    (c0, l0, g0), (c1, l1, g1) = res
    assert c0 == c1 and l0 == l1 and list(g0) == list(g1)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


@pytest.mark.parametrize("case", ["ALL", "HEADS"])
def test_loss_curve_tiny_50_steps_vs_reference_fixture(case):
    g = load_json("side_config_curve.json")[case]
    model = build_model(case_config(case), g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    assert len(model.state_dict()) == g["n_state_keys"]
    losses = run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- bf16: the fused path per side
def one_step(mc, dtype, seed=42, backward=True):
    model = build_model(mc, N_AP, N_BEH, seed=seed)
    model.compute_dtype = dtype
    model.cuda().train()
    torch.manual_seed(1)
    out = model(to_dev(O.make_mod_dict(O.synth_batch(B, T, N_AP, N_BEH, seed=0), "token_masking")))
    grads = None
    if backward:
        out.loss.backward()
        grads = {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}
    return model, out.loss.item(), grads


def test_bf16_mixed_model_vs_fp32_engine_and_unfused_kernels(monkeypatch):
    """H 256, dropout 0, encoder 8 heads / inter 512 / gelu, decoder 4 heads (dh 64) / inter 1024 / relu.  At R = 800 rows the shape's
    own mask is 11 (Engine._fused_mask: the MLP bit is off below 12,288 rows), so the fused run names MMFM_FUSED=15, the mask the default
    takes from there on.  Its plan: encoder layers launch mmfm_mlp_fwd, decoder layers the up / down GEMMs with relu, decoder attention
    sites have 4 heads.  bf16 against the fp32 engine on the same weights and batch: DESIGN.md section 3's bound (loss 2e-2 relative,
    gradient cosine >= 0.99 for tensors of >= 256 elements); MMFM_FUSED=15 against 0: loss 3e-3, cosine 0.995 (0.98 below 256); key.bias,
    whose true gradient is zero, is left out of both cosine checks."""
    from multi_modal_foundation_model_amd import _lib as L
    mc = sides(dropout=0.0, emb_dropout=0.0, **MIXED)
    monkeypatch.delenv("MMFM_FUSED", raising=False)
    _, l32, g32 = one_step(mc, "fp32")
    monkeypatch.setenv("MMFM_FUSED", "0")
    m0, l0, g0 = one_step(mc, "bf16")
    assert m0._engine._last["fused"] == 0
    del m0
    monkeypatch.setenv("MMFM_FUSED", "15")
    m15, l15, g15 = one_step(mc, "bf16")
    eng = m15._engine
    plan = eng._last
    assert plan["fused"] == 15 and eng.fused_mlp("encoder", 15) and not eng.fused_mlp("decoder", 15)
    # ---- the launches
    names = [fn.__name__ for fn, _, _ in plan["fwd"]]
    attn_at = [i for i, n in enumerate(names) if n == "mmfm_attn_fwd"]
    descs = attn_descs(plan)
    assert [(d.heads, d.dh) for d in descs] == [(8, 32)] * 2 + [(4, 64)] * 4
    assert [(d.heads, d.dh) for d in attn_descs(plan, "bwd")] == [(4, 64)] * 4 + [(8, 32)] * 2
    first_dec = attn_at[2]
    mlp_at = [i for i, n in enumerate(names) if n == "mmfm_mlp_fwd"]
    assert len(mlp_at) == 2 and all(i < first_dec for i in mlp_at), "the encoder layers' MLP blocks, and nobody else's, run mmfm_mlp_fwd"
    assert [keep[0].act for fn, _, keep in plan["fwd"] if fn.__name__ == "mmfm_mlp_fwd"] == [L.MLP_GELU] * 2
    gemms = [(i, keep[0]) for i, (fn, _, keep) in enumerate(plan["fwd"]) if fn.__name__ == "mmfm_gemm"]
    up = [(i, d) for i, d in gemms if (d.N, d.K) == (1024, 256)]
    down = [(i, d) for i, d in gemms if (d.N, d.K) == (256, 1024)]
    assert len(up) == len(down) == 2 and all(i > first_dec for i, _ in up + down)
    assert all(d.act == L.ACT_RELU and d.M == B * 2 * T for _, d in up)
    bwd_names = [fn.__name__ for _, seg in plan["bwd"] for fn, _, _ in seg]
    assert bwd_names.count("mmfm_mlp_bwd") == 2
    # ---- numbers
    print("loss fp32", l32, "bf16 fused", l15, "bf16 un-fused", l0)
    assert np.isfinite(l32) and abs(l15 - l32) / abs(l32) < 2e-2 and abs(l0 - l32) / abs(l32) < 2e-2
    assert l15 == pytest.approx(l0, rel=3e-3)
    assert list(g32) == list(g15) == list(g0)
    # softmax is invariant to a key bias: the true gradient of every key.bias is 0 and what the engines hold is rounding noise, whose
    # direction means nothing (measured here: cosine -0.05 for encoder.0.attn.key.bias) - skipped, as in every cosine test of the suite
    compared = [k for k in g32 if not k.endswith("key.bias")]
    assert len(g32) - len(compared) == 2 + 2 * 2
    worst = min(((cosine(g32[k], g15[k]), k) for k in compared if g32[k].numel() >= 256))
    print("worst gradient cosine bf16 vs fp32", worst)
    for k in g32:
        assert torch.isfinite(g15[k]).all(), k
    for k in compared:
        if g32[k].numel() >= 256:
            c = cosine(g32[k], g15[k])
            assert c >= 0.99, f"{k}: cosine {c} against the fp32 engine"
        c = cosine(g0[k], g15[k])
        assert c > (0.995 if g0[k].numel() >= 256 else 0.98), f"{k}: cosine {c} fused against un-fused"


# ---------------------------------------------------------------------------------------------- dropout per side
def forward_twice(model):
    losses = []
    for _ in range(2):
        torch.manual_seed(1)
        out = model(to_dev(O.make_mod_dict(O.synth_batch(B, T, N_AP, N_BEH, seed=0), "token_masking")))
        losses.append(out.loss.item())
    return losses


@pytest.mark.parametrize("dropped", ["encoder", "decoder"])
def test_dropout_on_one_side_only(monkeypatch, dropped):
    """transformer.dropout 0.4 on one side, 0 on the other (embedder.dropout 0 on both): the plan holds keep-bit workspaces - and with them
    generator launches, which mmfm_attn_fwd issues where the descriptor names a workspace - for the dropped side's sites only, sized by
    that side's head count; every descriptor of the other side has drop_p = drop_o = 0; the RNG state advances."""
    from multi_modal_foundation_model_amd import ops as K
    monkeypatch.delenv("MMFM_FUSED", raising=False)
    p = dict(encoder=(0.4, 0.0), decoder=(0.0, 0.4))[dropped]
    mc = sides(enc=dict(dropout=p[0]), dec=dict(dropout=p[1], **MIXED["dec"]), emb_dropout=0.0, n_enc=2, n_dec=2)
    model, l1, grads = one_step(mc, "bf16")
    eng = model._engine
    plan = eng._last
    Lq = 2 * T
    for which in ("fwd", "bwd"):
        descs = attn_descs(plan, which)
        enc, dec = (descs[:2], descs[2:]) if which == "fwd" else (descs[4:], descs[:4])
        for side_descs, want, heads in ((enc, p[0], 8), (dec, p[1], 4)):
            for d in side_descs:
                assert d.heads == heads
                assert d.drop_p.p == pytest.approx(want) and d.drop_o.p == pytest.approx(want)
                assert (d.keepbits is not None) == (want > 0) and (d.drop_p.state is not None) == (want > 0)
    keeps = {k: v for k, v in plan["b"].items() if k.endswith("/keep")}
    want_keys = {"enc0/sa/keep", "enc1/sa/keep"} if dropped == "encoder" else {f"dec{i}/{s}/keep" for i in (0, 1) for s in ("sa", "xa")}
    assert set(keeps) == want_keys
    assert all(v.numel() == K.attn_keepbits_bytes(B, 8 if dropped == "encoder" else 4, Lq, Lq) for v in keeps.values())
    sites = {s["key"]: s for s in eng.dropout_sites(B, T)}
    assert sites and all(k.startswith(dropped[:3]) and s["p"] == pytest.approx(0.4) for k, s in sites.items())
    assert all(torch.isfinite(g).all() for g in grads.values())
    a, b = forward_twice(model)
    print("two training forwards", a, b)
    assert np.isfinite(a) and np.isfinite(b) and a != b


def test_no_dropout_anywhere_is_deterministic_and_decoder_embedder_dropout_is_read():
    """Dropout 0 on every site: two training forwards of one batch are bit-identical (nothing advances the RNG state).  Decoder
    embedder.dropout 0.5 with everything else 0 - the value used to be ignored, the encoder's was read for both - changes the loss and
    makes two forwards differ."""
    mc0 = sides(dropout=0.0, emb_dropout=0.0, **MIXED)
    model, l0, _ = one_step(mc0, "bf16", backward=False)
    a, b = forward_twice(model)
    assert a == b == l0
    assert not model._engine.dropout_sites(B, T)
    del model
    mc1 = sides(dec_emb=dict(dropout=0.5), dropout=0.0, emb_dropout=0.0, **MIXED)
    model, l1, _ = one_step(mc1, "bf16", backward=False)
    a, b = forward_twice(model)
    print("no dropout", l0, "decoder embedder.dropout 0.5", l1, a, b)
    assert np.isfinite(l1) and l1 != l0 and a != b
    sites = model._engine.dropout_sites(B, T)
    assert sorted(s["key"] for s in sites) == ["decoder/embdrop/0", "decoder/embdrop/1"] and all(s["p"] == 0.5 for s in sites)


# ---------------------------------------------------------------------------------------------- resume, graph replay
def test_all_case_resume_from_train_state_is_bit_identical(tmp_path):
    """The ALL tiny model in fp32: 6 steps in one go == 3 steps, save_model + save_train_state, fresh objects restored from the files
    (load_train_state), 3 more steps."""
    def after_save(ck):
        keys = list(ck["model"].state_dict())
        assert "encoder.1.ln1.scale" in keys and "decoder.1.ln1.weight" in keys

    def after_restore(m2, opt2, sch2):
        enc, dec = (m2._engine.cfg.side(s) for s in ("encoder", "decoder"))
        assert (enc.heads, dec.heads, enc.inter, dec.inter, enc.norm, dec.norm) == (4, 2, 64, 128, "scalenorm", "layernorm")

    resume_roundtrip(tmp_path, case_config("ALL", n_enc=2, n_dec=2), B=2, after_save=after_save, after_restore=after_restore)


def test_all_case_graph_replay_gives_the_eager_losses(monkeypatch):
    """The ALL tiny model, 5 optimiser steps in fp32: with hipGraph replay (the plan runs eagerly once, is captured on the second step and
    replayed from the third) the losses are the ones of MMFM_GRAPH=0, bit for bit."""
    g = load_json("side_config_curve.json")["ALL"]
    graph_replay_matches_eager(monkeypatch, lambda: build_model(case_config("ALL"), g["n_ap"], g["n_beh"], seed=g["model_seed"]), g)
