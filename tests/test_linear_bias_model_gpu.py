"""transformer.attention_bias / transformer.mlp_bias = false on the MI355X, whole models: the fp32 engine against the reference's own
forward / backward and 50-step curves (tests/golden/linear_bias_*, scripts/make_linear_bias_goldens.py), the bf16 fused path against
the un-fused kernels, d_model 512 / dh 64 in bf16 against the fp32 engine, the flat gradient buffer, checkpoint resume."""
import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
from helpers import build_model, model_config, tiny_config
from model_checks import check_fixture_case, cosine, resume_roundtrip, run_curve, to_dev
from multi_modal_foundation_model_amd import ops as K
from multi_modal_foundation_model_amd.engine import _align
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu
CASES = ("FT", "TF", "FF", "FF_TT")
OFF = dict(attn_bias=False, mlp_bias=False)
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("linear_bias_fwd_bwd.npz")
    return _Z


def case_config(meta, case, **kw):
    (ea, em), (da, dm) = meta["switches"][case]
    return tiny_config(attn_bias=(ea, da), mlp_bias=(em, dm), **kw)


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("objective", ["encoding", "decoding", "token_masking"])
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """Loss, counts (exact), predictions, every gradient norm and (token_masking) every gradient tensor; the tolerances of the
    mlp_act_fwd_bwd.npz test."""
    z, meta = fixture()
    check_fixture_case(build_model(case_config(meta, case), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"]), z, meta, case, objective)


@pytest.mark.parametrize("norm", ["layernorm", "scalenorm"])
def test_loss_curve_tiny_50_steps_vs_reference_fixture(norm):
    g = load_json("linear_bias_curve.json")[f"FF/{norm}"]
    model = build_model(tiny_config(scalenorm=g["scalenorm"], **OFF), g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    assert len(model.state_dict()) == g["n_state_keys"]
    losses = run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- bf16: fused against un-fused
@pytest.mark.parametrize("norm", ["layernorm", "scalenorm"])
def test_bf16_fused_path_matches_unfused_kernels(monkeypatch, norm):
    """H = 256 / inter 512, (F, F), dropout 0: MMFM_FUSED=15 against MMFM_FUSED=0 within the bound of the existing fused-vs-unfused
    tests (loss 3e-3, gradient cosine 0.995, 0.98 for tensors below 256 elements).  The fused plan hands the kernels no bias: every
    mmfm_mlp_fwd gets b_down = NULL (and b_up = NULL behind a ScaleNorm), every norm-fed gradient launch dbias = NULL except the one of
    decoder_proj_context, which keeps its bias."""
    batch = O.synth_batch(16, 100, 668, 2, seed=0)
    sn = norm == "scalenorm"
    seen = dict(mlp=[], lng=[])
    mlp_fwd, lng = K.mlp_fwd, (K.sn_linear_grad if sn else K.ln_linear_grad)
    res = {}
    for mode in ("0", "15"):
        monkeypatch.setenv("MMFM_FUSED", mode)
        with monkeypatch.context() as mp:
            mp.setattr(K, "mlp_fwd", lambda d, plan=None: (seen["mlp"].append((d.b_up, d.b_down)), mlp_fwd(d, plan=plan))[1])
            if sn:
                mp.setattr(K, "sn_linear_grad", lambda Gdb, W, g, N, Kd, dW, dbias, *a, **kw:
                           (seen["lng"].append(dbias), lng(Gdb, W, g, N, Kd, dW, dbias, *a, **kw))[1])
            else:
                mp.setattr(K, "ln_linear_grad", lambda Gdb, W, g, b, N, Kd, dW, dbias, *a, **kw:
                           (seen["lng"].append(dbias), lng(Gdb, W, g, b, N, Kd, dW, dbias, *a, **kw))[1])
            model = build_model(model_config(dropout=0.0, emb_dropout=0.0, scalenorm=sn, **OFF), 668, 2, seed=42)
            model.compute_dtype = "bf16"
            model.cuda().train()
            model.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            o = model(to_dev(O.make_mod_dict(batch, "token_masking")))
            o.loss.backward()
            res[mode] = (o.loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
            assert not any(k.endswith(".bias") and (".attn." in k or ".cross_attn." in k or ".mlp." in k) for k in res[mode][1])
            eng = model._engine
            assert eng.G.numel() == eng.layout.n
        del model, eng
        torch.cuda.empty_cache()
    assert len(seen["mlp"]) == 10 and all(bd is None and ((bu is None) == sn) for bu, bd in seen["mlp"]), seen["mlp"]
    # ln1 x 10, ln2 x 10, query_norm / context_norm x 5 each, encoder_norm -> decoder_proj_context (keeps its bias; a LayerNorm always)
    assert len(seen["lng"]) == 30 + (0 if sn else 1) and sum(d is not None for d in seen["lng"]) == (0 if sn else 1), seen["lng"]
    l0, g0 = res["0"]
    l1, g1 = res["15"]
    assert np.isfinite(l0) and l1 == pytest.approx(l0, rel=3e-3)
    assert list(g0) == list(g1)
    for k in g0:
        if g0[k].abs().max() == 0:
            assert g1[k].abs().max() == 0, k
            continue
        c = cosine(g0[k], g1[k])
        assert c > (0.995 if g0[k].numel() >= 256 else 0.98), f"{k}: cosine {c}"


def test_bf16_step_at_d_model_512_dh64_matches_fp32_engine():
    """One optimiser-free step at H = 512 / 8 heads (dh 64) / inter 1024, (F, F), two layers a side, R = 1600 rows (the 256-tile dX
    GEMM's threshold is 1024): the bf16 loss within 2e-2 of the fp32 engine's, the per-step bound of the config-5 bf16-vs-fp32 test."""
    batch = O.synth_batch(8, 100, 668, 2, seed=0)
    res = {}
    for dtype in ("fp32", "bf16"):
        model = build_model(model_config(H=512, heads=8, inter=1024, n_enc=2, n_dec=2, dropout=0.0, emb_dropout=0.0, **OFF), 668, 2, seed=3)
        model.compute_dtype = dtype
        model.cuda().train()
        torch.manual_seed(1)
        out = model(to_dev(O.make_mod_dict(batch, "token_masking")))
        out.loss.backward()
        grads = {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}
        res[dtype] = (out.loss.item(), grads)
        del model
        torch.cuda.empty_cache()
    l32, l16 = res["fp32"][0], res["bf16"][0]
    print("fp32", l32, "bf16", l16, "relative gap", abs(l16 - l32) / abs(l32))
    assert np.isfinite(l32) and np.isfinite(l16)
    assert abs(l16 - l32) / abs(l32) < 2e-2
    for k, g in res["bf16"][1].items():
        assert torch.isfinite(g).all(), k
        assert not k.endswith("mlp.up_proj.bias") and not k.endswith("attn.query.bias")


# ---------------------------------------------------------------------------------------------- flat buffers
@pytest.mark.parametrize("case", CASES)
def test_gradient_buffer_has_no_orphan_elements(case):
    """G.numel() is the aligned sum of the layout, and after a backward every element outside a parameter (alignment padding) is
    still zero: no kernel wrote a bias gradient that has no owner."""
    _, meta = fixture()
    model = build_model(case_config(meta, case, n_enc=2, n_dec=2), 12, 2, seed=7).cuda().train()
    out = model(to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=0), "encoding")))
    out.loss.backward()
    eng = model._engine
    lay = eng.layout
    assert eng.G.numel() == eng.P.numel() == lay.n
    assert lay.n == _align(sum(_align(int(np.prod(s))) for _, s in lay.entries.values()), 64)
    owned = torch.zeros(lay.n, dtype=torch.bool)
    for off, shape in lay.entries.values():
        owned[off:off + int(np.prod(shape))] = True
    assert (eng.G.cpu()[~owned] == 0).all()
    assert set(dict(model.named_parameters())) == set(lay.entries)
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == eng.Gv(k).data_ptr(), k


# ---------------------------------------------------------------------------------------------- resume
def test_bias_free_resume_from_train_state_is_bit_identical(tmp_path):
    """(F, F): 6 steps in one go == 3 steps, save_model + train state, fresh objects restored from the files, 3 more steps
    (bf16, dropout on); the checkpoint's state dict carries no governed bias key."""
    def after_save(ck):
        keys = list(ck["model"].state_dict())
        assert not any(k.endswith(".bias") and (".attn." in k or ".cross_attn." in k or ".mlp." in k) for k in keys)
        assert "decoder_proj_context.bias" in keys and "encoder.0.ln1.bias" in keys

    resume_roundtrip(tmp_path, tiny_config(n_enc=2, n_dec=2, dropout=0.4, emb_dropout=0.2, **OFF), dtype="bf16", after_save=after_save)
