"""One whole training step with dropout ON against the oracle in double precision, fed the step's own masks.

torch's RNG cannot reproduce the engine's masks and does not have to: every mask is a pure function of (state, site, index).  After
one forward + backward the engine's RNG state is still the one the step used, so every site's multiplier is read back off the kernels
(tests/dropout_refs.py: the flat hash through mmfm_dropout_apply, attention drop_p from the engine's own keep-bit workspaces or the
one-hot-V read-out on the kernel family the plan runs, the fused MLP's RowDrop through the backward's t1) and handed to
oracle.mm_oracle.forward through its dropout_fn hook.  The token masks are the ones the model's masker drew for the step.  What the
oracle then computes is the step the engine claims to have run: loss, predictions and every parameter gradient must agree to the
bounds of the dropout-free tests.  A backward that keys a site differently from its forward, a counter built from the wrong stride, a
survivor scale applied twice or not at all, or a row-keyed hash off by a row each give a biased gradient that still trains - and
fail here."""
import numpy as np
import pytest

import dropout_refs as DR
from helpers import model_config, tiny_config
from model_checks import bf16_stats, check_bf16, engine_step_and_oracle
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

VARIANTS = {"base": (dict(), None), "pad": (dict(), [0, 3, 1]), "sep": (dict(sep=True), [0, 2, 0]), "causal": (dict(causal=True), [1, 0, 0]),
            "deep": (dict(n_enc=2, n_dec=2), [0, 0, 5])}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("objective", ["encoding", "token_masking"])
def test_fp32_dropout_step_vs_oracle_fed_the_steps_masks(variant, objective):
    """fp32 parity engine, tiny config (H 32, 4 heads, dh 8: attention.hip's fp32 kernels, flat-hash dropout everywhere), dropout 0.4 /
    embed dropout 0.2: loss, per-modality loss, n, predictions and every parameter gradient at the bounds of
    test_tiny_forward_backward_vs_reference_fixture."""
    kw, pad = VARIANTS[variant]
    mc = tiny_config(dropout=0.4, emb_dropout=0.2, **kw)
    batch = O.synth_batch(3, 8, 12, 2, seed=4, pad=pad)
    out, named, ref, grads, eng = engine_step_and_oracle(mc, 12, 2, batch, objective, "fp32", 0)
    sites = eng.dropout_sites(3, 8)
    n_layers = 2 if variant == "deep" else 1
    assert len(sites) == 4 + (3 + 5) * n_layers and all(s["kind"] in ("flat", "attn") for s in sites)
    assert out.loss.item() == pytest.approx(ref["loss"].item(), rel=2e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(ref["mod_n_examples"][m])
        assert out.mod_loss[m].item() == pytest.approx(ref["mod_loss"][m].item(), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), ref["mod_preds"][m].detach().cpu().numpy(), rtol=1e-4, atol=2e-5)
    for k, g in named.items():
        r = grads[k].cpu().numpy()
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(r).max(), err_msg=k)


@pytest.mark.parametrize("dropout", ["off", "on"])
def test_bf16_fused_dropout_step_vs_oracle_fed_the_steps_masks(monkeypatch, dropout):
    """bf16, every row-owner group fused (MMFM_FUSED=15), default widths (hidden 256, 8 heads: the dh-32 keep-bit attention pair, the
    fused MLP's RowDrop), n_enc = n_dec = 2, B = 16, T = 100, two padded trials, dropout 0.4 / 0.2, against the fp64 oracle at the bounds
    test_bf16_fused_row_owner_path_matches_unfused_kernels states: loss within 2e-2, cosine > 0.995 (> 0.98 under 256 elements), norm
    within 5e-2, key.bias skipped.  `off` is the same comparison at dropout 0: what bf16 alone costs against fp64.
    Measured on the MI355X (worst over tensors):
      dropout off: loss error 3.0e-5, cosine 0.999990 (>= 256 elements) / 0.999977 (< 256), norm error 3.7e-3
      dropout on : loss error 1.5e-5, cosine 0.999990 / 0.999976, norm error 3.9e-3."""
    monkeypatch.setenv("MMFM_FUSED", "15")
    on = dropout == "on"
    mc = model_config(n_enc=2, n_dec=2) if on else model_config(n_enc=2, n_dec=2, dropout=0.0, emb_dropout=0.0)
    pad = [0] * 16
    pad[3], pad[15] = 10, 37
    batch = O.synth_batch(16, 100, 668, 2, seed=2, pad=pad)
    out, named, ref, grads, eng = engine_step_and_oracle(mc, 668, 2, batch, "encoding", "bf16", 3)
    assert eng._fused_mask(16 * 200) == 15
    if on:
        kinds = {s["key"]: s["kind"] for s in eng.dropout_sites(16, 100)}
        assert len(kinds) == 4 + 2 * 3 + 2 * 5                         # 4 embdrop; p, o, mlpdrop per encoder layer; 2 x (p, o) + mlpdrop per decoder layer
        assert all(v == "rowdrop" for k, v in kinds.items() if k.endswith("/mlpdrop"))
        descs = DR.attn_site_descs(eng, 16, 100)
        assert all(s["keepbits"] is not None and descs[s["site"]][0].dh == 32 and DR.on_keepbit_kernels(*descs[s["site"]])
                   for s in eng.dropout_sites(16, 100) if s["kind"] == "attn")
    check_bf16(bf16_stats(out, named, ref, grads), f"bf16 fused, dropout {dropout}")


@pytest.mark.parametrize("dropout", ["off", "on"])
def test_bf16_dh64_dropout_step_vs_oracle_fed_the_steps_masks(dropout):
    """bf16 at dh = 64 (hidden 512, 8 heads, n_enc = n_dec = 1, B = 4, T = 100, CAUSAL + SEP on the decoder): every attention site runs
    the keep-bit pair of csrc/attention_long.hip (forward epilogue and the prep kernel's dropout'(d_o) / delta), the MLP and the
    tokenisers the un-fused kernels with the flat hash.  Same bounds as the fused test; `off` is the dropout-0 reference run.
    Measured on the MI355X (worst over tensors):
      dropout off: loss error 1.1e-4, cosine 0.999958 (>= 256 elements) / 0.999949 (< 256), norm error 6.3e-3
      dropout on : loss error 1.0e-4, cosine 0.999957 / 0.999959, norm error 5.1e-3."""
    on = dropout == "on"
    kw = dict(H=512, heads=8, n_enc=1, n_dec=1, causal=True, sep=True)
    mc = model_config(**kw) if on else model_config(dropout=0.0, emb_dropout=0.0, **kw)
    batch = O.synth_batch(4, 100, 96, 2, seed=6, pad=[0, 10, 0, 37])
    out, named, ref, grads, eng = engine_step_and_oracle(mc, 96, 2, batch, "encoding", "bf16", 3)
    if on:
        sites = eng.dropout_sites(4, 100)
        assert len(sites) == 4 + 3 + 5 and all(s["kind"] == "flat" for s in sites if not s["key"].endswith("/p"))
        descs = DR.attn_site_descs(eng, 4, 100)
        assert all(s["dh"] == 64 and s["keepbits"] is not None and DR.on_keepbit_kernels(*descs[s["site"]]) for s in sites if s["kind"] == "attn")
    check_bf16(bf16_stats(out, named, ref, grads), f"bf16 dh 64, dropout {dropout}")
