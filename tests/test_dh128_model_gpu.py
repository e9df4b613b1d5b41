"""Head dim 128 through whole models: hidden 256 / 2 heads against the reference's own forward / backward and 50-step curve
(tests/golden/dh128_*, scripts/make_dh128_goldens.py), one bf16 training step with dropout on against the fp64 oracle fed the masks
read off the kernels, and one step at hidden 1024 / 8 heads in fp32 and bf16.

The oracle (oracle/mm_oracle.py) takes any hidden_size / n_heads and every decoder mask, so no case here had to be moved to the
reference fixture for want of an oracle; the fixture covers what only the reference can say: its initial parameters and its AdamW curve."""
import numpy as np
import pytest
import torch

import dropout_refs as DR
from conftest import load_json, load_npz
from helpers import build_model, model_config
from model_checks import bf16_stats, check_bf16, check_fixture_outputs, engine_step_and_oracle, run_curve, to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("dh128_fwd_bwd.npz")
    return _Z


def sample(a, n):
    """scripts/make_dh128_goldens.py: the whole tensor up to n elements, else n elements at stride numel // n."""
    f = np.ascontiguousarray(a).reshape(-1)
    return f if f.size <= n else f[::f.size // n][:n]


def dh128_config(meta, **kw):
    return model_config(H=meta["H"], heads=meta["heads"], inter=meta["inter"], n_enc=meta["n_enc"], n_dec=meta["n_dec"], max_F=meta["max_F"],
                        dropout=0.0, emb_dropout=0.0, **kw)


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("case", ["dense", "causal", "causal_sep"])
def test_fp32_forward_backward_vs_reference_fixture(case):
    """Loss, counts (exact), token masks (exact), per-modality loss, predictions, the norm of every gradient and the stored elements of
    every gradient tensor at the tolerances of test_linear_bias_model_gpu.py::test_tiny_forward_backward_vs_reference_fixture.  The
    fixture stores gradients of more than 1024 elements as 1024 elements at a fixed stride (file size); the atol's scale is the stored
    elements' maximum, never more than the tensor's.
    The stored fp64 sum of each gradient looks at the elements the stride skips.  Its bound follows from the elementwise one: an element
    may be off by e = atol + rtol |ref|, whose root mean square over a tensor of n elements and norm g is at most atol + rtol g / sqrt(n);
    the rounding errors of two fp32 computations are not aligned, so the sum of n of them stays within 5 sqrt(n) times that,
    5 (sqrt(n) atol + rtol g)."""
    z, meta = fixture()
    sw = meta["cases"][case]
    model = build_model(dh128_config(meta, causal=sw["causal"], sep=sw["sep"]), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == meta["state"]
    for k, v in model.state_dict().items():                          # the seed gives the reference's initial parameters
        np.testing.assert_array_equal(sample(v.numpy(), meta["sample"]), z[f"init/{k}"], err_msg=k)
        assert float(v.double().sum()) == pytest.approx(float(z[f"init_stat/{k}"][0]), rel=1e-9, abs=1e-9), k
    check_fixture_outputs(model, z, case, meta["objective"], seed=meta["mask_seed"])
    eng = model._engine
    assert eng.cfg.hidden // eng.cfg.heads == 128
    named = dict(model.named_parameters())
    assert list(named) == meta["params"]
    for k in meta["params"]:
        g = named[k].grad
        gn = float(z[f"{case}/grad_stat/{k}"][1])
        assert float(g.double().norm()) == pytest.approx(gn, rel=5e-3, abs=1e-8), k
        ref = z[f"{case}/grad/{k}"]
        atol = 3e-6 + 1e-4 * np.abs(ref).max()
        gs = float(z[f"{case}/grad_stat/{k}"][0])
        assert abs(float(g.double().sum()) - gs) <= 5 * (np.sqrt(g.numel()) * atol + 2e-3 * gn), (k, float(g.double().sum()), gs)
        np.testing.assert_allclose(sample(g.cpu().numpy(), meta["sample"]), ref, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(ref).max(), err_msg=k)


def test_fp32_loss_curve_50_steps_vs_reference_fixture():
    """50 AdamW steps, mixed objectives: every loss within 1e-4 of the reference's, as every other curve here.  The final parameter
    norms are a coarse check that the optimiser reached every tensor: 1e-2, two orders above the losses' bound (a norm is dominated by
    the initial values; key.bias, whose true gradient is zero and whose Adam step therefore follows rounding noise, is skipped)."""
    g = load_json("dh128_curve.json")
    mc = model_config(H=g["H"], heads=g["heads"], inter=g["inter"], n_enc=g["n_enc"], n_dec=g["n_dec"], max_F=g["max_F"], dropout=0.0,
                      emb_dropout=0.0)
    model = build_model(mc, g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    assert len(model.state_dict()) == g["n_state_keys"]
    losses = run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)
    worst = 0.0
    for k, v in model.state_dict().items():
        if k.endswith("key.bias"):
            continue
        ref = g["final_norm"][k]
        worst = max(worst, abs(float(v.double().norm()) - ref) / (ref + 1e-12))
        assert float(v.double().norm()) == pytest.approx(ref, rel=1e-2, abs=1e-6), k
    print("worst final-norm gap", worst)


# ---------------------------------------------------------------------------------------------- bf16, dropout on
@pytest.mark.parametrize("T", [70, 72])
def test_bf16_dh128_dropout_step_vs_oracle_fed_the_steps_masks(T):
    """bf16 default path, hidden 256 / 2 heads, one layer a side, B = 4, dropout 0.4 / 0.2, CAUSAL + SEP on the decoder, two padded
    trials, against the fp64 oracle fed the step's own masks, with the criteria of test_dropout_step_gpu.py (loss 2e-2, cosine 0.995 /
    0.98, norm 5e-2).  Every attention site reports a keep-bit workspace.
      T = 70: L = 140 crosses a 128-row chunk; 140 is no multiple of 8, so the launches hand the workspace back and run the general
              tiled kernels of csrc/attention_bf16.hip with hash dropout (the read-out of tests/dropout_refs.py follows that rule).
      T = 72: L = 144, the keep-bit kernels of csrc/attention_long.hip; the masks are the bits of the engine's workspaces.
    Which of the two a site's launches run is the library's own answer for the plan's descriptor (ops.attn_family), here and in the
    read-out of tests/dropout_refs.py, and is compared with the table above."""
    mc = model_config(H=256, heads=2, inter=512, n_enc=1, n_dec=1, max_F=T, causal=True, sep=True)
    batch = O.synth_batch(4, T, 12, 2, seed=6, pad=[0, 10, 0, 37])
    out, named, ref, grads, eng = engine_step_and_oracle(mc, 12, 2, batch, "encoding", "bf16", 3)
    sites = eng.dropout_sites(4, T)
    attn = [s for s in sites if s["kind"] == "attn"]
    assert len(attn) == 3 and all(s["dh"] == 128 and s["keepbits"] is not None and s["shape"] == (4, 2, 2 * T, 2 * T) for s in attn)
    nbits = 4 * 2 * ((2 * T + 31) // 32) ** 2 * 128
    wrote = [bool(s["keepbits"][:nbits].any()) for s in attn]
    # (the engine does not clear its workspaces: where the launches hash, L = 140, their bytes say nothing)
    descs = DR.attn_site_descs(eng, 4, T)
    on_keepbit = [DR.on_keepbit_kernels(*descs[s["site"]]) for s in attn]
    assert on_keepbit == [T == 72] * 3, "L = 144 runs the keep-bit kernels, L = 140 the general ones"
    assert all(wrote) or not any(on_keepbit), "the keep-bit kernels fill every site's bit tiles"
    check_bf16(bf16_stats(out, named, ref, grads), f"bf16 dh 128, T {T}, dropout on")


# ---------------------------------------------------------------------------------------------- hidden 1024
def test_width_1024_step_fp32_vs_oracle_and_bf16():
    """hidden 1024 / 8 heads / inter 2048, one layer a side, B = 2, T = 8, 12 + 2 channels, dropout 0: the widest norm (H <= 1024), the
    GEMMs and the edges beside the dh-128 attention.  fp32 against the fp64 oracle at the fp32 bounds of the model tests; the bf16 loss is
    finite and within the bf16 step bound (2e-2) of the fp32 one."""
    mc = model_config(H=1024, heads=8, inter=2048, n_enc=1, n_dec=1, max_F=8, dropout=0.0, emb_dropout=0.0)
    batch = O.synth_batch(2, 8, 12, 2, seed=4, pad=[0, 2])
    out, named, ref, grads, eng = engine_step_and_oracle(mc, 12, 2, batch, "token_masking", "fp32", 0)
    assert eng.cfg.hidden == 1024 and eng.cfg.hidden // eng.cfg.heads == 128
    l32 = out.loss.item()
    assert l32 == pytest.approx(ref["loss"].item(), rel=2e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(ref["mod_n_examples"][m])
        assert out.mod_loss[m].item() == pytest.approx(ref["mod_loss"][m].item(), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), ref["mod_preds"][m].detach().cpu().numpy(), rtol=1e-4, atol=2e-5)
    for k, g in named.items():
        r = grads[k].cpu().numpy()
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(r).max(), err_msg=k)
    del out, named, ref, grads, eng
    torch.cuda.empty_cache()
    model = build_model(mc, 12, 2, seed=0)
    model.compute_dtype = "bf16"
    model.cuda().train()
    torch.manual_seed(5)
    o16 = model(to_dev(O.make_mod_dict(batch, "token_masking")))
    o16.loss.backward()
    l16 = o16.loss.item()
    print("fp32", l32, "bf16", l16, "relative gap", abs(l16 - l32) / abs(l32))
    assert np.isfinite(l16) and abs(l16 - l32) / abs(l32) < 2e-2
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
