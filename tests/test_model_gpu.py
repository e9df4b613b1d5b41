"""Whole-path parity on the MI355X: the API mirror (MultiModal -> HIP engine) against
 (1) fixtures produced by importing the reference (tests/golden/*), and
 (2) the CPU oracle on the same seeded inputs,
in fp32 parity mode.  Tolerances are stated per check; mask/index outputs are compared exactly."""
import math
import random

import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
from helpers import build_model, build_model_mods, load_config, make_optimizer, model_config, tiny_config
from model_checks import check_fixture_outputs, check_stored_grads, cosine, fixture_batch, resume_roundtrip, run_curve, to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

VARIANT_KW = {"base": {}, "pad": {}, "sep": dict(sep=True), "causal": dict(causal=True), "deep": dict(n_enc=2, n_dec=2)}


@pytest.mark.parametrize("variant", list(VARIANT_KW))
@pytest.mark.parametrize("objective", ["encoding", "decoding", "token_masking"])
def test_tiny_forward_backward_vs_reference_fixture(variant, objective):
    z, meta = load_npz("tiny_fwd_bwd.npz")
    model = build_model(tiny_config(**VARIANT_KW[variant]), meta["n_ap"], meta["n_beh"], seed=0)
    pre = f"{variant}/sd/"
    sd = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    model.load_state_dict(sd)
    p = f"{variant}/{objective}"
    check_fixture_outputs(model, z, p, objective, prefix=f"{variant}/batch/")
    B, T = z[f"{variant}/batch/spikes_data"].shape[:2]
    np.testing.assert_allclose(model._engine.b["enc_out"].view(B, 2 * T, -1).cpu().numpy(), z[f"{p}/enc_out"], rtol=1e-4, atol=2e-5)
    named = dict(model.named_parameters())
    assert check_stored_grads(named, z, p, list(named)) == list(named)           # the fixture keeps every gradient tensor


_MM_CASES = list(range(10))


@pytest.mark.parametrize("cid", _MM_CASES)
def test_masker_modes_through_engine_vs_reference_fixture(cid):
    """SURVEY.md §8 row f4 on the DEVICE path: every masker mode (models/masker.py:95-167) set on `model.masker` after construction
    (utils/eval_utils.py:63-67), eval_mask = None, through MultiModal.forward -> HIP engine -> backward, against
    oracle/make_goldens.py:fx_masker_modes_model (the reference's own forward/backward).  Masks and n exact, loss / predictions /
    gradient norms at fp32-parity tolerances, the generator and `random` streams consumed alike; a mode upstream cannot run on a
    two-modality batch must raise the same exception type here."""
    z, meta = load_npz("masker_modes_model.npz")
    c = meta["cases"][cid]
    model = build_model(tiny_config(max_F=meta["T"]), meta["n_ap"], meta["n_beh"], seed=0)
    model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")})
    for k, v in c["set"].items():
        setattr(model.masker, k, v)
    model.cuda().train()
    batch = fixture_batch(z)
    torch.manual_seed(31 + cid)
    random.seed(41 + cid)
    md = O.make_mod_dict(batch, "token_masking")
    md["ap"]["inputs_regions"] = np.asarray([meta["regions"]] * meta["B"])
    md = to_dev(md)
    if c["raises"]:
        with pytest.raises(Exception) as ei:
            model(md)
        assert type(ei.value).__name__ == c["raises"], f"upstream raises {c['raises']}, this path {type(ei.value).__name__}"
        return
    out = model(md)
    out.loss.backward()
    assert out.loss.item() == pytest.approx(c["loss"], rel=2e-5, nan_ok=True)      # nothing masked (channel 0 of co-smooth): 0/0 = NaN upstream too
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == c["n"][m]
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"c{cid}/mask/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(c["mod_loss"][m], rel=5e-5, abs=1e-6, nan_ok=True)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"c{cid}/preds/{m}"], rtol=1e-4, atol=2e-5)
    for k, prm in model.named_parameters():
        gn = 0.0 if prm.grad is None else float(prm.grad.double().norm())
        assert gn == pytest.approx(c["grad_norm"][k], rel=5e-3, abs=1e-8, nan_ok=True), k
    assert float(torch.rand(1)) == c["after_rand"] and random.random() == c["after_random"]        # same draws consumed


def test_default_config_scalars_vs_reference_fixture():
    g = load_json("default_scalars.json")
    model = build_model(load_config().model, 668, 2, seed=42).cuda().eval()
    batch = O.synth_batch(16, 100, 668, 2, seed=0)
    for obj in ("encoding", "decoding", "token_masking"):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        out = model(to_dev(O.make_mod_dict(batch, obj)))
        out.loss.backward()
        assert out.loss.item() == pytest.approx(g[obj]["loss"], rel=1e-5)
        for m in ("ap", "behavior"):
            assert int(out.mod_n_examples[m]) == g[obj]["n"][m]
            assert float(out.mod_preds[m].double().abs().sum()) == pytest.approx(g[obj]["pred_abssum"][m], rel=1e-4)
        for k, prm in model.named_parameters():
            assert float(prm.grad.double().norm()) == pytest.approx(g[obj]["grad_norm"][k], rel=5e-3, abs=1e-8), k


def test_config5_three_modalities_vs_reference_fixture():
    """BASELINE configs[4] as SURVEY.md §8d instantiates it: H=512, I=1024, dh=64, T=200, ap+behavior+lfp (L=600), 5+5
    layers; fp32 parity mode against the reference's own forward/backward (oracle/make_goldens.py:fx_config5_scalars).
    L=600 with dh=64 does not fit LDS: this runs the tiled attention kernels."""
    g = load_json("config5_scalars.json")
    mods = [tuple(m) for m in g["mods"]]
    model = build_model_mods(model_config(H=512, heads=8, inter=1024, max_F=200, n_modality=3), mods, seed=g["model_seed"])
    model.loss_mod["lfp"] = torch.nn.MSELoss(reduction="none")          # as upstream would add it (mm.py:79-82)
    model = model.cuda().eval()
    batch = O.synth_batch_mods(g["B"], g["T"], mods, seed=g["batch_seed"], pad=g["pad"])
    for case, masked in (("token_masking", None), ("mask_ap", "ap"), ("mask_lfp", "lfp")):
        c = g["cases"][case]
        model.zero_grad(set_to_none=True)
        torch.manual_seed(g["masker_seed"])
        out = model(to_dev(O.make_mod_dict_mods(batch, mods, masked)))
        out.loss.backward()
        assert out.loss.item() == pytest.approx(c["loss"], rel=1e-5)
        for m, _ in mods:
            assert int(out.mod_n_examples[m]) == c["n"][m]
            assert float(out.mod_preds[m].double().abs().sum()) == pytest.approx(c["pred_abssum"][m], rel=1e-4)
        for k, prm in model.named_parameters():
            gn = 0.0 if prm.grad is None else float(prm.grad.double().norm())
            assert gn == pytest.approx(c["grad_norm"][k], rel=5e-3, abs=1e-8), k
    for m, _ in mods:
        np.testing.assert_allclose(out.mod_preds[m][1, 150:153, 0].cpu().numpy(), g["pred_samples"][m], rtol=1e-3, atol=1e-5)


def test_config5_bf16_train_steps_finite_and_close():
    """Same shapes in bf16 throughput mode with dropout on: three optimisation steps run (tiled attention on bf16
    storage), the loss is finite and stays within bf16 distance of the fp32 reference value at step 0."""
    g = load_json("config5_scalars.json")
    mods = [tuple(m) for m in g["mods"]]
    model = build_model_mods(model_config(H=512, heads=8, inter=1024, max_F=200, n_modality=3, dropout=0.0, emb_dropout=0.0), mods,
                             seed=g["model_seed"])
    model.loss_mod["lfp"] = "mse"
    model.compute_dtype = "bf16"
    model = model.cuda().train()
    opt, sch = make_optimizer(model, 10)
    batch = O.synth_batch_mods(g["B"], g["T"], mods, seed=g["batch_seed"], pad=g["pad"])
    losses = []
    for s in range(3):
        torch.manual_seed(g["masker_seed"])
        out = model(to_dev(O.make_mod_dict_mods(batch, mods, "ap")))
        out.loss.backward()
        opt.step(); sch.step(); opt.zero_grad()
        losses.append(out.loss.item())
    assert np.isfinite(losses).all()
    assert losses[0] == pytest.approx(g["cases"]["mask_ap"]["loss"], rel=2e-2)
    assert losses[2] < losses[0]


def test_config5_bf16_drift_against_fp32_engine_and_dropout_run():
    """BASELINE configs[4] shapes (dh = 64, L = 600: csrc/attention_long.hip and the 256-tile GEMM) over TWELVE optimiser steps: the bf16
    engine against this library's own fp32 parity engine on the same batches and masks (the fp32 engine is pinned to the reference by
    test_config5_three_modalities_vs_reference_fixture) - every step within 2e-2, the mean relative gap within 8e-3.  Then the same
    model with dropout 0.4 / 0.2: the keep-bit attention pair runs in training (one bit workspace per attention site), losses stay
    finite and the first one sits where dropout puts it (within 30 % of the dropout-free value)."""
    g = load_json("config5_scalars.json")
    mods = [tuple(m) for m in g["mods"]]

    def make(dtype, dropout, emb_dropout):
        m = build_model_mods(model_config(H=512, heads=8, inter=1024, max_F=200, n_modality=3, dropout=dropout, emb_dropout=emb_dropout), mods,
                             seed=g["model_seed"])
        m.loss_mod["lfp"] = "mse"
        m.compute_dtype = dtype
        return m.cuda().train()

    def run(model, steps):
        opt, sch = make_optimizer(model, 20)
        out_l = []
        for s_ in range(steps):
            batch = O.synth_batch_mods(g["B"], g["T"], mods, seed=g["batch_seed"] + s_, pad=g["pad"])
            torch.manual_seed(g["masker_seed"] + s_)
            out = model(to_dev(O.make_mod_dict_mods(batch, mods, ("ap", "lfp", None)[s_ % 3])))
            out.loss.backward()
            opt.step(); sch.step(); opt.zero_grad()
            out_l.append(out.loss.item())
        return np.array(out_l)

    l32 = run(make("fp32", 0.0, 0.0), 12)
    mb = make("bf16", 0.0, 0.0)
    l16 = run(mb, 12)
    assert np.isfinite(l32).all() and np.isfinite(l16).all()
    rel = np.abs(l16 - l32) / np.abs(l32)
    assert rel.max() < 2e-2, (l16, l32)
    assert rel.mean() < 8e-3, rel
    del mb
    md = make("bf16", 0.4, 0.2)
    ld = run(md, 6)
    assert np.isfinite(ld).all()
    assert ld[0] == pytest.approx(l16[0], rel=0.3)
    assert any(k.endswith("/keep") for k in md._engine.b), "the keep-bit attention workspaces were not allocated: dropout ran on the hash path"


def test_loss_curve_tiny_50_steps_vs_reference_fixture():
    g = load_json("loss_curve.json")["tiny"]
    model = build_model(tiny_config(), 12, 2, seed=7).cuda()
    losses = run_curve(model, 50, 2, 8, 12, 2, 50, g["objective"])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)          # north star: curve within 1e-4


def test_loss_curve_tiny_1000_steps_vs_reference_fixture():
    """North star: 'masked-loss curve matching reference to 1e-4 over 1k synthetic steps' (reference CPU fp32 run,
    oracle/make_goldens.py:fx_loss_curve_1k; mixed objectives, OneCycleLR over the 1000 steps, dropout 0)."""
    g = load_json("loss_curve_1k.json")
    model = build_model(tiny_config(), 12, 2, seed=7).cuda()
    losses = run_curve(model, 1000, 2, 8, 12, 2, 1000, g["objective"])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


def test_loss_curve_default_30_steps_vs_reference_fixture():
    g = load_json("loss_curve.json")["default"]
    model = build_model(model_config(dropout=0.0, emb_dropout=0.0), 668, 2, seed=42).cuda()
    losses = run_curve(model, 30, 16, 100, 668, 2, 1000, g["objective"])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


def test_h64_two_layer_config_vs_reference_fixture():
    """BASELINE.json configs[0] as worded: 2+2 layers, d_model 64, 8 heads, inter 128 (fx_h64_curve): per-objective loss, exact n,
    every gradient norm, and the 100-step curve in fp32 parity mode."""
    g = load_json("h64_curve.json")
    mc = model_config(H=64, heads=8, inter=128, n_enc=2, n_dec=2, max_F=100, dropout=0.0, emb_dropout=0.0)
    model = build_model(mc, 668, 2, seed=g["model_seed"]).cuda().eval()
    batch = O.synth_batch(16, 100, 668, 2, seed=0)
    for obj in ("encoding", "decoding", "token_masking"):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        out = model(to_dev(O.make_mod_dict(batch, obj)))
        out.loss.backward()
        s = g["scalars"][obj]
        assert out.loss.item() == pytest.approx(s["loss"], rel=1e-5)
        for m in ("ap", "behavior"):
            assert int(out.mod_n_examples[m]) == s["n"][m]
            assert float(out.mod_preds[m].double().abs().sum()) == pytest.approx(s["pred_abssum"][m], rel=1e-4)
        for k, prm in model.named_parameters():
            assert float(prm.grad.double().norm()) == pytest.approx(s["grad_norm"][k], rel=5e-3, abs=1e-8), k
    model = build_model(mc, 668, 2, seed=g["model_seed"]).cuda()
    losses = run_curve(model, 100, 16, 100, 668, 2, 100, g["objective"])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


def test_loss_curve_default_1000_steps_fp32_vs_reference_fixture():
    """North star at the metric's own config: d_model 256, 5+5 layers, T=100, 668+2 channels, B=16, dropout 0, mixed objectives,
    OneCycleLR over the run - all 1000 steps of the reference's CPU curve (fx_loss_curve_1k_default) within rtol 1e-4 in fp32
    parity mode."""
    g = load_json("loss_curve_1k_default.json")
    model = build_model(model_config(dropout=0.0, emb_dropout=0.0), 668, 2, seed=42).cuda()
    losses = run_curve(model, 1000, 16, 100, 668, 2, 1000, g["objective"])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


@pytest.mark.parametrize("fused", ["0", "15"])
def test_loss_curve_default_1000_steps_bf16_drift_bound(monkeypatch, fused):
    """The same 1000 steps in bf16 throughput mode, with the un-fused kernels and with the benched set of row-owner fused kernels
    (MMFM_FUSED=15, every group; the explicit setting also lifts the small-batch guard).  Stated and tested bound against the fp32 reference
    curve: every step within 2e-2 relative, every 50-step window mean within 5e-3 relative."""
    monkeypatch.setenv("MMFM_FUSED", fused)
    g = load_json("loss_curve_1k_default.json")
    model = build_model(model_config(dropout=0.0, emb_dropout=0.0), 668, 2, seed=42)
    model.compute_dtype = "bf16"
    model.cuda()
    losses = np.asarray(run_curve(model, 1000, 16, 100, 668, 2, 1000, g["objective"]))
    ref = np.asarray(g["loss"])
    assert np.isfinite(losses).all()
    rel = np.abs(losses - ref) / np.abs(ref)
    assert rel.max() < 2e-2, f"worst step {int(rel.argmax())}: {losses[rel.argmax()]} vs {ref[rel.argmax()]}"
    win = np.abs(losses.reshape(20, 50).mean(1) - ref.reshape(20, 50).mean(1)) / ref.reshape(20, 50).mean(1)
    assert win.max() < 5e-3, f"window {int(win.argmax())}: {win.max()}"


def test_adamw_trajectory_vs_reference_fixture():
    z, _ = load_npz("sched_adamw.npz")
    model = build_model(tiny_config(), 12, 2, seed=7).cuda()
    losses = run_curve(model, 5, 2, 8, 12, 2, 20, ["encoding"] * 5)
    for s in range(5):
        assert losses[s] == pytest.approx(float(z[f"traj/loss{s}"]), rel=5e-5)
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), z[f"traj/final/{k}"], rtol=2e-4, atol=3e-6, err_msg=k)


def test_trainer_epoch_vs_reference_fixture():
    from trainer.make import make_multimodal_trainer
    from multi_modal_foundation_model_amd.ddp import Accelerator
    g = load_json("trainer_io.json")
    B, T, n_ap, n_beh = g["B"], g["T"], g["n_ap"], g["n_beh"]
    model = build_model(tiny_config(), n_ap, n_beh, seed=7)
    acc = Accelerator()
    model = acc.prepare(model)
    opt, sch = make_optimizer(model, 100)

    def loader(seed0):
        out = []
        for i in range(3):
            b = O.synth_batch(B, T, n_ap, n_beh, seed=seed0 + i)
            b["eid"] = ["synthetic"] * B
            b["neuron_regions"] = [["XX"] * B for _ in range(n_ap)]
            out.append(b)
        return out
    cfg = load_config()
    cfg["training"]["exact_masker_stream"] = True       # the fixture holds the reference's generator stream (trainer default: token masks only)
    tr = make_multimodal_trainer(model=model, train_dataloader=loader(0), eval_dataloader=loader(50), optimizer=opt, log_dir="/tmp",
                                 accelerator=acc, lr_scheduler=sch, avail_mod=["ap", "behavior"], config=cfg,
                                 modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=True,
                                 num_neurons=[n_ap])
    random.seed(42)
    torch.manual_seed(99)
    res = tr.train_epoch(0)
    ev = tr.eval_epoch()
    assert res["train_loss"] == pytest.approx(g["train_loss"], rel=5e-5)
    assert ev["eval_loss"] == pytest.approx(g["eval_loss"], rel=1e-4)
    assert sorted(ev.keys()) == g["eval_keys"]
    for m in ("ap", "behavior"):
        assert list(ev["eval_gt"][0][m].shape) == g["eval_gt_shapes"][m]
        assert list(ev["eval_preds"][0][m].shape) == g["eval_preds_shapes"][m]
        assert float(ev["eval_preds"][0][m].double().abs().sum()) == pytest.approx(g["eval_preds_abssum"][m], rel=1e-3)
    assert float(ev["eval_trial_avg_r2"]) == pytest.approx(g["eval_trial_avg_r2"], rel=5e-3, abs=5e-3)


def test_padded_default_shapes_vs_oracle():
    """B=5 with ragged padding, default widths: the HIP path against the CPU oracle on the same inputs."""
    mc = model_config(n_enc=2, n_dec=2, dropout=0.0, emb_dropout=0.0)
    model = build_model(mc, 668, 2, seed=3)
    cfg = O.OracleCfg.from_model_config(mc, {"ap": 668, "behavior": 2})
    sd = O.share_mod_emb({k: v.detach().clone() for k, v in model.state_dict().items()}, cfg)
    keys = O.trainable_keys(sd, cfg)
    for k in keys:
        sd[k].requires_grad_(True)
    batch = O.synth_batch(5, 100, 668, 2, seed=9, pad=[0, 10, 0, 37, 1])
    mk = O.OracleMasker(dict(load_config().model.masker))
    torch.manual_seed(5)
    ref = O.forward(sd, O.make_mod_dict(batch, "token_masking"), cfg, training=True, masker=mk)
    grads = torch.autograd.grad(ref["loss"], [sd[k] for k in keys])
    model.cuda().train()
    torch.manual_seed(5)
    out = model(to_dev(O.make_mod_dict(batch, "token_masking")))
    out.loss.backward()
    assert out.loss.item() == pytest.approx(ref["loss"].item(), rel=1e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(ref["mod_n_examples"][m])
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), ref["mod_preds"][m].detach().numpy(), rtol=1e-4, atol=3e-5)
    named = dict(model.named_parameters())
    for k, gr in zip(keys, grads):
        ref_g = gr.numpy()
        np.testing.assert_allclose(named[k].grad.cpu().numpy(), ref_g, rtol=2e-3, atol=1e-7 + 1e-4 * np.abs(ref_g).max(), err_msg=k)


def test_nothing_masked_gives_nan_like_reference():
    model = build_model(tiny_config(), 12, 2, seed=1).cuda().eval()
    md = to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=0), "encoding"))
    md["ap"]["eval_mask"] = torch.zeros_like(md["ap"]["eval_mask"])
    with torch.no_grad():
        out = model(md)
    assert math.isnan(out.loss.item()) and int(out.mod_n_examples["ap"]) == 0


def test_input_mask_path_fails_like_upstream():
    model = build_model(tiny_config(), 12, 2, seed=1).cuda()
    md = to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=0), "encoding"))
    md["ap"]["masking_mode"] = "temporal"
    with pytest.raises(UnboundLocalError):
        model(md)


def test_training_mode_dropout_is_deterministic_and_finite():
    mc = model_config(n_enc=1, n_dec=1)          # dropout 0.4 / 0.2 as configured
    batch = O.synth_batch(4, 100, 668, 2, seed=2)
    losses, gnorms = [], []
    for rep in range(2):
        model = build_model(mc, 668, 2, seed=3).cuda().train()
        model.engine_seed = 77
        out = model(to_dev(O.make_mod_dict(batch, "encoding")))
        out.loss.backward()
        losses.append(out.loss.item())
        gnorms.append(model._engine.G.double().norm().item())
    assert math.isfinite(losses[0]) and losses[0] == losses[1] and gnorms[0] == gnorms[1]
    model.eval()
    with torch.no_grad():
        l_eval = model(to_dev(O.make_mod_dict(batch, "encoding"))).loss.item()
    assert l_eval != losses[0]
    # a second training forward draws new masks (rng_advance)
    model.train()
    l2 = model(to_dev(O.make_mod_dict(batch, "encoding"))).loss.item()
    assert l2 != losses[0]


def test_grad_accumulation_semantics_without_zero_grad():
    model = build_model(tiny_config(), 12, 2, seed=7).cuda().train()
    md = lambda: to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=0), "encoding"))
    model(md()).loss.backward()
    g1 = model._engine.G.clone()
    model(md()).loss.backward()                    # no zero_grad(): torch semantics are +=
    torch.testing.assert_close(model._engine.G, 2 * g1, rtol=1e-6, atol=1e-9)
    model.zero_grad(set_to_none=True)
    model(md()).loss.backward()
    torch.testing.assert_close(model._engine.G, g1, rtol=0, atol=0)     # bitwise reproducible


def test_checkpoint_pickle_roundtrip(tmp_path):
    model = build_model(tiny_config(), 12, 2, seed=7).cuda().eval()
    md = lambda: to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=0), "encoding"))
    with torch.no_grad():
        l0 = model(md()).loss.item()
    path = tmp_path / "model_last.pt"
    torch.save({"model": model, "epoch": 3}, path)             # trainer/base.py:302-308
    ck = torch.load(path, weights_only=False)                   # our own file
    m2 = ck["model"].cuda().eval()
    m2.masker.ratio = 0.1                                       # eval_utils.py:65-67 mutates these
    with torch.no_grad():
        assert m2(md()).loss.item() == l0


# ------------------------------------------------------------------------------------ bf16 throughput mode
def test_bf16_mode_tracks_fp32_reference_fixture():
    """bf16 storage / fp32 accumulate vs the fp32 reference numbers: stated tolerance 2e-2 on the loss,
    gradient direction cosine >= 0.99 per large tensor (bf16 has 8 significant bits)."""
    g = load_json("default_scalars.json")
    model = build_model(load_config().model, 668, 2, seed=42)
    model.compute_dtype = "bf16"
    model.cuda().eval()
    ref = build_model(load_config().model, 668, 2, seed=42).cuda().eval()
    batch = O.synth_batch(16, 100, 668, 2, seed=0)
    for obj in ("encoding", "decoding"):
        for m in (model, ref):
            m.zero_grad(set_to_none=True)
        out = model(to_dev(O.make_mod_dict(batch, obj)))
        out.loss.backward()
        out32 = ref(to_dev(O.make_mod_dict(batch, obj)))
        out32.loss.backward()
        assert out.loss.item() == pytest.approx(g[obj]["loss"], rel=2e-2)
        for mname in ("ap", "behavior"):
            assert int(out.mod_n_examples[mname]) == g[obj]["n"][mname]
        p16, p32 = dict(model.named_parameters()), dict(ref.named_parameters())
        for k in p32:
            if p32[k].grad.abs().max() > 0 and p32[k].numel() >= 4096:
                c = cosine(p16[k].grad, p32[k].grad)
                assert c > 0.99, f"{obj} {k}: cosine {c}"


def test_bf16_loss_curve_stays_near_fp32():
    g = load_json("loss_curve.json")["default"]
    model = build_model(model_config(dropout=0.0, emb_dropout=0.0), 668, 2, seed=42)
    model.compute_dtype = "bf16"
    model.cuda()
    losses = run_curve(model, 12, 16, 100, 668, 2, 1000, g["objective"])
    np.testing.assert_allclose(losses, g["loss"][:12], rtol=2e-2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_alternating_batch_shapes_keep_their_plans(dtype):
    """A ragged last batch (the reference DataLoader has no drop_last) changes (B, T) and comes back: every cached plan
    and captured hipGraph must keep pointing at live buffers.  B = 6 -> 3 -> 6 -> 3 in train and eval, against an
    engine that only ever saw one shape."""
    mc = tiny_config(n_enc=2, n_dec=2)

    def fresh():
        m = build_model(mc, 12, 2, seed=7)
        m.compute_dtype = dtype
        return m.cuda()

    def step(model, B, seed, train):
        model.train(train)
        md = to_dev(O.make_mod_dict(O.synth_batch(B, 8, 12, 2, seed=seed), "encoding"))
        if not train:
            with torch.no_grad():
                return model(md).loss.item(), None
        model.zero_grad(set_to_none=True)
        out = model(md)
        out.loss.backward()
        return out.loss.item(), model._engine.G.clone()

    seq = [(6, 0, True), (6, 1, True), (6, 2, True), (3, 3, True), (6, 4, True), (3, 5, False), (6, 6, False), (6, 7, True),
           (3, 8, True), (3, 9, True), (3, 10, True), (6, 11, True)]
    mixed = fresh()
    got = [step(mixed, *a) for a in seq]
    for (B, seed, train), (loss, G) in zip(seq, got):
        ref = fresh()
        for _ in range(3):                       # run the single-shape engine past its graph capture as well
            l_ref, G_ref = step(ref, B, seed, train)
        assert loss == l_ref, (B, seed, train)
        if G is not None:
            torch.testing.assert_close(G, G_ref, rtol=0, atol=0)
    assert len(mixed._engine._pools) == 2


def test_shape_pool_eviction_drops_plans(monkeypatch):
    monkeypatch.setenv("MMFM_MAX_SHAPES", "2")
    model = build_model(tiny_config(), 12, 2, seed=7).cuda().eval()
    losses = {}
    with torch.no_grad():
        for B in (2, 3, 4, 2, 3, 4):
            l = model(to_dev(O.make_mod_dict(O.synth_batch(B, 8, 12, 2, seed=B), "encoding"))).loss.item()
            assert losses.setdefault(B, l) == l
    eng = model._engine
    assert len(eng._pools) == 2 and all((k[0], k[1]) in eng._pools for k in eng.plans)


@pytest.mark.parametrize("B", [16, 1024])
def test_bf16_fused_row_owner_path_matches_unfused_kernels(monkeypatch, B):
    """bf16 mode, default widths: the row-owner fused kernels (LN folded into the linears, one-launch MLP with recompute,
    LN backward in the dX epilogues, LN / linear gradients from G = dY^T x_hat) against the un-fused round-1 kernels on the
    same inputs: same loss to bf16 accuracy, same gradient direction for every tensor, and close to the fp32 reference.
    B = 1024 is the bench's batch (R = 204,800 rows: several 128-row passes per workgroup, persistent GEMM tiles)."""
    g = load_json("default_scalars.json")
    batch = O.synth_batch(B, 100, 668, 2, seed=0)
    res = {}
    for mode in ("0", "15"):
        monkeypatch.setenv("MMFM_FUSED", mode)
        model = build_model(model_config(dropout=0.0, emb_dropout=0.0), 668, 2, seed=42)
        model.compute_dtype = "bf16"
        model.cuda().train()
        out = {}
        for obj in ("encoding", "token_masking"):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            o = model(to_dev(O.make_mod_dict(batch, obj)))
            o.loss.backward()
            out[obj] = (o.loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
        assert model._engine._fused_mask(B * 200) == int(mode)          # (the env override also lifts the small-batch guard)
        res[mode] = out
        del model
        torch.cuda.empty_cache()
    for obj in ("encoding", "token_masking"):
        l0, g0 = res["0"][obj]
        l1, g1 = res["15"][obj]
        assert l1 == pytest.approx(l0, rel=3e-3)
        if B == 16:
            assert l1 == pytest.approx(g[obj]["loss"], rel=2e-2)          # the fixture is the reference's loss on this very batch
        for k in g0:
            if g0[k].abs().max() == 0:
                assert g1[k].abs().max() == 0, k
                continue
            if k.endswith("key.bias"):           # softmax is invariant to a key bias: its true gradient is 0, both are rounding noise
                continue
            c = cosine(g0[k], g1[k])
            assert c > (0.995 if g0[k].numel() >= 256 else 0.98), f"{obj} {k}: cosine {c}"
            n0, n1 = g0[k].double().norm().item(), g1[k].double().norm().item()
            assert n1 == pytest.approx(n0, rel=5e-2), f"{obj} {k}: norm {n1} vs {n0}"


def test_bf16_fused_path_trains_with_dropout_and_partial_rows(monkeypatch):
    """Dropout as configured, B = 5 (R = 1000 rows: not a multiple of the 128 / 256-row passes) and padded trials: a few
    optimiser steps stay finite and reduce the loss; a second engine with the same seed reproduces them bit for bit."""
    monkeypatch.setenv("MMFM_FUSED", "15")           # every fused group (explicit: lifts the small-batch guard)
    mc = model_config(n_enc=2, n_dec=2)
    curves = []
    for rep in range(2):
        model = build_model(mc, 668, 2, seed=3)
        model.compute_dtype = "bf16"
        model.engine_seed = 11
        model.cuda().train()
        opt, sch = make_optimizer(model, 20, lr=5e-4)
        torch.manual_seed(5)
        losses = []
        for s in range(6):
            batch = O.synth_batch(5, 100, 668, 2, seed=s % 2, pad=[0, 10, 0, 37, 1])
            out = model(to_dev(O.make_mod_dict(batch, "encoding")))
            out.loss.backward()
            opt.step(); sch.step(); opt.zero_grad()
            losses.append(out.loss.item())
        curves.append(losses)
    assert np.isfinite(curves[0]).all() and curves[0] == curves[1]
    assert curves[0][4] < curves[0][0]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_resume_from_train_state_is_bit_identical(tmp_path, dtype):
    """6 steps in one go == 3 steps, save_model (module pickle + train state), brand-new model / optimiser /
    scheduler / trainer objects restored from the files, 3 more steps.  Dropout is on (engine RNG), objectives are sampled
    (Python RNG) and token_masking draws masks (torch RNG): all three streams must continue exactly."""
    def after_restore(m2, opt2, sch2):
        assert opt2._t == 3 and sch2.last_epoch == 3

    resume_roundtrip(tmp_path, tiny_config(n_enc=2, n_dec=2, dropout=0.4, emb_dropout=0.2), dtype=dtype, after_restore=after_restore)


def test_optimizer_step_without_backward_is_a_noop():
    """torch skips parameters whose .grad is None; the flat gradient buffer must not be applied a second time."""
    model = build_model(tiny_config(), 12, 2, seed=7).cuda().train()
    opt, sch = make_optimizer(model, 10)
    out = model(to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=0), "encoding")))
    out.loss.backward()
    opt.step(); opt.zero_grad()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt.step()                                   # no backward since zero_grad()
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    sd = opt.state_dict()
    assert sd["fused"]["t"] == 1 and sd["fused"]["m"].abs().sum() > 0
