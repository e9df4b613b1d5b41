"""modal_filter on the MI355X, whole models: encoder and decoder over different modality sets, and share_modality_embeddings=False.
The fp32 engine against the reference's own forward / backward and 50-step curves (tests/golden/modal_filter_*,
scripts/make_modal_filter_goldens.py), NaN where the reference is NaN; the bf16 engine against the fp32 engine at the default widths;
a dropout-on step; checkpoint resume and hipGraph replay of a filtered model; the size-mismatch error; the default model's plan."""
import math
import random

import numpy as np
import pytest
import torch

import dropout_refs as DR
import model_checks as MC
from conftest import load_json
from helpers import build_model, load_config, make_optimizer, model_config, tiny_config
from modal_filter import BOTH, CASES, OBJECTIVES, case_model, fixture, switches
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- fp32 against the reference
def check_filtered_case(model, z, meta, case, objective):
    """model_checks.check_fixture_case for a model whose outputs hold the decoder's modalities only: the same quantities at the same
    bounds (loss 2e-5, counts and token masks exact, modality loss 5e-5 / 1e-6, predictions 1e-4 / 2e-5, gradient norms 5e-3, stored
    gradients through check_stored_grads), over the decoder's modalities.  Where the reference masks nothing in them (meta nan): loss NaN
    and every n = 0."""
    p, dec = f"{case}/{objective}", switches(case)["output"]
    model.cuda().train()
    torch.manual_seed(11)
    md = MC.to_dev(O.make_mod_dict(MC.fixture_batch(z), objective))
    out = model(md)
    assert list(out.mod_loss) == list(out.mod_n_examples) == list(out.mod_preds) == list(out.mod_targets) == dec
    for m in BOTH:                  # written as upstream: masks for every modality, gt / preds for the decoder's
        assert md[m]["inputs_mask"] is md[m]["targets_mask"] and md[m]["encoder_attn_mask"] is md[m]["inputs_attn_mask"]
        assert ("preds" in md[m]) == ("gt" in md[m]) == (m in dec)
    print(p, "loss", out.loss.item(), "reference", float(z[f"{p}/loss"]))
    for m in dec:
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
    if p in meta["nan"]:
        assert math.isnan(out.loss.item()) and math.isnan(float(z[f"{p}/loss"])) and all(int(out.mod_n_examples[m]) == 0 for m in dec)
        return
    out.loss.backward()
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=2e-5)
    for m in BOTH:
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"{p}/mask/{m}"])
    for m in dec:
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names and list(model.state_dict()) == [k for k, _ in meta["state"][case]]
    for k, gn in zip(names, z[f"{p}/grad_norm"]):
        assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=5e-3, abs=1e-8), k
    stored = MC.check_stored_grads(named, z, p, names)
    full = objective == meta["full_grad"] and case in meta["full_grad_cases"]
    assert len(stored) == (len(names) if full else 0)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """UNSHARED has both modalities on both sides and goes through model_checks.check_fixture_case itself; the filtered cases through its
    twin above."""
    z, meta = fixture()
    model = case_model(case, meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    if case == "UNSHARED":
        MC.check_fixture_case(model, z, meta, case, objective)
        eng = model._engine
        assert not eng.cfg.share_mod_emb and eng.layout.has("decoder_embeddings.ap.embedder.mod_emb.weight")
    else:
        check_filtered_case(model, z, meta, case, objective)
        plan = model._engine._last
        split = switches(case)["input"] != switches(case)["output"]
        assert ("dec/tokmask" in plan["b"]) == split and [fn.__name__ for fn, _, _ in plan["fwd"]].count("mmfm_mask_prep") == (2 if split else 1)
        unused = [i for i, m in enumerate(BOTH) if m not in switches(case)["input"] + switches(case)["output"]]
        assert not any(f"in/{i}" in plan["b"] or f"mask/{i}" in plan["b"] for i in unused)           # a modality no side has is not staged
        assert {k for k in plan["b"] if k.startswith("tgt/")} == {f"tgt/{BOTH.index(m)}" for m in switches(case)["output"]}


@pytest.mark.parametrize("case", ["DEC", "UNSHARED"])
def test_loss_curve_tiny_50_steps_vs_reference_fixture(case):
    """The objective rotation skips nothing: DEC's first `encoding` step is NaN in the reference, AdamW carries it into every parameter and
    every later step is NaN - here as there."""
    g = load_json("modal_filter_curve.json")[case]
    model = case_model(case, g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    assert len(model.state_dict()) == g["n_state_keys"]
    losses = MC.run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    fin = [i for i, nan in enumerate(g["nan"]) if not nan]
    print("finite steps", len(fin), "max relative gap", float(np.max(np.abs(np.array([losses[i] / g["loss"][i] for i in fin]) - 1))))
    assert [math.isnan(x) for x in losses] == g["nan"]
    np.testing.assert_allclose([losses[i] for i in fin], [g["loss"][i] for i in fin], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- bf16 at the default widths
def _wide_step(case, dtype, batch, dropout=0.0, seed=3):
    """One training step of `case` at the YAML widths (hidden 256, 8 heads, inter_size 512; 2 + 2 layers, 40 + 2 channels)."""
    model = case_model(case, 40, 2, seed=seed, config=model_config, n_enc=2, n_dec=2, dropout=dropout, emb_dropout=dropout / 2)
    model.compute_dtype, model.engine_seed = dtype, 77
    model.cuda().train()
    torch.manual_seed(5)
    out = model(MC.to_dev(O.make_mod_dict(batch, "token_masking")))
    out.loss.backward()
    torch.cuda.synchronize()
    return model, out


@pytest.mark.parametrize("case", ["DEC", "UNSHARED"])
def test_bf16_step_at_default_widths_vs_fp32_engine(case):
    """The tiny H = 32 model never reaches the row-owner or the fast attention kernels.  Hidden 256 / 8 heads (dh 32) / inter_size 512,
    B = 4, T = 100, one right-padded sample, 40 + 2 channels, dropout 0: one bf16 step against the fp32 engine on the same weights and
    masks, at model_checks.check_bf16's bounds.  DEC's sequences are L = T = 100 long (one modality a side): the dh-32 fast pair runs on 4
    tiles with a 4-row tail, the row-owner linears on R = 400 rows.
    Measured on the MI355X (worst over tensors): DEC loss error 2.8e-4, cosine 0.99995 (>= 256 elements) / 0.99999 (< 256), norm error
    2.2e-3; UNSHARED 8.1e-6, 0.99996 / 0.99999, 2.9e-3."""
    batch = O.synth_batch(4, 100, 40, 2, seed=6, pad=[0, 0, 37, 0])
    m32, o32 = _wide_step(case, "fp32", batch)
    m16, o16 = _wide_step(case, "bf16", batch)
    M = len(switches(case)["input"])
    assert m16._engine._fused_mask(4 * M * 100) == 11 and m16._engine._last["R"] == 4 * M * 100
    assert [int(o16.mod_n_examples[m]) for m in o16.mod_n_examples] == [int(o32.mod_n_examples[m]) for m in o32.mod_n_examples]
    named = {k: p.grad for k, p in m16.named_parameters()}
    grads = {k: p.grad.double() for k, p in m32.named_parameters()}
    assert list(named) == list(grads)
    MC.check_bf16(MC.bf16_stats(o16, named, dict(loss=o32.loss.double()), grads), f"bf16 {case} default widths vs fp32 engine")


def test_bf16_dropout_step_is_a_function_of_the_rng_state():
    """DEC in bf16 at the tiny shape with dropout 0.4 / 0.2: the backward regenerates the forward's masks from (rng state, site, index),
    so a step is a pure function of the engine's RNG state.  Two runs from the same state give the loss and every gradient bit for bit;
    the next step on the same batch and token masks draws new masks.  The engine's site table describes the filtered model: one
    tokeniser site a side, the block sites of the 1 + 1 layers, the tokeniser sites' multipliers readable at (B T, H) (tests/dropout_refs.py)."""
    from multi_modal_foundation_model_amd import ops as K
    batch = O.synth_batch(3, 8, 12, 2, seed=4, pad=[0, 3, 1])

    def step(model):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        out = model(MC.to_dev(O.make_mod_dict(batch, "token_masking")))
        out.loss.backward()
        torch.cuda.synchronize()
        return out.loss.item(), {k: p.grad.clone() for k, p in model.named_parameters()}

    def make():
        model = case_model("DEC", dropout=0.4, emb_dropout=0.2)
        model.compute_dtype, model.engine_seed = "bf16", 77
        return model.cuda().train()

    a, b = make(), make()
    la, ga = step(a)
    lb, gb = step(b)
    assert la == lb and math.isfinite(la) and all(torch.equal(ga[k], gb[k]) for k in ga)
    eng = a._engine
    sites = eng.dropout_sites(3, 8)
    assert sorted(s["key"] for s in sites if "/embdrop/" in s["key"]) == ["decoder/embdrop/1", "encoder/embdrop/0"]
    assert len(sites) == 2 + 3 + 5 and all(s["shape"] == (3, 4, 8, 8) for s in sites if s["kind"] == "attn")
    for s in sites:
        if "/embdrop/" in s["key"]:          # (B T, H) rows of the side's one tokeniser, read back off the kernels
            assert s["shape"] == (3 * 8, 32) and s["p"] == 0.2
            assert 0 < float((DR.flat_multiplier(K, eng.rng, s["site"], s["p"], *s["shape"]) == 0).double().mean()) < 1
    state = eng.rng.clone()
    l2, g2 = step(a)                                    # same batch, same token masks (seed 5), the RNG advanced: new dropout masks
    assert not torch.equal(eng.rng, state) and l2 != la
    assert any(not torch.equal(g2[k], ga[k]) for k in ga)


# ---------------------------------------------------------------------------------------------- resume, graph replay, errors, the default plan
def test_dec_case_resume_from_train_state_is_bit_identical(tmp_path):
    """model_checks.resume_roundtrip for DEC with the trainer's own modal_filter (single-modality output: eval_mask is 1 for behaviour, 0
    for spikes, trainer/base.py `single_modal`): 6 steps in one go == 3 steps, save_model + save_train_state, fresh objects restored from
    the files (load_train_state), 3 more steps, every state-dict tensor bit for bit; eval_epoch runs over modal_filter['output']."""
    from trainer.make import make_multimodal_trainer
    from multi_modal_foundation_model_amd.ddp import Accelerator
    B, T, n_ap, n_beh = 2, 8, 12, 2
    mf = dict(input=["ap"], output=["behavior"])

    def batches(lo, hi):
        out = []
        for i in range(lo, hi):
            b = O.synth_batch(B, T, n_ap, n_beh, seed=i)
            b["eid"] = ["synthetic"] * B
            b["neuron_regions"] = [["XX"] * B for _ in range(n_ap)]
            out.append(b)
        return out

    def make(model, loader, log_dir, evals=()):
        acc = Accelerator()
        model = acc.prepare(model)
        opt, sch = make_optimizer(model, 40, lr=1e-3)
        tr = make_multimodal_trainer(model=model, train_dataloader=loader, eval_dataloader=list(evals), optimizer=opt, log_dir=str(log_dir),
                                     accelerator=acc, lr_scheduler=sch, avail_mod=list(BOTH), config=load_config(), modal_filter=mf,
                                     mixed_training=True, num_neurons=[n_ap])
        return model, opt, sch, tr

    def fresh():
        model = case_model("DEC", n_ap, n_beh, seed=7, n_enc=2, n_dec=2, dropout=0.4, emb_dropout=0.2)
        model.engine_seed = 5
        return model

    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    m0, opt0, sch0, tr0 = make(fresh(), batches(0, 6), tmp_path / "a")
    random.seed(42); torch.manual_seed(99)
    tr0.train_epoch(0)
    want = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    assert all(bool(torch.isfinite(v).all()) for v in want.values())
    m1, opt1, sch1, tr1 = make(fresh(), batches(0, 3), tmp_path / "b", evals=batches(10, 12))
    random.seed(42); torch.manual_seed(99)
    tr1.train_epoch(0)
    tr1.save_model(name="last", epoch=0)
    del m1, opt1, sch1, tr1
    random.seed(0); torch.manual_seed(0)
    ck = torch.load(tmp_path / "b" / "model_last.pt", weights_only=False)            # our own file (whole-module pickle, like the reference)
    keys = list(ck["model"].state_dict())
    assert not any(k.startswith(("encoder_embeddings.behavior", "decoder_embeddings.ap")) for k in keys) and len(keys) == len(want)
    m2, opt2, sch2, tr2 = make(ck["model"], batches(3, 6), tmp_path / "b", evals=batches(10, 12))
    assert tr2.load_train_state(name="last") == 0
    assert (m2._engine.cfg.enc_mods, m2._engine.cfg.dec_mods) == (["ap"], ["behavior"])
    tr2.train_epoch(1)
    assert list(m2.state_dict()) == list(want)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, want[k]), k
    res = tr2.eval_epoch()                               # iterates modal_filter['output'] only
    assert math.isfinite(res["eval_loss"]) and set(res["eval_preds"][0]) == {"behavior"} and res["eval_preds"][0]["behavior"].shape == (4, T, n_beh)


def test_dec_case_graph_replay_gives_the_eager_losses(monkeypatch):
    g = load_json("modal_filter_curve.json")["DEC"]
    MC.graph_replay_matches_eager(monkeypatch, lambda: case_model("DEC", g["n_ap"], g["n_beh"], seed=g["model_seed"]), g)


@pytest.mark.parametrize("inp,out", [(BOTH, ["behavior"]), (["ap"], BOTH)])
def test_sets_of_different_size_raise_on_the_device_model(inp, out):
    """Upstream fails in CrossAttention.forward; the device model raises before any launch: no engine is made."""
    model = build_model(tiny_config(), 12, 2, seed=7, modal_filter=dict(input=inp, output=out)).cuda().train()
    torch.manual_seed(11)
    with pytest.raises(RuntimeError, match=f"length {8 * len(inp)} .* length {8 * len(out)} "):
        model(MC.to_dev(O.make_mod_dict(O.synth_batch(2, 8, 12, 2, seed=3), "token_masking")))
    assert model._engine is None
    from multi_modal_foundation_model_amd.engine import Engine
    from modal_filter import engine_config
    eng = Engine(engine_config(model, [("ap", 12), ("behavior", 2)]), "cuda")
    with pytest.raises(RuntimeError, match="lengths equal"):         # the plan builder refuses too, before it lays anything out
        eng._plan(2, 8, True, True)


def test_default_model_plan_call_count_is_unchanged():
    """The YAML model in bf16 at B = 64, T = 100 (every group fused): 81 forward + 222 backward calls, one mask_prep, no decoder-side mask
    buffers - through the default builders and through a modal_filter that names both modalities on both sides."""
    for mf in (None, dict(input=BOTH, output=BOTH)):
        model = build_model(load_config().model, 668, 2, seed=42, modal_filter=mf)
        model.compute_dtype = "bf16"
        model.cuda()
        plan = model.engine()._plan(64, 100, True, True)
        fwd, bwd = [fn.__name__ for fn, _, _ in plan["fwd"]], [fn.__name__ for _, seg in plan["bwd"] for fn, _, _ in seg]
        assert (len(fwd), len(bwd)) == (81, 222) and fwd.count("mmfm_mask_prep") == 1
        assert not any(k.startswith("dec/") for k in plan["b"]) and plan["count"] == "count"
        del model, plan
        torch.cuda.empty_cache()
