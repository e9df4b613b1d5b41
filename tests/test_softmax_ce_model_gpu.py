"""Softmax cross-entropy through the whole model on the MI355X: MultiModal with a categorical third modality whose `loss_mod` entry is
a multi_modal.losses.SoftmaxCrossEntropy.  The fp32 engine against the reference's own forward / backward and 50-step curves
(tests/golden/softmax_ce_*, scripts/make_softmax_ce_goldens.py: a per-trial label on a segmented plan, a per-bin label on the uniform
plan); a bf16 and an fp32 step against the loss recomputed in fp64 from the returned predictions (tests/ce_refs.py); hipGraph replay; a
frozen head; the accuracy of the evaluation predictions."""
import numpy as np
import pytest
import torch

import ce_refs as R
import edge_refs as E
from conftest import load_json, load_npz
from helpers import make_optimizer
from model_checks import to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-4                     # the fixture tolerance: losses, per-modality losses, gradient norms, the curve
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("softmax_ce_fwd_bwd.npz")
    return _Z


def mod_dict(case, objective, seed=R.CE_DATA_SEED):
    return to_dev(R.ce_mod_dict(case, R.ce_batch(case, seed), objective))


def call_names(plan):
    return [fn.__name__ for fn, _, _ in plan["fwd"]], [fn.__name__ for _, seg in (plan["bwd"] or []) for fn, _, _ in seg]


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("objective", R.CE_OBJECTIVES)
@pytest.mark.parametrize("case", list(R.CE_CASES))
def test_forward_backward_vs_reference_fixture(case, objective):
    z, meta = fixture()
    p = f"{case}/{objective}"
    c = R.CE_CASES[case]
    cat = c["mods"][2][0]
    model = R.make_ce_model(case).train()
    torch.manual_seed(meta["masker_seed"])
    md = mod_dict(case, objective)
    out = model(md)
    out.loss.backward()
    print(p, "loss", out.loss.item(), "reference", float(z[f"{p}/loss"]))
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=TOL)
    for (m, n), T in zip(c["mods"], c["T"]):
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"{p}/mask/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=TOL, abs=1e-6)
        assert tuple(out.mod_preds[m].shape) == (R.CE_B, T, n)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    if objective == "eval_masks":           # upstream's n_examples: C * (masked tokens)
        assert int(out.mod_n_examples[cat]) == c["mods"][2][1] * R.CE_B * c["T"][2]
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names and list(model.state_dict()) == [k for k, _ in meta["state"][case]]
    worst = 0.0
    for k, gn in zip(names, z[f"{p}/grad_norm"]):
        got = float(named[k].grad.double().norm())
        if k.endswith("key.bias"):          # softmax is invariant to a key bias: the true gradient is 0, both sides hold rounding noise
            assert got <= 1e-6 and float(gn) <= 1e-6, k
            continue
        worst = max(worst, abs(got - float(gn)) / max(float(gn), 1e-30) if gn > 0 else got)
        assert got == pytest.approx(float(gn), rel=TOL, abs=1e-8), k
    print(p, "worst relative gradient-norm gap", worst)
    stored = [k for k in names if f"{p}/grad/{k}" in z.files]
    assert len(stored) == (len(names) if p == meta["full_grad"] else 0)
    for k in stored:                        # elementwise: 1e-4 of the element, or of the tensor's largest where the element is small
        g, ref = named[k].grad.cpu().numpy(), z[f"{p}/grad/{k}"]
        np.testing.assert_allclose(g, ref, rtol=TOL, atol=1e-8 + TOL * np.abs(ref).max(), err_msg=k)
    plan = model._engine._last
    fwd, bwd = call_names(plan)
    assert fwd.count("mmfm_softmax_ce_fwd") == 1 and bwd.count("mmfm_softmax_ce_bwd") == 1
    assert fwd.count("mmfm_masked_loss_fwd") == 2 and not [n for n in fwd + bwd if "masked_loss_kind" in n]
    assert plan["T"] == (c["T"] if len(set(c["T"])) > 1 else c["T"][0])
    assert ("mmfm_mask_prep_seg" in fwd) == (case == "choice")
    assert model._engine.cfg.loss_kind[cat] == R.SOFTMAX_CE and model._engine.cfg.loss_param[cat] == c["eps"]
    assert model._engine.cfg.loss_weight == ({cat: tuple(c["weight"])} if c["weight"] else {})


def run_curve(model, case, steps, total_steps, objectives):
    opt, sch = make_optimizer(model, total_steps)
    model.train()
    torch.manual_seed(1234)
    losses = []
    for s in range(steps):
        out = model(mod_dict(case, objectives[s], seed=s))
        out.loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(out.loss.detach())
    return [x.item() for x in losses]


@pytest.mark.parametrize("case", list(R.CE_CASES))
def test_loss_curve_50_steps_vs_reference_fixture(case):
    g = load_json("softmax_ce_curve.json")[case]
    losses = run_curve(R.make_ce_model(case), case, 50, g["total_steps"], g["objective"])
    print(case, "max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=TOL)


# ---------------------------------------------------------------------------------------------- fp32 and bf16 against fp64 of the returned predictions
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_choice_step_against_fp64_of_the_returned_predictions(dtype):
    case = "choice"
    c = R.CE_CASES[case]
    (cat, Cn), Tc = c["mods"][2], c["T"][2]
    w = torch.tensor(c["weight"], device="cuda")
    model = R.make_ce_model(case, dtype)
    for training in (True, False):
        model.train(training)
        model.zero_grad(set_to_none=True)
        md = mod_dict(case, "eval_masks")
        with torch.set_grad_enabled(training):
            out = model(md)
        eng = model._engine
        plan = eng._last
        assert (plan["bwd"] is not None) == training
        args = [a for fn, a, _ in plan["fwd"] if fn.__name__ == "mmfm_softmax_ce_fwd"]
        assert len(args) == 1 and (args[0][11] is not None) == training, "rowstat: saved by the training plan, NULL in the forward-only plan"
        assert args[0][3] == eng.loss_w[cat].data_ptr() and args[0][4] == pytest.approx(c["eps"])
        pred, tgt, mask = out.mod_preds[cat], md[cat]["targets"], md[cat]["targets_mask"]
        assert pred.dtype == (torch.bfloat16 if (dtype == "bf16" and training) else torch.float32)
        rowmask = mask.to(torch.uint8)
        s, cnt, _, _ = R.masked_ce_sum(pred.reshape(-1, Cn), tgt.reshape(-1, Cn), rowmask, w, c["eps"])
        assert int(out.mod_n_examples[cat]) == int(cnt) == Cn * R.CE_B * Tc
        E.check_close(out.mod_loss[cat].reshape(1), s.reshape(1), E.TOL_LOSS, f"{dtype} train={training} mod_loss[{cat}]")
        # the total: behaviour's MSE over its masked bins in fp64 (ap is not masked), plus the cross-entropy, over the summed counts
        bp, bt, bm = out.mod_preds["behavior"], md["behavior"]["targets"], md["behavior"]["targets_mask"].bool()
        s_beh = ((E.f64(bp) - E.f64(bt)) ** 2)[bm].sum()
        total_n = cnt + float(bm.sum()) * 2
        assert int(out.mod_n_examples["ap"]) == 0 and int(out.mod_n_examples["behavior"]) == int(bm.sum()) * 2
        E.check_close(out.loss.detach().reshape(1), ((s + s_beh) / total_n).reshape(1), E.TOL_LOSS, f"{dtype} train={training} loss")
        if not training:
            from multi_modal_foundation_model_amd import metrics as Mx
            acc = float((R.first_argmax(pred.reshape(-1, Cn)) == R.first_argmax(tgt.reshape(-1, Cn)))[mask.reshape(-1).bool()].double().mean())
            assert Mx.accuracy(pred, tgt, mask) == pytest.approx(acc, abs=1e-12)
            conf = Mx.confusion(pred, tgt, mask)
            assert conf.shape == (Cn, Cn) and int(conf.sum()) == R.CE_B * Tc
            continue
        out.loss.backward()
        assert "mmfm_softmax_ce_bwd" in call_names(plan)[1]
        inv_n = torch.tensor(1.0 / total_n, dtype=torch.float64, device="cuda")
        dp, per_elem = R.masked_ce_bwd(pred.reshape(-1, Cn), tgt.reshape(-1, Cn), rowmask, torch.ones(1, device="cuda"), inv_n, w, c["eps"])
        per_elem = per_elem + 2 * E.U32 * dp.abs()            # inv_n is the engine's fp32 1 / n, not the fp64 one handed to the reference
        if dtype == "bf16":
            per_elem = per_elem + E.HALF_ULP_BF16 * dp.abs()      # dpred is stored in bf16
        got = E.f64(model.decoder_embeddings[cat].out.bias.grad)
        ref = dp.sum(0)
        bound = per_elem.sum(0) + dp.shape[0] * E.U32 * dp.abs().sum(0)
        err = (got - ref).abs()
        print(f"[softmax ce] {dtype} d out.bias[{cat}]: worst |err| / bound = {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), f"{dtype} out.bias.grad[{cat}]: {got.tolist()} vs {ref.tolist()} (bound {bound.tolist()})"


# ---------------------------------------------------------------------------------------------- graph replay, a frozen head
def test_graph_replay_gives_the_eager_losses(monkeypatch):
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MMFM_GRAPH", mode)
        model = R.make_ce_model("choice")
        res[mode] = run_curve(model, "choice", 5, 50, ["token_masking"] * 5)
        plan = model._engine._last
        assert (set(plan["graphs"]) == {"fwd", "bwd"}) == (mode == "1") and plan["runs"]["fwd"] == 5
    print("eager", res["0"], "graph", res["1"])
    assert res["0"] == res["1"] and all(np.isfinite(res["0"]))


def test_a_frozen_choice_head_prunes_its_backward_call():
    """Only the spike head trains: nothing below the heads needs d/ydec, so neither the cross-entropy backward nor behaviour's is emitted,
    and the spike head's gradient is what the all-trainable plan writes."""
    def step(freeze):
        model = R.make_ce_model("choice").train()
        if freeze:
            for k, prm in model.named_parameters():
                prm.requires_grad_(k.startswith("decoder_embeddings.ap.out."))
        torch.manual_seed(11)
        out = model(mod_dict("choice", "token_masking"))
        out.loss.backward()
        return model, out.loss.item(), call_names(model._engine._last)[1]
    full, loss_a, bwd_a = step(False)
    frozen, loss_b, bwd_b = step(True)
    assert loss_a == loss_b
    assert bwd_a.count("mmfm_softmax_ce_bwd") == 1 and bwd_a.count("mmfm_masked_loss_bwd") == 2
    assert "mmfm_softmax_ce_bwd" not in bwd_b and bwd_b.count("mmfm_masked_loss_bwd") == 1
    assert "decoder_embeddings.choice.out" in frozen._engine.backward_report(R.CE_B, R.CE_CASES["choice"]["T"])["pruned"]
    for k in ("weight", "bias"):
        a, b = (getattr(m.decoder_embeddings["ap"].out, k).grad for m in (full, frozen))
        assert torch.equal(a, b), k
    assert frozen.decoder_embeddings["choice"].out.weight.grad is None
