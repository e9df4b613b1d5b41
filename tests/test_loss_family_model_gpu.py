"""The loss family through the whole model: MultiModal with `loss_mod` entries of the new kinds (a rate-output spike head with
PoissonNLLLoss(log_input=False, full=True), a Huber behaviour head, an added BCE-with-logits modality) in fp32 and bf16, train and
eval mode, against the losses recomputed on the host in fp64 from the predictions the model returns (tests/loss_refs.py); and the
default two-modality model, whose step plan and loss must be what they were.  Runs on the MI355X only."""
import pytest
import torch
import torch.nn as nn

import edge_refs as E
import loss_refs as R
from helpers import build_model, load_config
from model_checks import to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

MODS, B, T, make_model = R.FAMILY_MODS, R.FAMILY_B, R.FAMILY_T, R.make_family_model
SPECS = {"ap": (R.POISSON_RATE, 1e-8, R.FULL), "behavior": (R.HUBER, 0.5, 0), "choice": (R.BCE_LOGITS, 0.0, 0)}


def make_batch():
    batch = O.synth_batch_mods(B, T, MODS, seed=3)
    g = torch.Generator().manual_seed(4)
    batch["data"]["ap"] = torch.poisson(torch.full((B, T, 12), 1.2), generator=g)          # counts >= 2 in every row: full=True bites
    batch["data"]["choice"] = (torch.rand(B, T, 3, generator=g) < 0.5).float()
    md = O.make_mod_dict_mods(batch, MODS, None)
    for i, (name, n) in enumerate(MODS):       # a token mask per modality, given the way an eval_mask is: [B, T, n], channel 0 is read
        mk = (torch.rand(B, T, generator=g) < 0.5).to(torch.int64)
        mk[0, i], mk[1, i + 1] = 1, 0
        md[name]["eval_mask"] = mk[:, :, None].repeat(1, 1, n)
    return to_dev(md)


def sum_bound(dpred_ref, per_elem, dim):
    """A column sum of elements each within `per_elem` of dpred_ref, accumulated in fp32: sum of the element bounds + n u sum|terms|."""
    n = dpred_ref.shape[dim]
    return per_elem.sum(dim) + n * E.U32 * dpred_ref.abs().sum(dim)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_three_modalities_on_the_new_kinds(dtype):
    model = make_model(dtype)
    for training in (True, False):
        model.train(training)
        model.zero_grad(set_to_none=True)
        md = make_batch()
        with torch.set_grad_enabled(training):             # eval: the forward-only plan, as the trainer's eval_epoch runs it
            out = model(md)
        eng = model._engine
        assert (eng._last["bwd"] is not None) == training
        assert eng.cfg.loss_kind == {m: s[0] for m, s in SPECS.items()}
        names = [fn.__name__ for fn, _, _ in eng._last["fwd"]]
        assert names.count("mmfm_masked_loss_kind_fwd") == 3 and "mmfm_masked_loss_fwd" not in names
        sums, counts = {}, {}
        for m, n in MODS:
            pred, tgt, mask = out.mod_preds[m], md[m]["targets"], md[m]["targets_mask"]
            assert pred.dtype == (torch.bfloat16 if (dtype == "bf16" and training) else torch.float32)
            if m == "ap":
                assert pred.min().item() > 0, "the rate head must predict positive rates for this test"
                assert bool((tgt[mask.bool()] >= 2).any())
            rowmask = mask.to(torch.uint8)
            kind, param, flags = SPECS[m]
            s, cnt, _, _ = R.masked_loss_sum(kind, pred.reshape(B * T, n), tgt.reshape(B * T, n), rowmask, param, flags)
            assert cnt > 0 and int(out.mod_n_examples[m]) == int(cnt)
            E.check_close(out.mod_loss[m].reshape(1), s.reshape(1), E.TOL_LOSS, f"{dtype} train={training} mod_loss[{m}]")
            sums[m], counts[m] = s, cnt
        total_n = sum(counts.values())
        loss_ref = sum(sums.values()) / total_n
        E.check_close(out.loss.detach().reshape(1), loss_ref.reshape(1), E.TOL_LOSS, f"{dtype} train={training} loss")
        if not training:
            continue
        out.loss.backward()
        assert "mmfm_masked_loss_kind_bwd" in [fn.__name__ for _, seg in eng._last["bwd"] for fn, _, _ in seg]
        inv_n = torch.tensor(1.0 / total_n, dtype=torch.float64, device="cuda")
        for m, n in MODS:
            kind, param, _ = SPECS[m]
            dp = R.masked_loss_bwd(kind, out.mod_preds[m].reshape(B * T, n), md[m]["targets"].reshape(B * T, n),
                                   md[m]["targets_mask"].to(torch.uint8), torch.ones(1, device="cuda"), inv_n, param)
            per_elem = E.TOL_DPRED[1] + E.TOL_DPRED[0] * dp.abs()                 # fp32: the kernel test's elementwise bound
            if dtype == "bf16":
                per_elem = per_elem + E.HALF_ULP_BF16 * dp.abs()                    # check_bf16: dpred is stored in bf16
            got = E.f64(model.decoder_embeddings[m].out.bias.grad)
            ref, bound = dp.sum(0), sum_bound(dp, per_elem, 0)
            err = (got - ref).abs()
            print(f"[loss family] {dtype} d out.bias[{m}]: worst |err| / bound = {float((err / bound).max()):.3e}")
            assert bool((err <= bound).all()), f"{dtype} out.bias.grad[{m}]: {got.tolist()} vs {ref.tolist()} (bound {bound.tolist()})"


def test_default_model_plan_and_loss_are_what_they_were():
    """The default model (loss_mod = the strings "poisson_nll_log_input" / "mse", kinds 0 / 1) builds the plan it always built - 81
    forward + 222 backward calls in bf16 once every group is fused, the two-kind loss entry points, none of the new ones - and a model
    whose entries are the reference's own modules builds the same plan and computes the same loss, bit for bit."""
    def run(loss_mod):
        model = build_model(load_config().model, 668, 2, seed=42)
        if loss_mod is not None:
            model.loss_mod.update(loss_mod)
        assert [type(model.loss_mod[m]) for m in ("ap", "behavior")] == ([str, str] if loss_mod is None else [nn.PoissonNLLLoss, nn.MSELoss])
        model.compute_dtype = "bf16"
        model.cuda().train()
        md = to_dev(O.make_mod_dict(O.synth_batch(64, 100, 668, 2, seed=0), "encoding"))        # R = 12,800 rows: every group fused
        out = model(md)
        out.loss.backward()
        plan = model._engine._last
        return out.loss.detach().clone(), [fn.__name__ for fn, _, _ in plan["fwd"]], [fn.__name__ for _, seg in plan["bwd"] for fn, _, _ in seg], model
    loss_a, fwd_a, bwd_a, model_a = run(None)
    assert model_a.loss_mod == {"ap": "poisson_nll_log_input", "behavior": "mse"}
    assert (len(fwd_a), len(bwd_a)) == (81, 222)
    assert fwd_a.count("mmfm_masked_loss_fwd") == 2 and bwd_a.count("mmfm_masked_loss_bwd") == 2
    assert not [n for n in fwd_a + bwd_a if "masked_loss_kind" in n]
    assert model_a._engine.cfg.loss_kind == {"ap": 0, "behavior": 1}
    del model_a
    loss_b, fwd_b, bwd_b, _ = run({"ap": nn.PoissonNLLLoss(reduction="none", log_input=True), "behavior": nn.MSELoss(reduction="none")})
    assert (fwd_b, bwd_b) == (fwd_a, bwd_a)
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b), (loss_a.item(), loss_b.item())
