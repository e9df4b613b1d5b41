"""Neuron padding (space_attn_mask with MultiModal.neuron_padding) on the MI355X, fp32 engine against the reference's own pieces composed
as mm.py:245-300 calls them with the channel mask honoured (tests/golden/neuron_padding_*, scripts/make_neuron_padding_goldens.py):
losses, per-modality sums and every gradient norm within 1e-4, counts exact, NaN where the reference is NaN, and a 50-step curve over
three sessions of different widths."""
import random

import numpy as np
import pytest
import torch

import mod_segments as S
import model_checks as MC
import neuron_padding as NP
from conftest import load_json, load_npz
from helpers import build_model, make_optimizer, tiny_config

pytestmark = pytest.mark.gpu

MODS = ("ap", "behavior")
REL = 1e-4
# gradient norms below this are rounding noise around an exact zero (a key bias: softmax is invariant to it), where a relative
# bound says nothing; the figure is the one tests/model_checks.py applies to gradient norms
NORM_FLOOR = 1e-8


def fresh(case=None, dtype="fp32", **cfg):
    model = build_model(tiny_config(**cfg), NP.TINY["n_ap"], NP.TINY["n_beh"], seed=NP.MODEL_SEED, neuron_padding=True,
                        input_masking=bool(case and NP.CASES[case].get("mode")))
    NP.set_masker(model.masker, case)
    model.compute_dtype = dtype
    return model.cuda().train()


@pytest.fixture(scope="module")
def golden():
    return load_npz("neuron_padding_fwd_bwd.npz")


def fixture_batch(z, case):
    batch = {mod: {k: torch.from_numpy(z[f"batch/{case}/{mod}/{k}"]) for k in ("inputs", "ts", "attn")} for mod in MODS}
    return batch, torch.from_numpy(z[f"batch/{case}/space_attn_mask"])


@pytest.mark.parametrize("case", list(NP.CASES))
def test_fp32_engine_against_the_reference_pieces(golden, case):
    z, meta = golden
    assert meta["cases"] == list(NP.CASES)
    model = fresh(case)
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names
    batch, v = fixture_batch(z, case)
    torch.manual_seed(NP.MASKER_SEED)
    random.seed(NP.MASKER_SEED)
    md = MC.to_dev(NP.case_mod_dict(case, batch, v))
    out = model(md)
    out.loss.backward()
    eng = model._engine
    ref_loss = float(z[f"{case}/loss"])
    print(case, "loss", out.loss.item(), "reference", ref_loss)
    for i, mod in enumerate(MODS):
        Bm, Tm, Nm = batch[mod]["inputs"].shape
        print(case, mod, "n", int(out.mod_n_examples[mod]), int(z[f"{case}/n/{mod}"]), "sum", out.mod_loss[mod].item(), float(z[f"{case}/mod_loss/{mod}"]))
        assert int(out.mod_n_examples[mod]) == int(z[f"{case}/n/{mod}"])
        np.testing.assert_array_equal(md[mod]["inputs_mask"].cpu().numpy(), z[f"{case}/mask/{mod}"])
        staged = eng.b[f"in/{i}"].view(Bm, Tm, -1)[..., :Nm]
        np.testing.assert_array_equal(staged.cpu().numpy(), z[f"{case}/inputs/{mod}"])
        assert out.mod_loss[mod].item() == pytest.approx(float(z[f"{case}/mod_loss/{mod}"]), rel=REL, abs=1e-6)
        assert tuple(out.mod_preds[mod].shape) == (Bm, Tm, Nm), "mod_preds keeps its [B, T, N] shape"
        real = (v[:, None, :].expand(Bm, Tm, Nm) != 0).numpy() if mod == "ap" else np.ones((Bm, Tm, Nm), dtype=bool)
        np.testing.assert_allclose(out.mod_preds[mod].cpu().numpy()[real], z[f"{case}/preds/{mod}"][real], rtol=1e-4, atol=2e-5)
    if np.isnan(ref_loss):                 # nothing is a target: 0 / 0 and NaN gradients, as upstream
        assert sum(int(n) for n in out.mod_n_examples.values()) == 0 and bool(torch.isnan(out.loss))
        for k, gn in zip(names, z[f"{case}/grad_norm"]):
            assert bool(torch.isnan(named[k].grad.double().norm())) == bool(np.isnan(gn)), k
        return
    assert out.loss.item() == pytest.approx(ref_loss, rel=REL)
    worst = max((abs(float(named[k].grad.double().norm()) / float(gn) - 1), k) for k, gn in zip(names, z[f"{case}/grad_norm"]) if gn > NORM_FLOOR)
    print(case, "worst gradient-norm error", worst)
    for k, gn in zip(names, z[f"{case}/grad_norm"]):
        assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=REL, abs=NORM_FLOOR), k
    stored = MC.check_stored_grads(named, z, case, names)
    assert len(stored) == (len(names) if case in NP.FULL_GRAD else 0)


def test_50_step_curve_over_three_sessions():
    g = load_json("neuron_padding_curve.json")
    assert g["sessions"] == list(NP.CURVE_SESSIONS) and len(set(g["sessions"])) == 3
    model = fresh()
    opt, sch = make_optimizer(model, g["total_steps"])
    random.seed(42)
    torch.manual_seed(1234)
    losses = []
    for s in range(g["total_steps"]):
        obj = random.sample(list(S.OBJECTIVES), 1)[0]
        assert obj == g["objective"][s]
        batch, v = NP.curve_batch(s)
        out = model(MC.to_dev(NP.make_mod_dict(batch, v, obj)))
        out.loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(out.loss.detach())
    losses = [x.item() for x in losses]
    print("curve", losses[:3], "...", losses[-1], "reference", g["loss"][:3], "...", g["loss"][-1])
    print("curve worst", max(abs(a / b - 1) for a, b in zip(losses, g["loss"])))
    np.testing.assert_allclose(losses, g["loss"], rtol=REL)
