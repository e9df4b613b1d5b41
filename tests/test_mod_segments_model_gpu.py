"""Modalities of different length, time stamps and padding on the MI355X, whole models (segmented plans).
The fp32 engine against the reference's own forward / backward and 50-step curve on ragged batches (tests/golden/mod_segments_*,
scripts/make_mod_segments_goldens.py); the bf16 engine against the fp32 engine at the default widths on a sequence that is a multiple
of no tile; a dropout-on step; hipGraph replay; the uniform plan next to a segmented one; the default model's plan."""
import contextlib
import math
from unittest import mock

import numpy as np
import pytest
import torch

import mod_segments as S
import model_checks as MC
from conftest import load_json, load_npz
from helpers import build_model, load_config, model_config, tiny_config
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("mod_segments_fwd_bwd.npz")
    return _Z


def case_model(case, seed=S.MODEL_SEED, config=tiny_config, **kw):
    sw = S.CASES[case]
    kw.setdefault("max_F", S.TINY["max_F"])
    return build_model(config(sep=sw.get("sep", False), causal=sw.get("causal", False), **kw), S.TINY["n_ap"], S.TINY["n_beh"], seed=seed)


@contextlib.contextmanager
def ragged(case):
    """model_checks' bodies on the case's ragged batches: the fixture batch and the curve's per-step batches (data seed = step) come
    from tests/mod_segments.py, the mod_dict is the per-modality one."""
    with mock.patch.object(MC, "fixture_batch", lambda z, prefix="batch/": S.case_batch(case)), \
            mock.patch.object(O, "synth_batch", lambda *a, seed, **kw: S.case_batch(case, seed)), \
            mock.patch.object(O, "make_mod_dict", S.make_mod_dict):
        yield


def test_fixture_batches_are_the_shared_recipe():
    z, _ = fixture()
    for case in S.CASES:
        for mod, d in S.case_batch(case).items():
            for k, v in d.items():
                np.testing.assert_array_equal(v.numpy(), z[f"batch/{case}/{mod}/{k}"])


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("case", list(S.CASES))
@pytest.mark.parametrize("objective", S.OBJECTIVES)
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """model_checks.check_fixture_case, bounds and all, with every gradient tensor of ALL / token_masking."""
    z, meta = fixture()
    assert f"{case}/{objective}" not in meta["nan"]
    model = case_model(case, seed=meta["model_seed"])
    with ragged(case):
        stored = MC.check_fixture_case(model, z, meta, case, objective)
    assert len(stored) == (len(meta["params"][case]) if (case, objective) == ("ALL", "token_masking") else 0)
    T = S.CASES[case]["T"]
    plan = model._engine._last
    names = [fn.__name__ for fn, _, _ in plan["fwd"]]
    assert plan["T"] == T and plan["R"] == S.TINY["B"] * sum(T) and names.count("mmfm_mask_prep_seg") == 1 and "mmfm_mask_prep" not in names
    assert names.count("mmfm_stitch_fwd_seg") == 4 and names.count("mmfm_layernorm_fwd_seg") == 1 and "mmfm_live_bins" not in names
    out_shapes = {m: tuple(model(MC.to_dev(S.make_mod_dict(S.case_batch(case), objective))).mod_preds[m].shape) for m in S.MODS}
    assert out_shapes == {"ap": (3, T[0], 12), "behavior": (3, T[1], 2)}


def test_loss_curve_tiny_50_steps_vs_reference_fixture():
    g = load_json("mod_segments_curve.json")["ALL"]
    model = case_model(g["case"], seed=g["model_seed"]).cuda()
    with ragged(g["case"]):
        losses = MC.run_curve(model, 50, g["B"], None, g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- bf16 at the default widths
WIDE = dict(B=4, T=(37, 23), n_ap=40, n_beh=2, max_F=40)


def wide_batch(seed=6):
    """B = 4, ap 37 bins / behaviour 23: L = 60 and R = 240 are multiples of neither the 128-row pass nor the 64-key tile.  Behaviour's
    stamps are reversed and shifted per sample, two samples of each modality are right-padded (sample 0 among them)."""
    return S.ragged_batch(WIDE["B"], WIDE["T"], WIDE["n_ap"], WIDE["n_beh"], seed, "shifted", ((5, 0, 11, 0), (0, 7, 0, 2)), WIDE["max_F"])


def wide_step(dtype, objective, heads, dropout=0.0, model=None, seed=3):
    if model is None:
        model = build_model(model_config(heads=heads, n_enc=2, n_dec=2, max_F=WIDE["max_F"], sep=True, causal=True, dropout=dropout,
                                         emb_dropout=dropout / 2), WIDE["n_ap"], WIDE["n_beh"], seed=seed)
        model.compute_dtype, model.engine_seed = dtype, 77
        model.cuda().train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    out = model(MC.to_dev(S.make_mod_dict(wide_batch(), objective)))
    out.loss.backward()
    torch.cuda.synchronize()
    return model, out


@pytest.mark.parametrize("heads", [8, 4], ids=["dh32", "dh64"])
@pytest.mark.parametrize("objective", S.OBJECTIVES)
def test_bf16_step_at_default_widths_vs_fp32_engine(objective, heads):
    """Hidden 256 / inter_size 512, 2 + 2 layers, sep + causal decoder masks, dropout 0: one bf16 step against the fp32 engine on the
    same weights and masks at model_checks.check_bf16's bounds.  8 heads: the dh-32 fast attention pair; 4 heads (dh 64):
    csrc/attention_long.hip sees a mod_id whose slots are 37 and 23 long."""
    m32, o32 = wide_step("fp32", objective, heads)
    m16, o16 = wide_step("bf16", objective, heads)
    assert m16._engine._last["R"] == 240 and m16._engine._last["T"] == WIDE["T"]
    assert [int(o16.mod_n_examples[m]) for m in S.MODS] == [int(o32.mod_n_examples[m]) for m in S.MODS]
    named = {k: p.grad for k, p in m16.named_parameters()}
    grads = {k: p.grad.double() for k, p in m32.named_parameters()}
    MC.check_bf16(MC.bf16_stats(o16, named, dict(loss=o32.loss.double()), grads), f"bf16 ragged {objective} {heads} heads vs fp32 engine")


def test_bf16_dropout_step_is_a_function_of_the_rng_state():
    """Two fresh models step from the same RNG state: the loss and every gradient bit for bit; the next step on the same batch and token
    masks draws new dropout masks.  The tokeniser sites report their own row counts."""
    (a, oa), (b, ob) = (wide_step("bf16", "token_masking", 8, dropout=0.4) for _ in range(2))
    ga, gb = ({k: p.grad.clone() for k, p in m.named_parameters()} for m in (a, b))
    assert oa.loss.item() == ob.loss.item() and math.isfinite(oa.loss.item()) and all(torch.equal(ga[k], gb[k]) for k in ga)
    eng = a._engine
    rows = {s["key"]: s["shape"][0] for s in eng.dropout_sites(WIDE["B"], WIDE["T"]) if "/embdrop/" in s["key"]}
    assert rows == {f"{side}/embdrop/{m}": WIDE["B"] * WIDE["T"][m] for side in ("encoder", "decoder") for m in (0, 1)}
    state = eng.rng.clone()
    _, o2 = wide_step("bf16", "token_masking", 8, model=a)
    assert not torch.equal(eng.rng, state) and o2.loss.item() != oa.loss.item()
    assert any(not torch.equal(p.grad, ga[k]) for k, p in a.named_parameters())
    assert eng.backward_report(WIDE["B"], WIDE["T"])["launches"] > 0 and "backward:" in eng.backward_summary(WIDE["B"], WIDE["T"])


# ---------------------------------------------------------------------------------------------- graph replay, plan pooling, the default plan
def test_ragged_graph_replay_gives_the_eager_losses(monkeypatch):
    g = dict(load_json("mod_segments_curve.json")["ALL"], T=None)
    with ragged("ALL"):
        MC.graph_replay_matches_eager(monkeypatch, lambda: case_model("ALL", seed=g["model_seed"]), g)


def test_uniform_plan_is_reused_around_a_ragged_batch():
    """Uniform, ragged, uniform again: the uniform batch keeps its plan (the int key, today's entry points) and its buffers; a batch of
    equal lengths whose stamps differ is a segmented plan of its own."""
    model = case_model("LEN").cuda().train()

    def step(md):
        torch.manual_seed(11)
        out = model(MC.to_dev(md))
        out.loss.backward()
        return out.loss.item(), model._engine._last

    uni = lambda: O.make_mod_dict(O.synth_batch(3, 8, 12, 2, seed=3), "token_masking")
    l0, p0 = step(uni())
    _, p1 = step(S.make_mod_dict(S.case_batch("LEN"), "token_masking"))
    l2, p2 = step(uni())
    _, p3 = step(S.make_mod_dict(S.case_batch("STAMPS"), "token_masking"))
    assert p0 is p2 and l0 == l2 and p0["T"] == 8 and p1["T"] == (8, 5) and p3["T"] == (8, 8) and len({id(p) for p in (p0, p1, p3)}) == 3
    names = lambda p: {fn.__name__ for fn, _, _ in p["fwd"]} | {fn.__name__ for _, seg in p["bwd"] for fn, _, _ in seg}
    assert not any(n.endswith("_seg") for n in names(p0))
    assert {"mmfm_mask_prep_seg", "mmfm_stitch_fwd_seg", "mmfm_stitch_bwd_seg", "mmfm_layernorm_fwd_seg", "mmfm_layernorm_bwd_seg"} <= names(p1)
    assert set(model._engine._pools) == {(3, 8), (3, (8, 5)), (3, (8, 8))}
    md = uni()                                          # equal copies of the stamps and the mask are shared bins too
    md["behavior"]["inputs_timestamp"] = md["behavior"]["inputs_timestamp"].clone()
    md["behavior"]["inputs_attn_mask"] = md["behavior"]["inputs_attn_mask"].clone()
    assert step(md)[1] is p0


def test_default_model_plan_call_count_is_unchanged():
    model = build_model(load_config().model, 668, 2, seed=42)
    model.compute_dtype = "bf16"
    model.cuda()
    plan = model.engine()._plan(64, 100, True, True)
    fwd, bwd = [fn.__name__ for fn, _, _ in plan["fwd"]], [fn.__name__ for _, seg in plan["bwd"] for fn, _, _ in seg]
    assert (len(fwd), len(bwd)) == (81, 222) and not any(n.endswith("_seg") for n in fwd + bwd)
