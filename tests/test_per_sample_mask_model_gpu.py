"""Per-sample token masking (MultiModal.per_sample_mask) on the MI355X, whole models.  The fp32 engine against the
reference with every sample's own masked tokens zeroed (tests/golden/per_sample_mask_*, scripts/make_per_sample_mask_goldens.py):
forward / backward of every case, eval-mode forwards, the 50-step curve; batch independence - a sample's predictions are those of the
sample run alone, which the switch-off model does not give; the bit-exact equivalences with the switch-off model where the two modes are
one model; the bf16 engine against the fp32 engine at hidden 256; a dropout-on step under hipGraph replay across batches with different
masks; live rows on against off; a frozen encoder, accumulation and a segmented batch; the switch-off plan."""
import contextlib
import math
from unittest import mock

import numpy as np
import pytest
import torch

import mod_segments as S
import model_checks as MC
import per_sample_mask as P
import plan_sig
from conftest import load_json, load_npz
from helpers import build_model, load_config, model_config, tiny_config
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("per_sample_mask_fwd_bwd.npz")
    return _Z


def case_model(case, seed=P.MODEL_SEED, on=True, **kw):
    sw = P.switches(case)
    cfg = tiny_config(max_F=P.TINY["max_F"], sep=bool(sw.get("sep")), causal=bool(sw.get("causal")), **kw)
    return build_model(cfg, P.TINY["n_ap"], P.TINY["n_beh"], seed=seed, **({"per_sample_mask": True} if on else {}))


@contextlib.contextmanager
def case_batches(case):
    """model_checks' bodies on the case's mod_dicts (tests/per_sample_mask.py): the case's batch and its explicit masks."""
    with mock.patch.object(MC, "fixture_batch", lambda z, prefix="batch/": case), \
            mock.patch.object(O, "make_mod_dict", lambda c, objective: P.mod_dict(c, objective)):
        yield


def _names(plan):
    return [fn.__name__ for fn, _, _ in plan["fwd"]], [fn.__name__ for _, seg in (plan["bwd"] or []) for fn, _, _ in seg]


def test_fixture_batches_are_the_shared_recipe():
    z, meta = fixture()
    assert set(meta["switches"]) == set(P.CASES) and meta["full_grad_cases"] == list(P.FULL_GRAD_CASES)
    for case in list(P.CASES) + [P.FILTER["case"]]:
        for mod, d in P.case_batch(case).items():
            for k, v in d.items():
                np.testing.assert_array_equal(v.numpy(), z[f"batch/{case}/{mod}/{k}"])
    m = z["DRAWN/token_masking/mask/ap"]
    assert any((m[b] != m[0]).any() for b in (1, 2)), "the drawn masks differ between samples"


# ---------------------------------------------------------------------------------------------- fp32 against the reference
CASE_OBJECTIVES = [(c, o) for c, sw in P.CASES.items() for o in sw.get("objectives", ("token_masking",))]


@pytest.mark.parametrize("case,objective", CASE_OBJECTIVES)
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """model_checks.check_fixture_case, bounds and all (loss, counts and token masks exact, predictions, every gradient norm), with every
    gradient tensor of PAD / token_masking; the plan is uniform or segmented as the batch is and runs the _rows entry points."""
    z, meta = fixture()
    model = case_model(case, seed=meta["model_seed"])
    with case_batches(case):
        stored = MC.check_fixture_case(model, z, meta, case, objective)
    assert len(stored) == (len(meta["params"][case]) if (case, objective) == ("PAD", "token_masking") else 0)
    T = P.CASES[case]["T"]
    plan = model._engine._last
    fwd, bwd = _names(plan)
    assert plan["T"] == (T if case == "SEG" else T[0])
    assert fwd.count("mmfm_mask_prep_rows") == 1 and fwd.count("mmfm_stitch_fwd_rows") == 4 and bwd.count("mmfm_stitch_bwd_rows") == 4
    assert not [n for n in fwd + bwd if n in ("mmfm_mask_prep", "mmfm_mask_prep_seg") or (n.startswith("mmfm_stitch_") and not n.endswith("_rows"))]
    assert "keep0" not in plan["b"] and tuple(plan["b"]["keep"].shape) == (3, sum(T)) and tuple(plan["b"]["keep_any"].shape) == (sum(T),)


def test_switch_off_model_misses_the_fixture():
    """The fixture discriminates: today's model is off the per-sample reference on S0_FULL by far more than the parity bound."""
    z, _ = fixture()
    model = case_model("S0_FULL", on=False).cuda().train()
    out = model(MC.to_dev(P.mod_dict("S0_FULL", "token_masking")))
    assert abs(out.loss.item() / float(z["S0_FULL/token_masking/loss"]) - 1) > 1e-3


@pytest.mark.parametrize("case", P.EVAL_CASES)
def test_eval_mode_forward_vs_reference_fixture(case):
    """The forward-only plan (eval_epoch, co_smoothing_core) runs per-sample masks with no code of its own."""
    z, _ = fixture()
    model = case_model(case).cuda().eval()
    with torch.no_grad():
        out = model(MC.to_dev(P.mod_dict(case, "token_masking")))
    p = f"{case}/eval"
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=2e-5)
    for m in P.MODS:
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    plan = model._engine._last
    assert plan["bwd"] is None and _names(plan)[0].count("mmfm_stitch_fwd_rows") == 4


def test_modal_filter_vs_reference_fixture():
    """The encoder over spikes, the decoder over behaviour: each side stitches under its own modality's per-sample masks (two mask
    launches, two buffer sets)."""
    z, meta = fixture()
    f = P.FILTER
    case, p = f["case"], f"{f['case']}/token_masking"
    model = build_model(tiny_config(max_F=P.TINY["max_F"]), P.TINY["n_ap"], P.TINY["n_beh"], seed=meta["model_seed"],
                        modal_filter=dict(input=f["input"], output=f["output"]), per_sample_mask=True)
    model.cuda().train()
    torch.manual_seed(11)
    md = MC.to_dev(P.mod_dict(case, "token_masking"))
    out = model(md)
    out.loss.backward()
    assert list(out.mod_loss) == f["output"]
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=2e-5)
    for m in f["output"]:
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    for m in P.MODS:
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"{p}/mask/{m}"])
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names and list(model.state_dict()) == [k for k, _ in meta["state"][case]]
    for k, gn in zip(names, z[f"{p}/grad_norm"]):
        assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=5e-3, abs=1e-8), k
    plan = model._engine._last
    fwd, bwd = _names(plan)
    assert fwd.count("mmfm_mask_prep_rows") == 2 and fwd.count("mmfm_stitch_fwd_rows") == 2 and bwd.count("mmfm_stitch_bwd_rows") == 2
    assert {"keep", "keep_any", "dec/keep", "dec/keep_any"} <= set(plan["b"])
    assert torch.equal(plan["b"]["keep"].cpu() != 0, md["ap"]["inputs_mask"].cpu() != 1)
    assert torch.equal(plan["b"]["dec/keep"].cpu() != 0, md["behavior"]["inputs_mask"].cpu() != 1)


def test_loss_curve_tiny_50_steps_vs_reference_fixture():
    g = load_json("per_sample_mask_curve.json")
    assert {k: g[k] for k in ("B", "T", "n_ap", "n_beh")} == {k: P.CURVE[k] for k in ("B", "T", "n_ap", "n_beh")}
    model = build_model(tiny_config(max_F=P.TINY["max_F"]), g["n_ap"], g["n_beh"], seed=g["model_seed"], per_sample_mask=True)
    losses = MC.run_curve(model.cuda(), 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- batch independence
B4 = dict(T=(8, 8), pad=((0, 2, 0, 1), (0, 2, 0, 1)),
          masks=(((0, 5), (1, 2, 3), (), (4, 6, 7)), ((7,), (), (0, 1, 2, 3), (2, 5))))


def b4_mod_dict(rows):
    """The B = 4 batch's samples `rows`, in that order, with their explicit masks, as an eval-mode mod_dict."""
    batch = S.ragged_batch(4, B4["T"], P.TINY["n_ap"], P.TINY["n_beh"], 21, "arange", B4["pad"], P.TINY["max_F"])
    em = P.explicit_masks(batch, B4["masks"])
    idx = torch.tensor(rows)
    md = S.make_mod_dict({m: {k: v[idx] for k, v in d.items()} for m, d in batch.items()}, "token_masking")
    for m in P.MODS:
        md[m]["eval_mask"] = em[m][idx]
    return MC.to_dev(md)


def preds(model, rows):
    with torch.no_grad():
        out = model(b4_mod_dict(rows))
    return {m: out.mod_preds[m].cpu().double() for m in P.MODS}


def gap(a, b):
    """max |a - b| in units of the project's prediction bound (rtol 1e-4, atol 2e-5): <= 1 meets it."""
    return float(((a - b).abs() / (2e-5 + 1e-4 * b.abs())).max())


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (2, 0, 3, 1)], ids=["batch", "permuted"])
def test_a_sample_is_predicted_as_if_alone(order):
    """fp32, eval mode, explicit per-sample masks, B = 4: each sample's predictions equal those of the same sample run alone at B = 1
    within 1e-4 - also under a permutation of the batch - and today's model does not meet that bound on the same batch."""
    on, off = (build_model(tiny_config(max_F=P.TINY["max_F"]), P.TINY["n_ap"], P.TINY["n_beh"], seed=7, **kw).cuda().eval()
               for kw in ({"per_sample_mask": True}, {}))
    alone = {b: preds(on, [b]) for b in range(4)}
    for b in range(4):          # at B = 1 the two modes are one model
        a0 = preds(off, [b])
        assert all(torch.equal(alone[b][m], a0[m]) for m in P.MODS)
    batch_on, batch_off = preds(on, list(order)), preds(off, list(order))
    worst_on = max(gap(batch_on[m][i:i + 1], alone[b][m]) for i, b in enumerate(order) for m in P.MODS)
    worst_off = max(gap(batch_off[m][i:i + 1], alone[b][m]) for i, b in enumerate(order) for m in P.MODS)
    print("per-sample", worst_on, "sample-0", worst_off)
    assert worst_on <= 1.0
    assert worst_off > 1.0, "the batch does not discriminate"


# ---------------------------------------------------------------------------------------------- where the two modes are one model
def train_step(model, md, dtype, seed=5):
    model.compute_dtype, model.engine_seed = dtype, 77
    model.cuda().train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    out = model(MC.to_dev(md))
    out.loss.backward()
    torch.cuda.synchronize()
    return out, {k: p.grad.clone() for k, p in model.named_parameters()}


def same_step(a, b):
    (oa, ga), (ob, gb) = a, b
    assert oa.loss.item() == ob.loss.item() and math.isfinite(oa.loss.item())
    for m in ob.mod_preds:
        assert torch.equal(oa.mod_preds[m], ob.mod_preds[m]), m
    for k in gb:
        assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_single_sample_batch_is_todays_model_bit_for_bit(dtype):
    """B = 1, token_masking with drawn masks, dropout on: switch on equals switch off - loss, predictions and every gradient."""
    res = []
    for on in (True, False):
        model = build_model(tiny_config(dropout=0.2, emb_dropout=0.1), 12, 2, seed=7, **({"per_sample_mask": True} if on else {}))
        res.append(train_step(model, O.make_mod_dict(O.synth_batch(1, 12, 12, 2, seed=3), "token_masking"), dtype))
        assert ("mmfm_stitch_fwd_rows" in _names(model._engine._last)[0]) == on
    same_step(*res)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_shared_mask_batch_is_todays_model_bit_for_bit(monkeypatch, dtype):
    """An unpadded `encoding` step (every sample carries sample 0's mask), live rows forced on (the bf16 engine then compacts: every spike
    bin dead, every behaviour bin live): switch on equals switch off."""
    monkeypatch.setenv("MMFM_LIVE_ROWS", "1")
    res = []
    for on in (True, False):
        model = build_model(tiny_config(dropout=0.2, emb_dropout=0.1), 12, 2, seed=7, **({"per_sample_mask": True} if on else {}))
        res.append(train_step(model, O.make_mod_dict(O.synth_batch(4, 12, 12, 2, seed=3), "encoding"), dtype))
        fwd = _names(model._engine._last)[0]
        assert ("mmfm_stitch_fwd_rows" in fwd) == on and ("mmfm_gemm_live" in fwd) == (dtype == "bf16")
    same_step(*res)


# ---------------------------------------------------------------------------------------------- bf16 at hidden 256
WIDE = dict(B=4, n_ap=40, n_beh=2, max_F=40)


def wide_step(dtype, T):
    mc = model_config(heads=8, n_enc=2, n_dec=2, max_F=WIDE["max_F"], sep=True, causal=True, dropout=0.0, emb_dropout=0.0)
    model = build_model(mc, WIDE["n_ap"], WIDE["n_beh"], seed=3, per_sample_mask=True)
    batch = S.ragged_batch(WIDE["B"], (T, T), WIDE["n_ap"], WIDE["n_beh"], 6)
    out, grads = train_step(model, S.make_mod_dict(batch, "token_masking"), dtype)
    return model, out, grads


def test_bf16_step_at_hidden_256_vs_fp32_engine():
    """Hidden 256 / 8 heads / inter_size 512, 2 + 2 layers, sep + causal decoder masks, dropout 0, drawn masks: one bf16 step against the
    fp32 engine on the same weights and masks at model_checks.check_bf16's bounds, unchanged (tests/test_context_window_model_gpu.py)."""
    m32, o32, g32 = wide_step("fp32", 20)
    m16, o16, g16 = wide_step("bf16", 20)
    keep = m16._engine._last["b"]["keep"]
    assert torch.equal(keep, m32._engine._last["b"]["keep"]) and not torch.equal(keep[0], keep[1])
    assert [int(o16.mod_n_examples[m]) for m in P.MODS] == [int(o32.mod_n_examples[m]) for m in P.MODS]
    MC.check_bf16(MC.bf16_stats(o16, g16, dict(loss=o32.loss.double()), {k: v.double() for k, v in g32.items()}), "bf16 per-sample masks vs fp32 engine")


# ---------------------------------------------------------------------------------------------- dropout and hipGraph replay
def test_dropout_step_under_graph_replay_across_batches_with_different_masks(monkeypatch):
    """bf16, dropout on, four steps over two batches with different explicit masks (A, B, A, B): eager, capture, replay, replay.  The masks
    are data in static buffers: every loss and the last step's gradients equal those of MMFM_GRAPH=0 bit for bit, and after each replay
    the plan's keep buffer holds that step's masks."""
    seq = ["S0_OPEN", "BIN_ALL", "S0_OPEN", "BIN_ALL"]
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MMFM_GRAPH", mode)
        model = case_model("S0_OPEN", dropout=0.2, emb_dropout=0.1)
        losses = []
        for case in seq:
            md = P.mod_dict(case, "token_masking")
            out, grads = train_step(model, md, "bf16")
            losses.append(out.loss.item())
            plan = model._engine._last
            want = torch.cat([md[m]["inputs_mask"] for m in P.MODS], 1) != 1
            assert torch.equal(plan["b"]["keep"] != 0, want), case
            assert torch.equal(plan["b"]["keep_any"] != 0, want.any(0)), case
        assert (set(plan["graphs"]) == {"fwd", "bwd"}) == (mode == "1") and plan["runs"]["fwd"] == len(seq)
        res[mode] = (losses, grads)
    assert res["0"][0] == res["1"][0] and all(math.isfinite(x) for x in res["0"][0]) and len(set(res["0"][0])) == len(seq)
    for k, g in res["0"][1].items():
        assert torch.equal(res["1"][1][k], g), k


# ---------------------------------------------------------------------------------------------- live rows
def test_live_rows_on_against_off(monkeypatch):
    """bf16, dropout on, BIN_ALL's masks at B = 3: spike bin 3 is dead in every sample (it leaves the tokeniser chains), bins 0 and 6 are
    masked in some (they stay, and their masked samples' compact d_tok rows are zeros).  Live rows forced on against off: loss,
    predictions and every gradient that does not pass through a tokeniser's dY^T.X bit for bit; the tokenisers' weight gradients sum
    the same terms in other groups, so they are held to model_checks.check_bf16's bounds (tests/test_live_rows_model_gpu.py)."""
    res = {}
    for live in ("1", "0"):
        monkeypatch.setenv("MMFM_LIVE_ROWS", live)
        model = case_model("BIN_ALL", dropout=0.2, emb_dropout=0.1)
        res[live] = train_step(model, P.mod_dict("BIN_ALL", "token_masking"), "bf16")
        plan = model._engine._last
        fwd = _names(plan)[0]
        assert ("mmfm_gemm_live" in fwd) == ("mmfm_live_bins" in fwd) == (live == "1")
        if live == "1":
            rec = plan["b"]["live"].cpu()
            assert rec[0, 0].item() == 7 and rec[1, 0].item() == 8, "spikes: one dead bin; behaviour: none, though bins are masked in some samples"
    (on, gon), (off, goff) = res["1"], res["0"]
    assert on.loss.item() == off.loss.item() and math.isfinite(on.loss.item())
    for m in off.mod_preds:
        assert torch.equal(on.mod_preds[m], off.mod_preds[m]), m
    regrouped = (".embedder.token_embed.", ".embedder.projection.")
    for k in goff:
        assert bool(torch.isfinite(gon[k]).all()), k
        if not any(r in k for r in regrouped):
            assert torch.equal(gon[k], goff[k]), f"gradient {k}"
    MC.check_bf16(MC.bf16_stats(on, gon, dict(loss=off.loss.double()), {k: v.double() for k, v in goff.items()}), "live vs full rows under per-sample masks")


# ---------------------------------------------------------------------------------------------- compositions
def test_frozen_encoder_accumulation_and_a_segmented_batch():
    """A frozen encoder prunes the backward like any other plan's; a two-batch accumulation gives the sum of the two batches' gradients
    bit for bit; both on the segmented batch SEG and on the uniform PAD."""
    for case in ("SEG", "PAD"):
        model = case_model(case).cuda().train()
        md = lambda seed: MC.to_dev(P.mod_dict(case, "token_masking", seed))

        def grads(seeds):
            model.zero_grad(set_to_none=True)
            for s in seeds:
                torch.manual_seed(11)
                model(md(s)).loss.backward()
            torch.cuda.synchronize()
            return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        g3, g4, g34 = grads([3]), grads([4]), grads([3, 4])
        for k in g34:
            assert torch.equal(g34[k], g3[k] + g4[k]), k
        full = _names(model._engine._last)[1]
        for k, p in model.named_parameters():
            if k.startswith(("encoder.", "encoder_embeddings.", "encoder_norm.")):
                p.requires_grad_(False)
        gf = grads([3])
        eng = model._engine
        pruned = _names(eng._last)[1]
        assert len(pruned) < len(full) and pruned.count("mmfm_stitch_bwd_rows") <= full.count("mmfm_stitch_bwd_rows")
        T = P.CASES[case]["T"]
        assert eng.plan_key(3, T if case == "SEG" else T[0], True, True, eng.freeze_pattern()) in eng.plans
        assert all(key[-1] == ("rows",) for key in eng.plans)
        for k, g in gf.items():
            np.testing.assert_allclose(g.cpu().numpy(), g3[k].cpu().numpy(), rtol=1e-5, atol=1e-8, err_msg=k)


# ---------------------------------------------------------------------------------------------- the plan
def default_plan(on, B=64, T=100):
    model = build_model(load_config().model, 668, 2, seed=42, **({"per_sample_mask": True} if on else {}))
    model.compute_dtype = "bf16"
    model.cuda()
    eng = model.engine()
    return model, eng, eng._plan(B, T, True, True)


def test_plan_is_todays_with_the_switch_off_and_moves_with_the_switch():
    """Switch off: the default model's plan under today's key.  Switch on: the same calls but for the mask launch, the stitch launches
    and the source of the live-bin records.  Moving the switch after the engine was built gives another engine."""
    m0, e0, p0 = default_plan(False)
    assert list(e0.plans) == [(64, 100, True, True)] and e0.cfg.per_sample_mask is False and "keep0" in p0["b"] and "keep" not in p0["b"]
    f0, b0 = _names(p0)
    assert not [n for n in f0 + b0 if n.endswith("_rows")]
    m1, e1, p1 = default_plan(True)
    assert list(e1.plans) == [(64, 100, True, True, None, None, ("rows",))] and e1.cfg.per_sample_mask is True and e1.cfg != e0.cfg
    f1, b1 = _names(p1)
    swap = {"mmfm_mask_prep": "mmfm_mask_prep_rows", "mmfm_stitch_fwd": "mmfm_stitch_fwd_rows", "mmfm_stitch_fwd_live": "mmfm_stitch_fwd_rows",
            "mmfm_stitch_bwd": "mmfm_stitch_bwd_rows", "mmfm_stitch_bwd_live": "mmfm_stitch_bwd_rows"}
    assert [swap.get(n, n) for n in f0] == f1 and [swap.get(n, n) for n in b0] == b1
    s0, s1 = (plan_sig.plan_signature(e, p, full=True) for e, p in ((e0, p0), (e1, p1)))
    assert list(s0) == list(s1)
    m1.per_sample_mask = False
    e2 = m1.engine()
    assert e2 is not e1 and e2.cfg == e0.cfg
    m1.per_sample_mask = True
    assert m1.engine() is not e2 and m1.engine().cfg == e1.cfg
