"""context.forward / context.backward honoured (MultiModal.context_mask) on the MI355X, whole models.  The fp32 engine
against the reference with its encoder mask windowed over time stamps (tests/golden/context_window_*,
scripts/make_context_window_goldens.py): forward / backward of every case and objective, eval-mode forwards, the 50-step curve; the bf16
engine against the fp32 engine at the default widths; a dropout-on step under hipGraph replay; the plan's calls with the switch off, on
without a window and on with one; a frozen trunk and two-batch accumulation under the window; a modal_filter model against the
reference; the live-row tokeniser path under the window."""
import contextlib
import math
from unittest import mock

import numpy as np
import pytest
import torch

import context_window as W
import mod_segments as S
import model_checks as MC
import plan_sig
from conftest import load_json, load_npz
from helpers import build_model, load_config, model_config, tiny_config
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("context_window_fwd_bwd.npz")
    return _Z


def with_ctx(cfg, ctx):
    cfg["context"]["forward"], cfg["context"]["backward"] = ctx
    return cfg


def case_model(case, seed=W.MODEL_SEED):
    return build_model(with_ctx(tiny_config(max_F=W.TINY["max_F"]), W.CASES[case]["ctx"]), W.TINY["n_ap"], W.TINY["n_beh"], seed=seed,
                       context_mask=True)


@contextlib.contextmanager
def case_batches(case):
    """model_checks' bodies on the case's batches (tests/context_window.py), per-modality mod_dicts."""
    with mock.patch.object(MC, "fixture_batch", lambda z, prefix="batch/": W.case_batch(case)), \
            mock.patch.object(O, "make_mod_dict", S.make_mod_dict):
        yield


def _names(plan):
    return [fn.__name__ for fn, _, _ in plan["fwd"]], [fn.__name__ for _, seg in (plan["bwd"] or []) for fn, _, _ in seg]


def test_fixture_batches_are_the_shared_recipe():
    z, meta = fixture()
    assert {k: tuple(v["ctx"]) for k, v in meta["switches"].items()} == {k: v["ctx"] for k, v in W.CASES.items()}
    for case in list(W.CASES) + [W.FILTER["case"]]:
        for mod, d in W.case_batch(case).items():
            for k, v in d.items():
                np.testing.assert_array_equal(v.numpy(), z[f"batch/{case}/{mod}/{k}"])


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("case", list(W.CASES))
@pytest.mark.parametrize("objective", W.OBJECTIVES)
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """model_checks.check_fixture_case, bounds and all (loss, counts and token masks exact, predictions, every gradient norm), with every
    gradient tensor of SEG / token_masking; the plan is uniform or segmented as the batch is and carries the window calls."""
    z, meta = fixture()
    model = case_model(case, seed=meta["model_seed"])
    with case_batches(case):
        stored = MC.check_fixture_case(model, z, meta, case, objective)
    assert len(stored) == (len(meta["params"][case]) if (case, objective) == ("SEG", "token_masking") else 0)
    T = W.CASES[case]["T"]
    plan = model._engine._last
    fwd, bwd = _names(plan)
    assert plan["T"] == (T if case == "SEG" else T[0])
    assert fwd.count("mmfm_attn_pos_prep") == 1 and fwd.count("mmfm_attn_win_fwd") == 2 and fwd.count("mmfm_attn_fwd") == 1
    assert bwd.count("mmfm_attn_win_bwd") == 2 and bwd.count("mmfm_attn_bwd") == 1 and "mmfm_attn_pos_prep" not in bwd


@pytest.mark.parametrize("case", W.EVAL_CASES)
def test_eval_mode_forward_vs_reference_fixture(case):
    """The forward-only plan runs windowed with no code of its own."""
    z, _ = fixture()
    model = case_model(case).cuda().eval()
    with torch.no_grad():
        out = model(MC.to_dev(S.make_mod_dict(W.case_batch(case), "encoding")))
    p = f"{case}/eval"
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=2e-5)
    for m in W.MODS:
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    plan = model._engine._last
    fwd, bwd = _names(plan)
    assert plan["bwd"] is None and fwd.count("mmfm_attn_win_fwd") == 2 and fwd.count("mmfm_attn_pos_prep") == 1


def curve_model(g):
    return build_model(with_ctx(tiny_config(max_F=W.TINY["max_F"]), tuple(g["ctx"])), g["n_ap"], g["n_beh"], seed=g["model_seed"], context_mask=True)


def test_loss_curve_tiny_50_steps_vs_reference_fixture():
    g = load_json("context_window_curve.json")
    assert tuple(g["ctx"]) == W.CURVE["ctx"]
    losses = MC.run_curve(curve_model(g).cuda(), 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- bf16 at the default widths
WIDE = dict(B=4, n_ap=40, n_beh=2, max_F=40)


def wide_batch(T):
    """T = (37, 23): the ragged batch of test_mod_segments_model_gpu.py (behaviour's stamps reversed and shifted, padding); T = 20: shared bins."""
    if isinstance(T, tuple):
        return S.ragged_batch(WIDE["B"], T, WIDE["n_ap"], WIDE["n_beh"], 6, "shifted", ((5, 0, 11, 0), (0, 7, 0, 2)), WIDE["max_F"])
    return S.ragged_batch(WIDE["B"], (T, T), WIDE["n_ap"], WIDE["n_beh"], 6)


def wide_step(dtype, T, ctx, heads=8, dropout=0.0, model=None, objective="token_masking"):
    if model is None:
        mc = with_ctx(model_config(heads=heads, n_enc=2, n_dec=2, max_F=WIDE["max_F"], sep=True, causal=True, dropout=dropout,
                                   emb_dropout=dropout / 2), ctx)
        model = build_model(mc, WIDE["n_ap"], WIDE["n_beh"], seed=3, context_mask=True)
        model.compute_dtype, model.engine_seed = dtype, 77
        model.cuda().train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    out = model(MC.to_dev(S.make_mod_dict(wide_batch(T), objective)))
    out.loss.backward()
    torch.cuda.synchronize()
    return model, out


@pytest.mark.parametrize("T", [(37, 23), 20], ids=["ragged", "uniform"])
@pytest.mark.parametrize("ctx", [(0, 5), (3, 3)], ids=["causal5", "pm3"])
def test_bf16_step_at_default_widths_vs_fp32_engine(T, ctx):
    """Hidden 256 / 8 heads / inter_size 512, 2 + 2 layers, sep + causal decoder masks, dropout 0: one bf16 step against the fp32 engine on
    the same weights and masks at model_checks.check_bf16's bounds, unchanged.  Uniform T = 20 (L = 40): the windowed sites run the WIN
    forms of the keep-bit dh-32 kernels; T = (37, 23) (L = 60, not a multiple of 8): the general bf16 kernels."""
    m32, o32 = wide_step("fp32", T, ctx)
    m16, o16 = wide_step("bf16", T, ctx)
    assert m16._engine._last["T"] == T and m16._engine.cfg.context == ctx
    assert [int(o16.mod_n_examples[m]) for m in W.MODS] == [int(o32.mod_n_examples[m]) for m in W.MODS]
    named = {k: p.grad for k, p in m16.named_parameters()}
    grads = {k: p.grad.double() for k, p in m32.named_parameters()}
    MC.check_bf16(MC.bf16_stats(o16, named, dict(loss=o32.loss.double()), grads), f"bf16 window {ctx} T {T} vs fp32 engine")


@pytest.mark.parametrize("T,family", [((40, 24), "KEEPBIT_DH32"), ((37, 23), "BF16")], ids=["keepbit", "general"])
def test_bf16_dropout_step_under_graph_replay_is_a_function_of_the_rng_state(monkeypatch, T, family):
    """Dropout 0.4 under the window, hipGraph replay on: two fresh models run three steps each (eager, capture, replay) from the same RNG
    state - every loss and every gradient of the replayed step bit for bit, and new masks from step to step.  T = (40, 24), L = 64: the
    windowed sites run the DROP WIN instantiations of the keep-bit dh-32 kernels; T = (37, 23), L = 60: the general bf16 kernels, which
    hash.  The family of every windowed site is asked of the library, in both directions."""
    from multi_modal_foundation_model_amd import _lib as Lb, ops as K
    monkeypatch.setenv("MMFM_GRAPH", "1")
    runs = []
    for _ in range(2):
        model, losses = None, []
        for _step in range(3):
            model, out = wide_step("bf16", T, (0, 5), dropout=0.4, model=model)
            losses.append(out.loss.item())
        plan = model._engine._last
        assert set(plan["graphs"]) == {"fwd", "bwd"}
        runs.append((losses, {k: p.grad.clone() for k, p in model.named_parameters()}, model))
    (la, ga, a), (lb, gb, _) = runs
    assert la == lb and all(math.isfinite(x) for x in la) and len(set(la)) == 3
    assert all(torch.equal(ga[k], gb[k]) for k in ga)
    sites = {s["key"]: s for s in a._engine.dropout_sites(WIDE["B"], T) if s["kind"] == "attn"}
    assert sites and all(s["keepbits"] is not None for s in sites.values()), "dh 32: windowed sites keep their keep-bit workspace"
    plan = a._engine._last
    entries = [(fn.__name__, keep) for fn, _, keep in plan["fwd"]] + [(fn.__name__, keep) for _, seg in plan["bwd"] for fn, _, keep in seg]
    fams = [K.attn_win_family(keep[0], keep[1], name.endswith("_bwd")) & Lb.ATTN_FAMILY_MASK for name, keep in entries if name.startswith("mmfm_attn_win_")]
    assert len(fams) == 8 and set(fams) == {getattr(Lb, "ATTN_FAMILY_" + family)}


# ---------------------------------------------------------------------------------------------- the plan
def default_plan(ctx, on, B=64, T=100):
    model = build_model(with_ctx(load_config().model, ctx), 668, 2, seed=42, **({"context_mask": True} if on else {}))
    model.compute_dtype = "bf16"
    model.cuda()
    eng = model.engine()
    return eng, eng._plan(B, T, True, True)


def test_plan_is_todays_with_the_switch_off_or_without_a_window():
    """Switch off with context (0, 5), and switch on with (-1, -1): the default model's plan under its key, call for call and argument for
    argument (tests/plan_sig.py); switch on with (0, 5): the same calls except the enc*/sa and dec*/xa attention entries - now
    mmfm_attn_win_* on the same descriptors - plus the one mmfm_attn_pos_prep."""
    e0, p0 = default_plan((-1, -1), False)
    sig = lambda eng, plan: plan_sig.plan_signature(eng, plan, full=True)
    s0 = sig(e0, p0)
    for ctx, on in (((0, 5), False), ((-1, -1), True)):
        e1, p1 = default_plan(ctx, on)
        assert e1.cfg == e0.cfg and list(e1.plans) == [(64, 100, True, True)]
        assert sig(e1, p1) == s0
    e2, p2 = default_plan((0, 5), True)
    assert list(e2.plans) == [(64, 100, True, True, None, None, ("window", -5, 0))]
    f0, b0 = _names(p0)
    f2, b2 = _names(p2)
    n_enc, n_dec = e0.cfg.n_enc, e0.cfg.n_dec
    assert f2.count("mmfm_attn_pos_prep") == 1 and f2.count("mmfm_attn_win_fwd") == n_enc + n_dec and f2.count("mmfm_attn_fwd") == n_dec
    assert b2.count("mmfm_attn_win_bwd") == n_enc + n_dec and b2.count("mmfm_attn_bwd") == n_dec
    s2 = sig(e2, p2)
    assert list(s2) == list(s0)
    for unit in s0:
        r0, r2 = s0[unit]["records"], [r for r in s2[unit]["records"] if r["fn"] != "mmfm_attn_pos_prep"]
        assert len(r0) == len(r2), unit
        for a, b in zip(r0, r2):
            if b["fn"].startswith("mmfm_attn_win_"):
                assert a["fn"] == b["fn"].replace("_win_", "_") and b["keep"][1]["lo"] == -5 and b["keep"][1]["hi"] == 0
                assert b["keep"][0] == a["keep"][0] and b["keep"][0]["keepbits"] is not None     # the descriptor, keep-bit workspace included
            else:
                assert a == b, (unit, a["fn"])


def test_frozen_trunk_and_accumulation_under_the_window():
    """A frozen encoder prunes the windowed plan's backward like any other (the encoder's attention backward leaves with its segment), and a
    two-batch accumulation gives the sum of the two batches' gradients."""
    model = case_model("W11").cuda().train()
    md = lambda seed: MC.to_dev(S.make_mod_dict(W.case_batch("W11", seed), "token_masking"))

    def grads(seeds):
        model.zero_grad(set_to_none=True)
        for s in seeds:
            torch.manual_seed(11)
            model(md(s)).loss.backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    g3, g4, g34 = grads([3]), grads([4]), grads([3, 4])
    for k in g34:
        assert torch.equal(g34[k], g3[k] + g4[k]), k              # the engine's stash / add is torch's rule, bit for bit
    full = [fn.__name__ for _, seg in model._engine._last["bwd"] for fn, _, _ in seg]
    for k, p in model.named_parameters():
        if k.startswith(("encoder.", "encoder_embeddings.", "encoder_norm.")):
            p.requires_grad_(False)
    gf = grads([3])
    plan = model._engine._last
    pruned = [fn.__name__ for _, seg in plan["bwd"] for fn, _, _ in seg]
    assert len(pruned) < len(full) and pruned.count("mmfm_attn_win_bwd") <= full.count("mmfm_attn_win_bwd")
    assert model._engine.plan_key(3, 8, True, True, model._engine.freeze_pattern()) in model._engine.plans
    for k, g in gf.items():
        np.testing.assert_allclose(g.cpu().numpy(), g3[k].cpu().numpy(), rtol=1e-5, atol=1e-8, err_msg=k)


# ---------------------------------------------------------------------------------------------- modal_filter, live rows
@pytest.mark.parametrize("objective", W.FILTER["objectives"])
def test_modal_filter_under_the_window_vs_reference_fixture(objective):
    """The encoder over spikes, the decoder over behaviour whose stamps differ from the spikes': cross-attention windows decoder query i by
    the ENCODER's stamp i on both sides, as upstream's xa_mask = encoder_attn_mask does.  Loss, count (exact), token masks (exact),
    predictions, every gradient norm and, for token_masking, every gradient tensor against the reference within the bounds of
    model_checks.check_fixture_case."""
    z, meta = fixture()
    f = W.FILTER
    case, p = f["case"], f"{f['case']}/{objective}"
    assert meta["modal_filter"]["input"] == f["input"] and meta["modal_filter"]["output"] == f["output"] and tuple(meta["modal_filter"]["ctx"]) == f["ctx"]
    model = build_model(with_ctx(tiny_config(max_F=W.TINY["max_F"]), f["ctx"]), W.TINY["n_ap"], W.TINY["n_beh"], seed=meta["model_seed"],
                        modal_filter=dict(input=f["input"], output=f["output"]), context_mask=True)
    model.cuda().train()
    torch.manual_seed(11)
    md = MC.to_dev(S.make_mod_dict(W.case_batch(case), objective))
    out = model(md)
    out.loss.backward()
    assert list(out.mod_loss) == f["output"]
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=2e-5)
    for m in f["output"]:
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    for m in W.MODS:
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"{p}/mask/{m}"])
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names and list(model.state_dict()) == [k for k, _ in meta["state"][case]]
    for k, gn in zip(names, z[f"{p}/grad_norm"]):
        assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=5e-3, abs=1e-8), k
    stored = MC.check_stored_grads(named, z, p, names)
    assert len(stored) == (len(names) if objective == W.FULL_GRAD else 0)
    plan = model._engine._last
    fwd, bwd = _names(plan)
    assert plan["T"] == f["T"] and fwd.count("mmfm_attn_pos_prep") == 1 and fwd.count("mmfm_attn_win_fwd") == 2 and bwd.count("mmfm_attn_win_bwd") == 2
    # the one pos buffer holds the ENCODER's stamps (the spikes'), not the decoder's
    want = W.case_batch(case)["ap"]["ts"].to(torch.int32)
    assert torch.equal(plan["b"]["attn/pos"].cpu(), want) and not torch.equal(want, W.case_batch(case)["behavior"]["ts"].to(torch.int32))


def test_live_rows_under_the_window(monkeypatch):
    """One bf16 training step with the live-row tokeniser path forced on (MMFM_LIVE_ROWS=1) against the same step with it off, under a
    window, uniform plan, `encoding` (every spike bin dead, every behaviour bin live): the loss, the predictions and every gradient bit
    for bit, as tests/test_live_rows_model_gpu.py asks of the dense model; both plans carry the window calls."""
    res = {}
    for live in ("1", "0"):
        monkeypatch.setenv("MMFM_LIVE_ROWS", live)
        model = build_model(with_ctx(tiny_config(dropout=0.2, emb_dropout=0.1), (1, 2)), 12, 2, seed=7, context_mask=True)
        model.compute_dtype, model.engine_seed = "bf16", 77
        model.cuda().train()
        torch.manual_seed(5)
        out = model(MC.to_dev(O.make_mod_dict(O.synth_batch(4, 12, 12, 2, seed=3, pad=[0, 0, 2, 0]), "encoding")))
        out.loss.backward()
        torch.cuda.synchronize()
        fwd, bwd = _names(model._engine._last)
        assert ("mmfm_gemm_live" in fwd) == ("mmfm_live_bins" in fwd) == (live == "1")
        assert fwd.count("mmfm_attn_win_fwd") == 2 and fwd.count("mmfm_attn_pos_prep") == 1 and bwd.count("mmfm_attn_win_bwd") == 2
        res[live] = (out, {k: p.grad.clone() for k, p in model.named_parameters()})
    (on, gon), (off, goff) = res["1"], res["0"]
    assert on.loss.item() == off.loss.item() and math.isfinite(on.loss.item())
    for m in off.mod_preds:
        assert torch.equal(on.mod_preds[m], off.mod_preds[m]), m
    for k in goff:
        assert torch.equal(gon[k], goff[k]), k
