"""A model with per-session read-in / read-out layers (use_session) on the engine: the fp32 step against the reference-built
fixtures of scripts/make_session_stitch_goldens.py, both loss curves with the bytes of absent sessions kept, pad independence, a bf16
step against the fp32 engine, a dropout-on step, graph replay across mixes of one batch shape, the two freeze patterns, evaluation
through co_smoothing_core, and the switch-off model's unchanged bits.  Runs on the MI355X only."""
import random

import numpy as np
import pytest
import torch

import session_stitch as R
from conftest import load_json, load_npz
from helpers import build_model, make_optimizer, tiny_config
from model_checks import bf16_stats, check_bf16, check_stored_grads, fixture_batch, to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu
T_ = R.TINY


def stitched_config(bias=True, width=T_["P"], **kw):
    mc = tiny_config(max_F=T_["max_F"], **kw)
    mc["use_session"] = True
    mc["stitcher"] = {"width": width, "bias": bias}
    return mc


def make_model(bias=True, dtype="fp32", sessions=None, mc=None, seed=R.MODEL_SEED):
    model = build_model(mc or stitched_config(bias), T_["N_max"], T_["n_beh"], seed=seed, sessions=sessions or R.SESSIONS)
    model.compute_dtype = dtype
    return model.cuda().train()


def mod_dict(batch, objective, eids):
    md = O.make_mod_dict(batch, objective)
    md["ap"]["eid"] = eids
    return to_dev(md)


def step(model, batch, objective, eids, seed=R.MASKER_SEED, scale=1.0):
    torch.manual_seed(seed)
    random.seed(seed)
    md = mod_dict(batch, objective, eids)
    out = model(md)
    (out.loss * scale).backward()
    return out, md


def absent_names(model, eids):
    present = {model.session_index[e] for e in ([eids] if isinstance(eids, str) else eids)}
    return [k for k, _ in model.named_parameters() if k.startswith("session_") and int(k.split(".")[2]) not in present]


@pytest.fixture(scope="module")
def golden():
    return load_npz("session_stitch_fwd_bwd.npz")


# ------------------------------------------------------------------------------------------------- fp32 against the reference fixtures
@pytest.mark.parametrize("case", list(R.CASES) + list(R.XCASES))
def test_fp32_step_matches_the_reference(golden, case):
    z, meta = golden
    if case in R.XCASES:            # modality segments / input masking, on the mixed batch
        eids, bias, mode = R.XEIDS, True, R.XCASES[case].get("mode")
        model = build_model(stitched_config(), T_["N_max"], T_["n_beh"], seed=R.MODEL_SEED, sessions=R.SESSIONS, input_masking=bool(mode)).cuda().train()
        if mode:
            import input_masking as IM
            IM.set_masker(model.masker, mode)
    else:
        eids, obj, bias, _ = R.CASES[case]
        model = make_model(bias)
    named = dict(model.named_parameters())
    assert list(named) == meta["params"][case]
    for k, p in named.items():          # the session layers are drawn last: every parameter has the reference's bits
        assert np.array_equal(p.detach().cpu().numpy(), z[f"init/{meta['init'][case][k]}"]), k
    assert model.session_index == {e: k for k, e in enumerate(R.SESSIONS)}
    model.zero_grad(set_to_none=True)
    if case in R.XCASES:
        torch.manual_seed(R.MASKER_SEED)
        random.seed(R.MASKER_SEED)
        md = to_dev(R.xcase_mod_dict(case, R.xcase_batch(case)))
        out = model(md)
        out.loss.backward()
    else:
        out, md = step(model, R.case_batch(fixture_batch(z), case), obj, eids)
    print(case, "loss", out.loss.item(), "reference", float(z[f"{case}/loss"]))
    assert out.loss.item() == pytest.approx(float(z[f"{case}/loss"]), rel=1e-4)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(z[f"{case}/n/{m}"])
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"{case}/mask/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{case}/mod_loss/{m}"]), rel=1e-4, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{case}/preds/{m}"], rtol=1e-4, atol=1e-4)
    assert tuple(out.mod_preds["ap"].shape) == (T_["B"], T_["T"], T_["N_max"])         # (the spikes keep 8 bins in every case)
    for b, e in enumerate(eids):        # exact zeros beyond the session's neurons
        assert bool((out.mod_preds["ap"][b, :, R.SESSIONS[e]:] == 0).all())
    absent = absent_names(model, eids)
    for k, gn in zip(meta["params"][case], z[f"{case}/grad_norm"]):
        if k in absent:
            assert named[k].grad is None and np.isnan(gn), k
        else:
            assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=5e-3, abs=1e-8), k
    stored = check_stored_grads(named, z, case, meta["params"][case])
    assert len(stored) == (len(named) if case in R.FULL_GRAD else len([k for k in named if k.startswith("session_")]) - len(absent))


# ------------------------------------------------------------------------------------------------- curves
@pytest.mark.parametrize("name", ["turns", "accum"])
def test_curves_and_absent_sessions_keep_their_bytes(name):
    g = load_json("session_stitch_curve.json")
    c = g[name]
    model = make_model()
    opt, sch = make_optimizer(model, c["steps"])
    random.seed(42)
    torch.manual_seed(1234)
    losses, i = [], 0
    for s in range(c["steps"]):
        seen = set()
        for j in range(c["micro"]):
            obj = random.sample(list(R.OBJECTIVES), 1)[0]
            assert obj == c["objective"][i]
            eid = R.EIDS[i % 3]
            seen.add(eid)
            batch = O.synth_batch(T_["B"], T_["T"], T_["N_max"], T_["n_beh"], seed=i)
            batch["spikes_data"] = R.pad_batch(batch["spikes_data"], [eid] * T_["B"])
            out = model(mod_dict(batch, obj, eid))               # one string for the whole batch, as the trainer passes it
            (out.loss / c["micro"]).backward()
            losses.append(out.loss.detach())
            i += 1
        eng = model._engine
        spans = [eng.layout.entries[k] for k in absent_names(model, list(seen))]
        before = [[t[o:o + int(np.prod(sh))].clone() for o, sh in spans] for t in (eng.P, opt._m, opt._v) if t is not None]
        opt.step()
        sch.step()
        opt.zero_grad()
        for t, olds in zip([t for t in (eng.P, opt._m, opt._v) if t is not None], before):
            for (o, sh), old in zip(spans, olds):
                assert torch.equal(t[o:o + int(np.prod(sh))].view(torch.int32), old.view(torch.int32))
        assert (len(spans) > 0) == (c["micro"] == 1)
    got = [x.item() for x in losses]
    print(name, got[:3], "...", got[-1], "reference", c["loss"][-1])
    np.testing.assert_allclose(got, c["loss"], rtol=1e-4)


# ------------------------------------------------------------------------------------------------- pad independence
def test_pad_values_change_no_bit(golden):
    z, _ = golden
    eids = R.CASES["mixed"][0]
    outs = []
    for pad in (-1.0, 0.0, 1e30, float("nan")):
        model = make_model()
        out, _ = step(model, R.case_batch(fixture_batch(z), "mixed", pad=pad), "token_masking", eids)
        outs.append([out.loss.detach(), out.mod_preds["ap"].detach()] + [p.grad.clone() for _, p in model.named_parameters() if p.grad is not None])
    assert bool(torch.isfinite(outs[0][0]))
    for o in outs[1:]:
        assert len(o) == len(outs[0])
        for a, b in zip(o, outs[0]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_batch_padded_beyond_the_largest_session_changes_no_bit(golden):
    """The loader pads to its own width (--n_neurons), which may exceed every session: the extra columns are dropped unread and come
    back as zeros in mod_preds."""
    z, _ = golden
    eids = R.CASES["mixed"][0]
    batch = R.case_batch(fixture_batch(z), "mixed")
    wide = dict(batch, spikes_data=torch.nn.functional.pad(batch["spikes_data"], (0, 3), value=float("nan")))
    res = []
    for bt in (batch, wide):
        model = make_model()
        out, _ = step(model, bt, "encoding", eids)          # (no masker draw: its stream depends on the batch's width)
        res.append((out, [p.grad.clone() for _, p in model.named_parameters() if p.grad is not None]))
    (a, ga), (b, gb) = res
    assert tuple(b.mod_preds["ap"].shape) == (T_["B"], T_["T"], T_["N_max"] + 3) and bool((b.mod_preds["ap"][..., T_["N_max"]:] == 0).all())
    assert torch.equal(a.loss, b.loss) and torch.equal(a.mod_preds["ap"], b.mod_preds["ap"][..., :T_["N_max"]])
    assert int(a.mod_n_examples["ap"]) == int(b.mod_n_examples["ap"]) and all(torch.equal(x, y) for x, y in zip(ga, gb))


def test_entry_script_trains_multi_session_with_use_session(tmp_path):
    import os
    import subprocess
    import sys
    from conftest import ROOT
    script = os.path.join(ROOT, "multi_modal_foundation_model_amd", "src", "train_multi_modal.py")
    cmd = [sys.executable, script, "--mixed_training", "--use_session", "--stitch_width", "64", "--n_sessions", "3", "--epochs", "1",
           "--batches_per_epoch", "3", "--dtype", "bf16", "--base_path", str(tmp_path), "--overwrite"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------- bf16 against the fp32 engine
BIG = dict(B=6, T=33, sizes={"a": 150, "b": 129, "c": 64}, P=72, eids=["b", "a", "c", "a", "b", "c"])


def big_step(dtype, dropout=0.0, seed=R.MODEL_SEED):
    mc = stitched_config(width=BIG["P"], H=256, heads=8, inter=512, dropout=dropout, emb_dropout=dropout)
    mc["encoder"]["embedder"]["max_F"] = mc["decoder"]["embedder"]["max_F"] = BIG["T"]
    model = make_model(dtype=dtype, sessions=BIG["sizes"], mc=mc, seed=seed)
    model.engine_seed = 77
    batch = O.synth_batch(BIG["B"], BIG["T"], 150, T_["n_beh"], seed=4)
    for b, e in enumerate(BIG["eids"]):
        batch["spikes_data"][b, :, BIG["sizes"][e]:] = float("nan")
    out, _ = step(model, batch, "token_masking", BIG["eids"])
    return model, out


def test_bf16_step_against_the_fp32_engine():
    m32, o32 = big_step("fp32")
    m16, o16 = big_step("bf16")
    ref = dict(loss=o32.loss.detach().double())
    grads = {k: p.grad.double() for k, p in m32.named_parameters()}
    named = {k: p.grad for k, p in m16.named_parameters()}
    assert all(g is not None for g in named.values())
    check_bf16(bf16_stats(o16, named, ref, grads), "stitched bf16 step")
    for b, e in enumerate(BIG["eids"]):
        assert bool((o16.mod_preds["ap"][b, :, BIG["sizes"][e]:] == 0).all())


def test_dropout_on_step_is_finite_and_repeatable():
    (m1, o1), (m2, o2), (m0, o0) = big_step("bf16", dropout=0.2), big_step("bf16", dropout=0.2), big_step("bf16")
    assert bool(torch.isfinite(o1.loss)) and o1.loss.item() == o2.loss.item() and o1.loss.item() != o0.loss.item()
    for (k, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert bool(torch.isfinite(p.grad).all()) and torch.equal(p.grad, q.grad), k


# ------------------------------------------------------------------------------------------------- graph replay across mixes
def test_graph_replay_matches_eager_across_mixes(monkeypatch, golden):
    """Six optimiser steps over three mixes of one batch shape: with hipGraph replay (eager once, captured on the second step, replayed
    from the third - under mixes the capture never saw) the losses and the final parameters are those of MMFM_GRAPH=0, bit for bit.
    The body of model_checks.graph_replay_matches_eager with the eids a stitched batch needs."""
    z, _ = golden
    mixes = [R.CASES[c][0] for c in ("mixed", "absent", "single7/token_masking")]
    res, final = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MMFM_GRAPH", mode)
        model = make_model()
        opt, sch = make_optimizer(model, 6)
        torch.manual_seed(1234)
        losses = []
        for s in range(6):
            eids = mixes[s % 3]
            batch = O.synth_batch(T_["B"], T_["T"], T_["N_max"], T_["n_beh"], seed=s)
            batch["spikes_data"] = R.pad_batch(batch["spikes_data"], eids)
            out = model(mod_dict(batch, "token_masking", eids))
            out.loss.backward()
            opt.step(); sch.step(); opt.zero_grad()
            losses.append(out.loss.item())
        plan = model._engine._last
        assert (set(plan["graphs"]) == {"fwd", "bwd"}) == (mode == "1") and plan["runs"]["fwd"] == 6
        assert len([k for k in model._engine.plans if k[3]]) == 1          # one training plan served every mix
        res[mode], final[mode] = losses, {k: p.detach().clone() for k, p in model.named_parameters()}
    assert res["0"] == res["1"] and all(np.isfinite(res["0"]))
    for k, v in final["0"].items():
        assert torch.equal(final["1"][k], v), k


# ------------------------------------------------------------------------------------------------- freeze patterns
@pytest.mark.parametrize("keep", ["session_out.", "session_"])
def test_freeze_patterns_prune_the_backward(golden, keep):
    z, _ = golden
    eids = R.CASES["mixed"][0]
    batch = R.case_batch(fixture_batch(z), "mixed")
    full = make_model()
    step(full, batch, "token_masking", eids)
    frozen = make_model()
    for k, p in frozen.named_parameters():
        p.requires_grad_(k.startswith(keep))
    step(frozen, batch, "token_masking", eids)
    want = dict(full.named_parameters())
    for k, p in frozen.named_parameters():
        if k.startswith(keep):
            assert torch.equal(p.grad, want[k].grad), k
        else:
            assert p.grad is None, k
    rep = frozen._engine.backward_report(T_["B"], T_["T"])
    print(keep, frozen._engine.backward_summary(T_["B"], T_["T"]))
    assert "session_out.ap" not in rep["pruned"] and ("session_in.ap" in rep["pruned"]) == (keep == "session_out.")
    if keep == "session_out.":          # the loss backward of the stitched modality and the read-out's weight gradient, nothing else
        assert rep["launches"] == 2 and [n for name, n, _ in rep["segments"] if name != "head"] == [0] * (len(rep["segments"]) - 1)
    else:                               # down to the read-in: every segment still runs, no trunk weight gradient does
        assert all(n > 0 for _, n, _ in rep["segments"]) and rep["launches"] < rep["full"]
        assert {"encoder.0.attn.qkv", "decoder.0.mlp.down_proj", "decoder_proj_context", "decoder_embeddings.ap.out"} <= set(rep["pruned"])


# ------------------------------------------------------------------------------------------------- evaluation, refusals, switch off
def test_co_smoothing_core_forward_pred_on_a_stitched_model():
    from utils.eval_utils import co_smoothing_core
    model = make_model().eval()
    K_, n = 5, R.SESSIONS[R.EIDS[1]]
    b = O.synth_batch(K_, T_["T"], n, T_["n_beh"], seed=9)
    batch = {k: v.cuda() for k, v in b.items()}
    batch.update(eid=[R.EIDS[1]] * K_, neuron_regions=np.asarray([["XX"] * n] * K_))
    res = co_smoothing_core(model, batch, "forward_pred", heldout_idxs=[6, 7], region_list=["XX"] * n)        # the last two bins held out
    assert tuple(res["rates"].shape) == (K_, T_["T"], n) and bool(torch.isfinite(res["rates"]).all())
    assert len(res["bps"]) == n and list(res["bins"]) == [6, 7] and bool(torch.isfinite(res["loss"]))


def test_unknown_eid_and_narrow_batch_are_refused_before_any_draw(golden):
    z, _ = golden
    model = make_model()
    batch = fixture_batch(z)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="nobody"):
        model(mod_dict(batch, "token_masking", ["nobody"] * T_["B"]))
    narrow = dict(batch, spikes_data=batch["spikes_data"][..., :7])
    with pytest.raises(ValueError, match="ses.12"):
        model(mod_dict(narrow, "token_masking", [R.EIDS[0]] * T_["B"]))
    assert torch.equal(torch.get_rng_state(), state)


def test_switch_off_keeps_the_models_bits(golden):
    """use_session: false - the default - is today's model: no session parameter, no session launch, and the loss of the tiny fixture
    of tests/golden/tiny_fwd_bwd.npz to the bits the plain builder gives."""
    z, _ = golden
    batch = fixture_batch(z)
    a = build_model(tiny_config(max_F=T_["max_F"]), T_["N_max"], T_["n_beh"], seed=R.MODEL_SEED).cuda().train()
    mc = tiny_config(max_F=T_["max_F"])
    mc["stitcher"] = {"width": 8}           # a section without the switch changes nothing
    b = build_model(mc, T_["N_max"], T_["n_beh"], seed=R.MODEL_SEED).cuda().train()
    assert not any(k.startswith("session_") for k in b.state_dict()) and list(a.state_dict()) == list(b.state_dict())
    losses = []
    for model in (a, b):
        torch.manual_seed(R.MASKER_SEED)
        out = model(to_dev(O.make_mod_dict(batch, "token_masking")))
        out.loss.backward()
        losses.append(out.loss.detach())
        assert not any("session" in fn.__name__ for part in ("fwd",) for fn, _, _ in model._engine._last[part])
    assert torch.equal(losses[0], losses[1])
    with pytest.raises(ValueError, match="use_session"):
        build_model(tiny_config(max_F=T_["max_F"]), T_["N_max"], T_["n_beh"], seed=1, sessions=R.SESSIONS)
