"""Input masking (mask_type: input with MultiModal.input_masking) through the whole model on the MI355X: the fp32 engine against the
reference's own pieces composed as mm.py:245-300 calls them (tests/golden/input_masking_*, scripts/make_input_masking_goldens.py) at the
tolerances tests/test_model_gpu.py uses for its reference fixtures (tests/model_checks.py); bf16 against fp32 per broadcast pattern;
hipGraph replay; eviction of element-mask patterns; a frozen trunk with accumulation; the refusals; the switch left off."""
import random

import numpy as np
import pytest
import torch

import input_masking as IM
import model_checks as MC
from conftest import load_json, load_npz
from helpers import build_model, build_model_mods, make_optimizer, tiny_config

pytestmark = pytest.mark.gpu

MODS = ("ap", "behavior")
# one mode per broadcast pattern of the element masks: [B,T,1], [B,1,N], [1,1,N], [1,T,1], [B,T,N]
PATTERN_MODES = ["temporal", "neuron", "co-smooth", "forward-pred", "random"]


def fresh(case=None, dtype="fp32", input_masking=True, **cfg):
    model = build_model(tiny_config(**cfg), IM.TINY["n_ap"], IM.TINY["n_beh"], seed=IM.MODEL_SEED, input_masking=input_masking)
    IM.set_masker(model.masker, case)
    model.compute_dtype = dtype
    return model.cuda().train()


def step(model, batch, mode, seed=IM.MASKER_SEED, backward=True, zero_grad=True):
    if zero_grad:
        model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    random.seed(seed)
    md = MC.to_dev(IM.make_mod_dict(batch, mode))
    out = model(md)
    if backward:
        out.loss.backward()
    return out, md


def fixture_batch(z, case):
    return {mod: {k: torch.from_numpy(z[f"batch/{case}/{mod}/{k}"]) for k in ("inputs", "ts", "attn")} for mod in MODS}


@pytest.fixture(scope="module")
def golden():
    return load_npz("input_masking_fwd_bwd.npz")


@pytest.mark.parametrize("case", list(IM.CASES))
def test_fp32_engine_against_the_reference_pieces(golden, case):
    z, meta = golden
    assert meta["cases"] == list(IM.CASES)
    model = fresh(case)
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names
    batch = fixture_batch(z, case)
    out, md = step(model, batch, IM.CASES[case]["mode"])
    eng = model._engine
    ref_loss = float(z[f"{case}/loss"])
    print(case, "loss", out.loss.item(), "reference", ref_loss)
    for i, mod in enumerate(MODS):
        Bm, Tm, Nm = batch[mod]["inputs"].shape
        assert int(out.mod_n_examples[mod]) == int(z[f"{case}/n/{mod}"])
        sm = md[mod]["spike_mask"]
        assert sm.dtype == torch.int64 and tuple(sm.shape) == (Bm, Tm, Nm)
        np.testing.assert_array_equal(sm.cpu().numpy(), z[f"{case}/tm/{mod}"].astype(np.int64))
        assert int(md[mod]["inputs_mask"].sum()) == 0, "no token is masked on this branch"
        staged = eng.b[f"in/{i}"].view(Bm, Tm, -1)[..., :Nm]
        np.testing.assert_array_equal(staged.cpu().numpy(), z[f"{case}/inputs/{mod}"])
        assert out.mod_loss[mod].item() == pytest.approx(float(z[f"{case}/mod_loss/{mod}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[mod].cpu().numpy(), z[f"{case}/preds/{mod}"], rtol=1e-4, atol=2e-5)
    if np.isnan(ref_loss):                 # nothing is a target (causal: no bin drawn at p = 0.01): 0 / 0 and NaN gradients, as upstream
        assert sum(int(v) for v in out.mod_n_examples.values()) == 0 and bool(torch.isnan(out.loss))
        assert bool(np.isnan(z[f"{case}/grad_norm"]).any())
        for k, gn in zip(names, z[f"{case}/grad_norm"]):
            assert bool(torch.isnan(named[k].grad.double().norm())) == bool(np.isnan(gn)), k
        return
    assert out.loss.item() == pytest.approx(ref_loss, rel=2e-5)
    for k, gn in zip(names, z[f"{case}/grad_norm"]):
        assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=5e-3, abs=1e-8), k
    stored = MC.check_stored_grads(named, z, case, names)
    assert len(stored) == (len(names) if case in IM.FULL_GRAD else 0)


def test_50_step_curve(golden):
    g = load_json("input_masking_curve.json")
    model = fresh()
    opt, sch = make_optimizer(model, g["total_steps"])
    random.seed(42)
    torch.manual_seed(1234)
    losses = []
    for s in range(g["total_steps"]):
        mode = random.sample(IM.CURVE_MODES, 1)[0]
        assert mode == g["mode"][s]
        out = model(MC.to_dev(IM.make_mod_dict(IM.case_batch(seed=s), mode)))
        out.loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(out.loss.detach())
    losses = [x.item() for x in losses]
    print("curve", losses[:3], "...", losses[-1], "reference", g["loss"][:3], "...", g["loss"][-1])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


@pytest.mark.parametrize("mode", PATTERN_MODES)
def test_bf16_step_against_fp32(mode):
    batch = IM.case_batch()
    runs = {}
    for dtype in ("fp32", "bf16"):
        model = fresh(dtype=dtype)
        out, md = step(model, batch, mode)
        runs[dtype] = (out, {k: p.grad.detach().clone() for k, p in model.named_parameters()}, md)
    (o32, g32, md32), (o16, g16, md16) = runs["fp32"], runs["bf16"]
    for mod in MODS:
        assert torch.equal(md16[mod]["spike_mask"], md32[mod]["spike_mask"])
        assert int(o16.mod_n_examples[mod]) == int(o32.mod_n_examples[mod]) == int(md32[mod]["spike_mask"].sum())
    MC.check_bf16(MC.bf16_stats(o16, g16, dict(loss=o32.loss.detach()), g32), f"input masking {mode} bf16 vs fp32")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_replay_gives_the_eager_bits(dtype):
    model = fresh(dtype=dtype)
    batch = IM.case_batch()
    res = []
    for _ in range(3):                       # eager, captured and replayed, replayed
        model.zero_grad(set_to_none=True)
        out, _ = step(model, batch, "intra-region")
        res.append((out.loss.detach().clone(), model._engine.G.clone()))
    plan = model._engine._last
    assert set(plan["graphs"]) == {"fwd", "bwd"} and plan["runs"]["fwd"] == 3
    for loss, G in res[1:]:
        assert torch.equal(loss, res[0][0]) and torch.equal(G.view(torch.int32), res[0][1].view(torch.int32))


def test_alternating_patterns_evict_and_rebuild():
    from multi_modal_foundation_model_amd.engine import MAX_PATTERNS
    model = fresh()
    batch = IM.case_batch()
    B, T = IM.TINY["B"], IM.TINY["T"]
    first = {}
    for mode in PATTERN_MODES:
        out, _ = step(model, batch, mode)
        first[mode] = (out.loss.detach().clone(), model._engine.G.clone())
    eng = model._engine
    assert len(PATTERN_MODES) == MAX_PATTERNS + 1 and len(eng._elem_lru[(B, T)]) == MAX_PATTERNS
    live = {k[5] for k in eng.plans if len(k) > 5}
    assert live == set(eng._elem_lru[(B, T)]) and len(live) == MAX_PATTERNS, "the least recently used pattern's plans are dropped"
    for mode in PATTERN_MODES + PATTERN_MODES[::-1]:          # every one is evicted and rebuilt at least once more
        out, _ = step(model, batch, mode)
        assert torch.equal(out.loss.detach(), first[mode][0]), mode
        assert torch.equal(eng.G.view(torch.int32), first[mode][1].view(torch.int32)), mode
        assert len({k[5] for k in eng.plans if len(k) > 5}) == MAX_PATTERNS
    # the plain token-mask plan of the shape lives beside them under the key it always had
    model.input_masking = False
    out = model(MC.to_dev(IM.make_mod_dict(batch, None)))
    assert (B, T, True, True) in eng.plans and bool(torch.isfinite(out.loss))


def test_frozen_trunk_with_accumulation_equals_the_all_trainable_twin():
    cfg = dict(n_enc=2, n_dec=2)
    batches = [IM.case_batch(seed=s) for s in (0, 1)]
    grads = {}
    for name in ("twin", "frozen"):
        model = fresh(**cfg)
        named = dict(model.named_parameters())
        frozen = [k for k in named if k.startswith(("encoder.", "decoder."))] if name == "frozen" else []
        assert (len(frozen) > 0) == (name == "frozen")
        for k in frozen:
            named[k].requires_grad_(False)
        for s, (batch, mode) in enumerate(zip(batches, ("neuron", "intra-region"))):       # two patterns, no zero_grad in between
            step(model, batch, mode, seed=100 + s, zero_grad=False)
        grads[name] = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in named.items()}
        assert all(grads[name][k] is None for k in frozen)
        if frozen:                                # the element-masked plan of a freeze pattern is pruned like any other
            rep = model._engine._last["report"]
            assert rep["pruned"] and sum(n for _, n, _ in rep["segments"]) < sum(full for _, _, full in rep["segments"])
    kept = [k for k, g in grads["frozen"].items() if g is not None]
    assert kept and len(kept) < len(grads["twin"])
    for k in kept:
        assert torch.equal(grads["frozen"][k].view(torch.int32), grads["twin"][k].view(torch.int32)), k


def ce_model_and_dict(mode):
    from multi_modal.losses import SoftmaxCrossEntropy
    mods = [("ap", 12), ("behavior", 2), ("choice", 3)]
    model = build_model_mods(tiny_config(n_modality=3), mods, seed=0, input_masking=True)
    model.loss_mod["choice"] = SoftmaxCrossEntropy()
    IM.set_masker(model.masker)
    model.cuda().train()
    md = IM.make_mod_dict(IM.case_batch(), mode)
    lab = torch.nn.functional.one_hot(torch.randint(0, 3, (IM.TINY["B"], IM.TINY["T"]), generator=torch.Generator().manual_seed(1)), 3).float()
    md["choice"] = dict(md["behavior"], inputs=lab.clone(), targets=lab.clone(), inputs_modality=torch.tensor(2))
    return model, md


@pytest.mark.parametrize("mode", ["temporal", "forward-pred"])
def test_softmax_cross_entropy_modality_runs_under_a_row_mask(mode):
    """The target mask is constant over the classes: the existing softmax cross-entropy kernels run with it as their row mask and the
    count is N per set row.  Checked against the loss recomputed in fp64 from the returned predictions (tests/ce_refs.py)."""
    import ce_refs as CR
    model, md = ce_model_and_dict(mode)
    torch.manual_seed(3)
    random.seed(3)
    md = MC.to_dev(md)
    out = model(md)
    out.loss.backward()
    tm = md["choice"]["spike_mask"]
    assert tuple(tm.shape) == (IM.TINY["B"], IM.TINY["T"], 3) and bool((tm == tm[:, :, :1]).all()) and int(tm.sum()) > 0
    assert int(out.mod_n_examples["choice"]) == int(tm.sum())
    el = CR.ce_elem(out.mod_preds["choice"].double(), md["choice"]["targets"].double(), None, 0.0)
    assert out.mod_loss["choice"].item() == pytest.approx(float((el * tm).sum()), rel=1e-5)
    total = sum(v.double() for v in out.mod_loss.values()) / sum(int(v) for v in out.mod_n_examples.values())
    assert out.loss.item() == pytest.approx(float(total), rel=1e-5)
    g = model.decoder_embeddings["choice"].out.bias.grad
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_softmax_cross_entropy_modality_is_refused_before_any_draw():
    model, md = ce_model_and_dict("neuron")
    torch.manual_seed(3)
    before = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="choice.*neuron"):
        model(MC.to_dev(md))
    assert torch.equal(torch.get_rng_state(), before) and model._engine is None, "refused before any draw and any launch"


def test_switch_off_still_fails_like_upstream():
    model = fresh(input_masking=False)
    assert model.input_masking is False
    with pytest.raises(UnboundLocalError, match="mask"):
        model(MC.to_dev(IM.make_mod_dict(IM.case_batch(), "neuron")))


def test_engine_refuses_malformed_element_masks():
    model = fresh()
    batch = IM.case_batch()
    step(model, batch, "neuron", backward=False)
    eng, B, T = model._engine, IM.TINY["B"], IM.TINY["T"]
    x = [batch[m]["inputs"].cuda() for m in MODS]
    zeros = [torch.zeros(B, T, dtype=torch.int64, device="cuda")] * 2
    ts, attn = batch["ap"]["ts"].cuda(), batch["ap"]["attn"].cuda()
    bad = torch.zeros(B, 2, 12, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="element mask"):
        eng.forward(B, T, x, x, zeros, ts, attn, training=True, elem=[(bad, bad, None), None])
    with pytest.raises(ValueError, match="element-mask entries"):
        eng.forward(B, T, x, x, zeros, ts, attn, training=True, elem=[(bad, bad, None)])


def test_trainer_trains_with_input_masking(tmp_path):
    """training.input_masking through the trainer: the mode is sampled per step from training.mask_mode, every step has a finite loss
    and the parameters move; the epoch ran element-masked plans of at most three patterns."""
    from multi_modal_foundation_model_amd.ddp import Accelerator
    from oracle import mm_oracle as O
    from trainer.make import make_multimodal_trainer
    from helpers import load_config
    B, T, n_ap, n_beh, n_batches = 4, IM.TINY["T"], IM.TINY["n_ap"], IM.TINY["n_beh"], 6
    batches = []
    for i in range(n_batches):
        b = O.synth_batch(B, T, n_ap, n_beh, seed=i)
        b["eid"] = ["synthetic"] * B
        b["neuron_regions"] = [[r] * B for r in IM.regions(1)[0]]
        batches.append(b)
    model = build_model(tiny_config(), n_ap, n_beh, seed=7)
    IM.set_masker(model.masker)
    model.masker.ratio = 0.9                  # (a step that draws no target at all is 0 / 0: kept out of this test by construction)
    acc = Accelerator()
    model = acc.prepare(model)
    opt, sch = make_optimizer(model, n_batches, lr=1e-3)
    cfg = load_config()
    for k, v in dict(mask_type="input", input_masking=True, mask_mode=list(IM.CURVE_MODES)).items():
        cfg["training"][k] = v
    tr = make_multimodal_trainer(model=model, train_dataloader=batches, eval_dataloader=[], optimizer=opt, log_dir=str(tmp_path), accelerator=acc,
                                 lr_scheduler=sch, avail_mod=["ap", "behavior"], config=cfg,
                                 modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=True, num_neurons=[n_ap])
    assert model.input_masking is True          # (mixed_training: the objective is sampled too; its eval masks are ignored on this branch)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    random.seed(42)
    torch.manual_seed(99)
    res = tr.train_epoch(0)
    assert np.isfinite(res["train_loss"])
    assert any(not torch.equal(p, before[k]) for k, p in model.named_parameters())
    keys = {k[5] for k in model._engine.plans if len(k) > 5}
    assert 1 <= len(keys) <= 3          # [B,T,1] on both; [B,1,N] on both; [B,1,N] on the spikes alone (a region mode: behaviour is left alone)
