"""Neuron padding (space_attn_mask with MultiModal.neuron_padding) through the whole model on the MI355X: the switch off is the recorded
plan and an all-ones mask is the switch off, bit for bit; the pad value is never read; bf16 against the fp32 engine at the bound of
tests/model_checks.py; dropout, hipGraph replay across batches with different masks, accumulation over two sessions, a frozen trunk;
exact zeros in the head rows of channels no sample of a batch has; the refusals; the trainer on multi-session batches."""
import random

import numpy as np
import pytest
import torch

import input_masking as IM
import model_checks as MC
import mod_segments as S
import neuron_padding as NP
import plan_sig as PS
from conftest import load_json
from helpers import build_model, build_model_mods, load_config, make_optimizer, model_config, tiny_config

pytestmark = pytest.mark.gpu

B, T, N = NP.TINY["B"], NP.TINY["T"], NP.TINY["n_ap"]


def fresh(dtype="fp32", neuron_padding=True, input_masking=False, **cfg):
    model = build_model(tiny_config(**cfg), N, NP.TINY["n_beh"], seed=NP.MODEL_SEED, neuron_padding=neuron_padding, input_masking=input_masking)
    IM.set_masker(model.masker)
    model.compute_dtype = dtype
    return model.cuda().train()


def padded_batch(n, seed=NP.DATA_SEED, value=NP.PAD_VALUE, side="right"):
    v = NP.channel_mask(n, side=side)
    return NP.pad_spikes(S.ragged_batch(B, (T, T), N, NP.TINY["n_beh"], seed, max_F=NP.TINY["max_F"]), v, value), v


def step(model, batch, v, objective="token_masking", mode=None, seed=NP.MASKER_SEED, zero_grad=True):
    if zero_grad:
        model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    random.seed(seed)
    out = model(MC.to_dev(NP.make_mod_dict(batch, v, objective, mode)))
    out.loss.backward()
    return out


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def same_step(a, b, what):
    (oa, ga), (ob, gb) = a, b
    assert torch.equal(bits(oa.loss.detach()), bits(ob.loss.detach())), f"{what}: loss bits"
    for mod in oa.mod_loss:
        assert torch.equal(bits(oa.mod_loss[mod]), bits(ob.mod_loss[mod])) and int(oa.mod_n_examples[mod]) == int(ob.mod_n_examples[mod]), (what, mod)
    for k in ga:
        assert torch.equal(bits(ga[k]), bits(gb[k])), f"{what}: gradient bits of {k}"


def test_switch_off_builds_the_recorded_plan_and_all_ones_changes_only_the_loss_launches(monkeypatch):
    """The default model under the switch off, on a batch that carries the mask: the plan is the one tests/golden/plan_signatures.json
    records, under the key it always had.  The switch on: a plan of its own whose launches differ in the spike loss alone."""
    from multi_modal_foundation_model_amd.synthetic import synth_batch
    for k in PS.SWITCHES + PS.AUTO:
        monkeypatch.delenv(k, raising=False)
    case = next(c for c in PS.CASES if c["name"] == "default_B16")
    golden = load_json("plan_signatures.json")[case["name"]]
    model = build_model(load_config().model, 668, 2, seed=42)
    model.compute_dtype = case["dtype"]
    model.cuda().train()
    assert model.neuron_padding is False
    b = synth_batch(case["B"], case["T"], 668, 2, seed=1)
    batch = dict(ap=dict(inputs=b["spikes_data"], ts=b["spikes_timestamps"], attn=b["time_attn_mask"]),
                 behavior=dict(inputs=b["target"], ts=b["spikes_timestamps"], attn=b["time_attn_mask"]))
    v = torch.ones(case["B"], 668, dtype=torch.int64)
    off = step(model, batch, v, "encoding")
    eng = model._engine
    assert set(eng.plans) == {(case["B"], case["T"], True, True)}
    sig = PS.plan_signature(eng, eng._last)
    assert list(sig) == list(golden)
    for unit, want in golden.items():
        assert sig[unit]["names"] == want["names"] and sig[unit]["sha256"] == want["sha256"], unit
    model.neuron_padding = True
    on = step(model, batch, v, "encoding")
    assert len(eng.plans) == 2 and eng._last is not eng.plans[(case["B"], case["T"], True, True)]
    sig_on = PS.plan_signature(eng, eng._last)
    swap = {"mmfm_masked_loss_fwd": "mmfm_masked_loss_chan_fwd", "mmfm_masked_loss_bwd": "mmfm_masked_loss_chan_bwd"}
    for unit, want in golden.items():
        names, seen = list(want["names"]), set()
        for i, nm in enumerate(names):            # the spike loss is the first loss launch of each direction
            if nm in swap and nm not in seen:
                names[i] = swap[nm]
                seen.add(nm)
        assert sig_on[unit]["names"] == names, unit
    assert int(on.mod_n_examples["ap"]) == int(off.mod_n_examples["ap"]) == case["B"] * case["T"] * 668


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("objective", ["encoding", "token_masking"])
def test_all_ones_mask_is_the_switch_off_bit_for_bit(objective, dtype):
    batch, _ = padded_batch((N,) * B)
    ones = torch.ones(B, N, dtype=torch.int64)
    runs = []
    for switch, v in ((False, ones), (True, ones), (False, None)):
        model = fresh(dtype, neuron_padding=switch)
        out = step(model, batch, v, objective)
        runs.append((out, grads_of(model)))
        chan_plans = [k for k in model._engine.plans if len(k) > 5]
        assert len(chan_plans) == (1 if switch else 0)
    same_step(runs[0], runs[1], f"{objective} {dtype}: all-ones mask against the switch off")
    same_step(runs[0], runs[2], f"{objective} {dtype}: the key is ignored under the switch off")
    assert bool(torch.isfinite(runs[0][0].loss))


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("objective", ["encoding", "token_masking"])
def test_the_pad_value_is_never_read(objective, side):
    n = (N, 7, 0)
    runs = []
    values = (-1.0, 0.0, 1e30, float("nan"))
    for value in values:
        batch, v = padded_batch(n, value=value, side=side)
        model = fresh()
        out = step(model, batch, v, objective)
        runs.append((out, grads_of(model)))
        assert bool(torch.isfinite(out.loss)), value
    for value, run in zip(values[1:], runs[1:]):
        same_step(runs[0], run, f"{objective} {side}: pad value {value} against -1")


def test_switch_off_reads_the_padding_as_upstream_does():
    """The counterpart of the test above: with the switch off the -1 of a padded channel is an input and a target, and is counted."""
    batch, v = padded_batch((N, 7, 0))
    on, off = fresh(), fresh(neuron_padding=False)
    o_on, o_off = step(on, batch, v, "encoding"), step(off, batch, v, "encoding")
    assert int(o_off.mod_n_examples["ap"]) == B * T * N and int(o_on.mod_n_examples["ap"]) == T * (N + 7)
    assert o_on.loss.item() != o_off.loss.item()


def test_bf16_step_against_the_fp32_engine():
    """Hidden 256, B 4, n = (668, 484, 300, 0): the bf16 step against the fp32 engine on the same masks, at tests/model_checks.py's bound."""
    Bb, Tb, n = 4, 100, (668, 484, 300, 0)
    v = NP.channel_mask(n, n_ap=668)
    runs = {}
    for dtype in ("fp32", "bf16"):
        batch = NP.pad_spikes(S.ragged_batch(Bb, (Tb, Tb), 668, 2, 5, max_F=Tb), v)
        model = build_model(model_config(n_enc=2, n_dec=2, dropout=0.0, emb_dropout=0.0), 668, 2, seed=3, neuron_padding=True)
        model.compute_dtype = dtype
        model.cuda().train()
        out = step(model, batch, v, "token_masking", seed=5)
        runs[dtype] = (out, grads_of(model))
    (o32, g32), (o16, g16) = runs["fp32"], runs["bf16"]
    for mod in ("ap", "behavior"):
        assert int(o16.mod_n_examples[mod]) == int(o32.mod_n_examples[mod]) > 0
    assert int(o32.mod_n_examples["ap"]) % 4 == 0 and int(o32.mod_n_examples["ap"]) <= Tb * sum(n)
    MC.check_bf16(MC.bf16_stats(o16, g16, dict(loss=o32.loss.detach()), g32), "neuron padding bf16 vs fp32")


def test_head_rows_of_channels_no_sample_has_get_exactly_zero_gradient():
    batch, v = padded_batch((9, 7, 0))
    for dtype, objective in (("fp32", "encoding"), ("bf16", "token_masking")):
        model = fresh(dtype, dropout=0.1, emb_dropout=0.1)                      # a dropout-on step
        out = step(model, batch, v, objective)
        assert bool(torch.isfinite(out.loss))
        g = grads_of(model)
        w, bias = g["decoder_embeddings.ap.out.weight"], g["decoder_embeddings.ap.out.bias"]
        assert tuple(w.shape)[0] == N
        assert bool((w[9:] == 0).all()) and bool((bias[9:] == 0).all()), "channels 9.. are padding in every sample of the batch"
        assert bool((w[:9] != 0).any(dim=1).all()) and float(bias[:9].abs().min()) > 0
        # ... and their zeroed inputs move nothing in either tokeniser (under `encoding` every spike token is masked: nothing does)
        for side in ("encoder", "decoder"):
            te = g[f"{side}_embeddings.ap.embedder.token_embed.weight"]
            assert bool((te[:, 9:] == 0).all())
        if objective == "token_masking":
            assert bool((g["encoder_embeddings.ap.embedder.token_embed.weight"][:, :9] != 0).any())
        assert all(bool(torch.isfinite(x).all()) for x in g.values())
        if objective == "encoding":
            assert int(out.mod_n_examples["ap"]) == T * (9 + 7)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graph_replay_across_batches_with_different_masks(dtype, monkeypatch):
    """Two batches of one shape whose masks differ share a plan (the mask is data in a static buffer): replayed graphs give the eager bits."""
    pairs = [padded_batch((N, 7, 0), seed=0), padded_batch((4, 12, 9), seed=1, side="left")]
    res = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("MMFM_GRAPH", graph)
        model = fresh(dtype)
        res[graph] = []
        for i in range(6):
            batch, v = pairs[i % 2]
            out = step(model, batch, v, "encoding")
            res[graph].append((out.loss.detach().clone(), int(out.mod_n_examples["ap"]), model._engine.G.clone()))
        plan = model._engine._last
        assert len(model._engine.plans) == 1 and plan["runs"]["fwd"] == 6
        assert (set(plan["graphs"]) == {"fwd", "bwd"}) == (graph == "1")
    assert [r[1] for r in res["1"]] == [T * (N + 7), T * 25] * 3
    for (l0, n0, g0), (l1, n1, g1) in zip(res["0"], res["1"]):
        assert torch.equal(l0, l1) and n0 == n1 and torch.equal(bits(g0), bits(g1))
    assert torch.equal(res["1"][0][0], res["1"][2][0]) and not torch.equal(res["1"][0][0], res["1"][1][0])


def test_accumulation_over_two_sessions_adds_the_two_gradients():
    sessions = [padded_batch((9,) * B, seed=0), padded_batch((6,) * B, seed=1)]
    single = []
    for batch, v in sessions:
        model = fresh()
        step(model, batch, v, "encoding")
        single.append(grads_of(model))
    model = fresh()
    for batch, v in sessions:                          # no zero_grad in between
        step(model, batch, v, "encoding", zero_grad=False)
    for k, g in grads_of(model).items():
        assert torch.equal(bits(g), bits(single[1][k] + single[0][k])), k


def test_frozen_trunk_equals_the_all_trainable_twin():
    batch, v = padded_batch((N, 7, 0))
    grads = {}
    for name in ("twin", "frozen"):
        model = fresh(n_enc=2, n_dec=2)
        named = dict(model.named_parameters())
        frozen = [k for k in named if k.startswith(("encoder.", "decoder."))] if name == "frozen" else []
        for k in frozen:
            named[k].requires_grad_(False)
        step(model, batch, v, "token_masking")
        grads[name] = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in named.items()}
        if frozen:
            rep = model._engine._last["report"]
            assert rep["pruned"] and sum(n_ for _, n_, _ in rep["segments"]) < sum(full for _, _, full in rep["segments"])
            assert model._engine.backward_report(B, T)["launches"] == sum(n_ for _, n_, _ in rep["segments"])
    kept = [k for k, g in grads["frozen"].items() if g is not None]
    assert kept and len(kept) < len(grads["twin"])
    for k in kept:
        assert torch.equal(bits(grads["frozen"][k]), bits(grads["twin"][k])), k


def test_frozen_heads_prune_the_chan_backward_like_the_row_form():
    """Nothing below the heads is trainable and neither is the spike head: its loss backward is not launched, as the row form's is not."""
    batch, v = padded_batch((N, 7, 0))
    names = {}
    for switch in (False, True):
        model = fresh(neuron_padding=switch)
        for k, p in model.named_parameters():
            p.requires_grad_(k.startswith("decoder_embeddings.behavior.out"))
        step(model, batch, v, "token_masking")
        names[switch] = [fn.__name__ for _, seg in model._engine._last["bwd"] for fn, _, _ in seg]
    assert not any("chan" in nm for nm in names[True]) and names[True] == names[False]


@pytest.mark.parametrize("mode,form", [("temporal", "chan"), ("forward-pred", "chan"), ("neuron", "elem"), ("co-smooth", "elem"), ("random", "elem")])
def test_input_masking_modes_take_the_form_their_target_mask_allows(mode, form):
    """With input masking, a [B,T,1] / [1,T,1] target mask is the chan form's row mask; one that carries the channel axis is AND-ed
    with the channel mask and runs the element form.  Either way the count is the number of set elements of spike_mask x v."""
    batch, v = padded_batch((N, 7, 0))
    model = fresh(input_masking=True)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(NP.MASKER_SEED)
    random.seed(NP.MASKER_SEED)
    md = MC.to_dev(NP.make_mod_dict(batch, v, mode=mode))
    out = model(md)
    out.loss.backward()
    fwd = [fn.__name__ for fn, _, _ in model._engine._last["fwd"]]
    assert ("mmfm_masked_loss_chan_fwd" in fwd) == (form == "chan")
    want = int((md["ap"]["spike_mask"] * v.cuda()[:, None, :]).sum())
    assert int(out.mod_n_examples["ap"]) == want
    staged = model._engine.b["in/0"].view(B, T, -1)[..., :N]
    assert bool((staged[v.cuda()[:, None, :].expand(B, T, N) == 0] == 0).all()), "padded channels are staged as zeros"
    g = model.decoder_embeddings["ap"].out.weight.grad
    assert bool(torch.isfinite(g).all()) and (want == 0 or float(g.abs().max()) > 0)


@pytest.mark.parametrize("mode", ["neuron", "temporal", "random"])
def test_the_maskers_own_corruption_keeps_its_noise_and_loses_only_the_padding(mode):
    """zero_ratio 0.5: the masker corrupts the inputs itself - noise and kept values under its mask.  What is staged is its output with
    the padded channels zeroed, nothing else."""
    batch, v = padded_batch((N, 7, 0))
    model = fresh(input_masking=True)
    model.masker.zero_ratio, model.masker.random_ratio = 0.5, 1.0
    torch.manual_seed(NP.MASKER_SEED)
    random.seed(NP.MASKER_SEED)
    md = MC.to_dev(NP.make_mod_dict(batch, v, mode=mode))
    out = model(md)
    out.loss.backward()
    corrupted, real = md["ap"]["inputs"], v.cuda()[:, None, :].expand(B, T, N) != 0
    staged = model._engine.b["in/0"].view(B, T, -1)[..., :N]
    assert torch.equal(staged, torch.where(real, corrupted, torch.zeros_like(corrupted)))
    under = (md["ap"]["spike_mask"] != 0) & real
    assert bool((staged[under] != 0).any()), "zero_ratio 0.5 leaves noise or kept values under the masker's mask"
    assert int(out.mod_n_examples["ap"]) == int(under.sum()) and bool(torch.isfinite(out.loss))


def test_softmax_cross_entropy_modality_with_the_key_is_refused():
    from multi_modal.losses import SoftmaxCrossEntropy
    mods = [("ap", 12), ("behavior", 2), ("choice", 3)]
    model = build_model_mods(tiny_config(n_modality=3), mods, seed=0, neuron_padding=True)
    model.loss_mod["choice"] = SoftmaxCrossEntropy()
    IM.set_masker(model.masker)
    model.cuda().train()
    batch, v = padded_batch((N, 7, 0))
    md = NP.make_mod_dict(batch, v, "token_masking")
    lab = torch.nn.functional.one_hot(torch.randint(0, 3, (B, T), generator=torch.Generator().manual_seed(1)), 3).float()
    md["choice"] = dict(md["behavior"], inputs=lab.clone(), targets=lab.clone(), inputs_modality=torch.tensor(2))
    md["choice"]["space_attn_mask"] = torch.ones(B, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="'choice'"):
        model(MC.to_dev(md))
    assert not model._engine.plans, "refused when the plan is built: nothing is cached"
    del md["choice"]["space_attn_mask"]                # without the key the modality is as it always was
    torch.manual_seed(1)
    assert bool(torch.isfinite(model(MC.to_dev(md)).loss))


def test_engine_refuses_malformed_channel_masks():
    model = fresh()
    batch, v = padded_batch((N, 7, 0))
    step(model, batch, v, "encoding")
    eng = model._engine
    x = [batch[m]["inputs"].cuda() for m in ("ap", "behavior")]
    ones = [torch.ones(B, T, dtype=torch.int64, device="cuda")] * 2
    ts, attn = batch["ap"]["ts"].cuda(), batch["ap"]["attn"].cuda()
    good = v.to(torch.uint8).cuda()
    for bad in (good[:, :5], good.bool(), good[:2], good[None]):
        with pytest.raises(ValueError, match="channel mask"):
            eng.forward(B, T, x, x, ones, ts, attn, training=True, chan=[bad, None])
    with pytest.raises(ValueError, match="channel-mask entries"):
        eng.forward(B, T, x, x, ones, ts, attn, training=True, chan=[good])
    # one [1, N] mask for all samples is a plan of its own
    out = eng.forward(B, T, x, x, ones, ts, attn, training=True, chan=[good[1:2], None])
    assert int(out["mod_n"][0]) == B * T * 7 and len({k for k in eng.plans if len(k) > 5}) == 2


def test_trainer_trains_on_multi_session_batches(tmp_path):
    """training.neuron_padding through the trainer on MultiSessionLoader batches: finite losses, moving parameters, one channel-masked
    plan for all sessions, and head rows beyond the widest session untouched by the optimiser's gradient."""
    from multi_modal_foundation_model_amd.ddp import Accelerator
    from multi_modal_foundation_model_amd.synthetic import MultiSessionLoader
    from trainer.make import make_multimodal_trainer
    n_ap, n_batches = 320, 4
    loader = MultiSessionLoader(n_batches, 4, T=T, n_ap=n_ap, n_beh=2, n_sessions=2)
    assert max(loader.sizes) < n_ap or loader.sizes[0] != loader.sizes[1]
    model = build_model(tiny_config(), n_ap, 2, seed=7)
    acc = Accelerator()
    model = acc.prepare(model)
    opt, sch = make_optimizer(model, n_batches, lr=1e-3)
    cfg = load_config()
    cfg["training"]["neuron_padding"] = True
    tr = make_multimodal_trainer(model=model, train_dataloader=loader, eval_dataloader=[], optimizer=opt, log_dir=str(tmp_path), accelerator=acc,
                                 lr_scheduler=sch, avail_mod=["ap", "behavior"], config=cfg,
                                 modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=True, num_neurons=[n_ap])
    assert model.neuron_padding is True
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    random.seed(42)
    torch.manual_seed(99)
    res = tr.train_epoch(0)
    assert np.isfinite(res["train_loss"])
    assert any(not torch.equal(p, before[k]) for k, p in model.named_parameters())
    assert len({k[5] for k in model._engine.plans if len(k) > 5}) == 1
