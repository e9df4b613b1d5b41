"""Shared by the whole-model GPU tests (and, for to_dev, by scripts/step_timer.py): the one definition of the batch mover, the gradient
cosine, the optimiser-step curve, the reference-fixture forward / backward check, the checkpoint-resume and hipGraph-replay bodies and
the engine step / fp64 oracle pair with its bf16 criteria.  A plain module like helpers.py: the tests keep their configs, case tables
and whatever they assert beyond these bodies."""
import contextlib
import random
from unittest import mock

import numpy as np
import pytest
import torch

import dropout_refs as DR
from helpers import build_model, load_config, make_optimizer
from oracle import mm_oracle as O


def to_dev(md, targets=True):
    """The mod dict on the GPU; `targets` also names the targets' modality / time stamps, which the tests pass and the step timers
    (targets=False) never did."""
    for d in md.values():
        for k, v in list(d.items()):
            if isinstance(v, torch.Tensor):
                d[k] = v.cuda()
        if targets:
            d["targets_modality"] = d["inputs_modality"]
            d["targets_timestamp"] = d["inputs_timestamp"]
    return md


def cosine(a, b, eps=1e-30):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + eps))


def run_curve(model, steps, B, T, n_ap, n_beh, total_steps, objectives):
    opt, sch = make_optimizer(model, total_steps)
    model.train()
    torch.manual_seed(1234)
    losses = []
    for s in range(steps):
        out = model(to_dev(O.make_mod_dict(O.synth_batch(B, T, n_ap, n_beh, seed=s), objectives[s])))
        out.loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(out.loss.detach())
    return [x.item() for x in losses]


# ---------------------------------------------------------------------------------------------- fp32 against a reference fixture
def fixture_batch(z, prefix="batch/"):
    return {k.split("/")[-1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}


def check_fixture_outputs(model, z, p, objective, prefix="batch/", seed=11):
    """One training forward + backward of `model` on the fixture's batch against the records under `p`: loss, counts (exact), token
    masks (exact), per-modality loss and predictions.  Returns the model output."""
    model.cuda().train()
    torch.manual_seed(seed)
    md = to_dev(O.make_mod_dict(fixture_batch(z, prefix), objective))
    out = model(md)
    out.loss.backward()
    print(p, "loss", out.loss.item(), "reference", float(z[f"{p}/loss"]))
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=2e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"{p}/mask/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    return out


def check_stored_grads(named, z, p, names):
    """Every gradient tensor the fixture keeps under `p`, elementwise.  Returns the names it found."""
    stored = [k for k in names if f"{p}/grad/{k}" in z.files]
    for k in stored:
        g, ref = named[k].grad.cpu().numpy(), z[f"{p}/grad/{k}"]
        np.testing.assert_allclose(g, ref, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(ref).max(), err_msg=k)
    return stored


def check_fixture_case(model, z, meta, case, objective, prefix="batch/"):
    """check_fixture_outputs, then the parameter order (and the state dict's, where the fixture records `state`), every gradient norm
    and every stored gradient tensor.  How many tensors must be stored follows the fixture's meta: with `full_grad_cases`, all of them
    for those cases under the full-gradient objective and none elsewhere; without, all of them under the full-gradient objective
    (`full_grad` is an objective, or a list of case/objective pairs).  Returns the stored names."""
    p = f"{case}/{objective}"
    check_fixture_outputs(model, z, p, objective, prefix)
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names
    if "state" in meta:
        assert list(model.state_dict()) == [k for k, _ in meta["state"][case]]
    for k, gn in zip(names, z[f"{p}/grad_norm"]):
        assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=5e-3, abs=1e-8), k
    stored = check_stored_grads(named, z, p, names)
    full = p in meta["full_grad"] if isinstance(meta["full_grad"], list) else objective == meta["full_grad"]
    if "full_grad_cases" in meta:
        assert len(stored) == (len(names) if full and case in meta["full_grad_cases"] else 0)
    else:
        assert not full or len(stored) == len(names)
    return stored


# ---------------------------------------------------------------------------------------------- resume, graph replay
def resume_roundtrip(tmp_path, mc, dtype="fp32", B=4, after_save=None, after_restore=None):
    """6 trainer steps in one go == 3 steps, save_model (module pickle + train state), brand-new model / optimiser / scheduler / trainer
    objects restored from the files (load_train_state), 3 more steps: every state-dict tensor bit for bit.  Objectives are sampled
    (Python RNG), token_masking draws masks (torch RNG) and dropout, where `mc` has any, the engine's RNG: all must continue exactly.
    after_save(checkpoint) and after_restore(model, optimizer, scheduler) hold the caller's own asserts."""
    from trainer.make import make_multimodal_trainer
    from multi_modal_foundation_model_amd.ddp import Accelerator
    T, n_ap, n_beh = 8, 12, 2

    def batches(lo, hi):
        out = []
        for i in range(lo, hi):
            b = O.synth_batch(B, T, n_ap, n_beh, seed=i)
            b["eid"] = ["synthetic"] * B
            b["neuron_regions"] = [["XX"] * B for _ in range(n_ap)]
            out.append(b)
        return out

    def make(model, loader, log_dir):
        model.compute_dtype = dtype
        acc = Accelerator()
        model = acc.prepare(model)
        opt, sch = make_optimizer(model, 40, lr=1e-3)
        tr = make_multimodal_trainer(model=model, train_dataloader=loader, eval_dataloader=[], optimizer=opt, log_dir=str(log_dir),
                                     accelerator=acc, lr_scheduler=sch, avail_mod=["ap", "behavior"], config=load_config(),
                                     modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=True,
                                     num_neurons=[n_ap])
        return model, opt, sch, tr

    # reference run: 6 steps
    m0 = build_model(mc, n_ap, n_beh, seed=7); m0.engine_seed = 5
    m0, opt0, sch0, tr0 = make(m0, batches(0, 6), tmp_path / "a")
    random.seed(42); torch.manual_seed(99)
    tr0.train_epoch(0)
    want = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    # interrupted run: 3 steps, save, fresh objects, 3 more
    m1 = build_model(mc, n_ap, n_beh, seed=7); m1.engine_seed = 5
    (tmp_path / "b").mkdir()
    m1, opt1, sch1, tr1 = make(m1, batches(0, 3), tmp_path / "b")
    random.seed(42); torch.manual_seed(99)
    tr1.train_epoch(0)
    tr1.save_model(name="last", epoch=0)
    del m1, opt1, sch1, tr1
    random.seed(0); torch.manual_seed(0)                                  # scramble every host stream
    ck = torch.load(tmp_path / "b" / "model_last.pt", weights_only=False)  # our own file (whole-module pickle, like the reference)
    if after_save:
        after_save(ck)
    m2, opt2, sch2, tr2 = make(ck["model"], batches(3, 6), tmp_path / "b")
    assert tr2.load_train_state(name="last") == 0
    if after_restore:
        after_restore(m2, opt2, sch2)
    tr2.train_epoch(1)
    assert list(m2.state_dict()) == list(want)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, want[k]), k


def graph_replay_matches_eager(monkeypatch, make_model, g, steps=5, params=False):
    """`steps` optimiser steps (5, in fp32 unless make_model() sets another compute_dtype) of make_model() at the curve fixture's shape
    `g`: with hipGraph replay (the plan runs eagerly once, is captured on the second step and replayed from the third) the losses are
    the ones of MMFM_GRAPH=0, bit for bit; params=True: so is every parameter after the last step."""
    res, final = {}, {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MMFM_GRAPH", mode)
        model = make_model().cuda()
        res[mode] = run_curve(model, steps, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], ["token_masking"] * steps)
        plan = model._engine._last
        assert (set(plan["graphs"]) == {"fwd", "bwd"}) == (mode == "1") and plan["runs"]["fwd"] == steps
        if params:
            final[mode] = {k: p.detach().clone() for k, p in model.named_parameters()}
    print("eager", res["0"], "graph", res["1"])
    assert res["0"] == res["1"] and all(np.isfinite(res["0"]))
    for k, v in final.get("0", {}).items():
        assert torch.equal(final["1"][k], v), k


# ---------------------------------------------------------------------------------------------- one step against the fp64 oracle
def engine_step_and_oracle(mc, n_ap, n_beh, batch, objective, dtype, model_seed, embed=None, oracle_dtype=torch.float64):
    """One training step of the HIP engine, then the fp64 oracle (on the GPU, plain torch) with the step's token masks and dropout
    multipliers (tests/dropout_refs.py); `embed` stands in for oracle.mm_oracle.embed where the model's tokeniser is not the default
    one.  oracle_dtype = torch.float32 runs the oracle itself in single precision on the same inputs, masks and multipliers: what plain
    fp32 torch is off the fp64 oracle by.  Returns the model output, {name: grad}, the oracle's output dict, {name: oracle grad} and
    the engine."""
    from multi_modal_foundation_model_amd import ops as K
    model = build_model(mc, n_ap, n_beh, seed=model_seed)
    model.compute_dtype = dtype
    model.engine_seed = 77
    model.cuda().train()
    torch.manual_seed(5)
    md = to_dev(O.make_mod_dict(batch, objective))
    out = model(md)
    out.loss.backward()
    torch.cuda.synchronize()
    eng = model._engine
    B, T = batch["spikes_data"].shape[:2]
    mults = {k: v.cuda() for k, v in DR.collect_step_multipliers(K, eng, B, T).items()} if eng._sites else {}
    cfg = O.OracleCfg.from_model_config(mc, {"ap": n_ap, "behavior": n_beh})
    sd = O.share_mod_emb({k: v.detach().to(oracle_dtype).clone() for k, v in model.state_dict().items()}, cfg)
    keys = O.trainable_keys(sd, cfg)
    for k in keys:
        sd[k].requires_grad_(True)
    ref_md = O.make_mod_dict(batch, objective)
    for m, d in ref_md.items():
        for k, v in list(d.items()):
            if isinstance(v, torch.Tensor):
                d[k] = v.cuda().to(oracle_dtype) if v.is_floating_point() else v.cuda()
        d["eval_mask"] = md[m]["inputs_mask"][:, :, None].to(torch.int64)          # the token masks the step ran with
    used = set()
    with mock.patch.object(O, "embed", embed) if embed else contextlib.nullcontext():
        ref = O.forward(sd, ref_md, cfg, training=True, dropout_fn=DR.oracle_dropout_fn(mults, used))
    assert used == set(mults), sorted(set(mults) ^ used)                           # every site of the engine is a site of the model
    grads = dict(zip(keys, torch.autograd.grad(ref["loss"], [sd[k] for k in keys])))
    named = {k: p.grad for k, p in model.named_parameters()}
    assert set(named) == set(keys)
    return out, named, ref, grads, eng


def bf16_stats(out, named, ref, grads):
    """Worst loss error, gradient cosine (tensors of >= 256 / < 256 elements) and norm ratio error over all tensors but key.bias
    (softmax is invariant to a key bias: its true gradient is 0)."""
    st = dict(loss=abs(out.loss.item() / ref["loss"].item() - 1), cos_big=1.0, cos_small=1.0, norm=0.0)
    for k, g in named.items():
        r = grads[k]
        if k.endswith("key.bias"):
            continue
        if float(r.abs().max()) == 0:
            assert float(g.abs().max()) == 0, k
            continue
        c = cosine(g, r)
        which = "cos_big" if r.numel() >= 256 else "cos_small"
        if c < st[which]:
            st[which], st[which + "_at"] = c, k
        n = abs(g.double().norm().item() / r.norm().item() - 1)
        if n > st["norm"]:
            st["norm"], st["norm_at"] = n, k
    return st


def check_bf16(st, what):
    print(f"{what}: {st}")
    assert st["loss"] < 2e-2, (what, st)
    assert st["cos_big"] > 0.995 and st["cos_small"] > 0.98, (what, st)
    assert st["norm"] < 5e-2, (what, st)
