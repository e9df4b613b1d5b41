"""embedder.act / pos / bias on the MI355X, whole models: the fp32 engine against the reference's own forward / backward and 50-step curves
(tests/golden/embedder_opts_*, scripts/make_embedder_goldens.py); the bf16 engine against an fp64 restatement (the tokeniser written here,
the rest oracle/mm_oracle.py) at the tiny size and at the default widths; one dropout-on step without position tables against the same
restatement fed the step's own masks; checkpoint resume and hipGraph replay of a non-default embedder model."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_refs as DR
from conftest import load_json
from embedder_opts import CASES, OBJECTIVES, case_config, fixture
from helpers import build_model, make_optimizer
from oracle import mm_oracle as O
from side_config import sides

pytestmark = pytest.mark.gpu
K_TANH = (2.0 / np.pi) ** 0.5


def to_dev(md):
    for d in md.values():
        for k, v in list(d.items()):
            if isinstance(v, torch.Tensor):
                d[k] = v.cuda()
        d["targets_modality"] = d["inputs_modality"]
        d["targets_timestamp"] = d["inputs_timestamp"]
    return md


def cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------- fp32 against the reference
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_tiny_forward_backward_vs_reference_fixture(case, objective):
    """Loss, counts (exact), predictions, every gradient norm and (the full-gradient cases / token_masking) every gradient tensor; the
    quantities and tolerances of test_side_config_model_gpu.py::test_tiny_forward_backward_vs_reference_fixture."""
    z, meta = fixture()
    model = build_model(case_config(case), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    model.cuda().train()
    batch = {k.split("/")[-1]: torch.from_numpy(z[k]) for k in z.files if k.startswith("batch/")}
    torch.manual_seed(11)
    md = to_dev(O.make_mod_dict(batch, objective))
    out = model(md)
    out.loss.backward()
    p = f"{case}/{objective}"
    print(p, "loss", out.loss.item(), "reference", float(z[f"{p}/loss"]))
    assert out.loss.item() == pytest.approx(float(z[f"{p}/loss"]), rel=2e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(z[f"{p}/n/{m}"])
        np.testing.assert_array_equal(md[m]["inputs_mask"].cpu().numpy(), z[f"{p}/mask/{m}"])
        assert out.mod_loss[m].item() == pytest.approx(float(z[f"{p}/mod_loss/{m}"]), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), z[f"{p}/preds/{m}"], rtol=1e-4, atol=2e-5)
    names = meta["params"][case]
    named = dict(model.named_parameters())
    assert list(named) == names
    assert list(model.state_dict()) == [k for k, _ in meta["state"][case]]
    for k, gn in zip(names, z[f"{p}/grad_norm"]):
        assert float(named[k].grad.double().norm()) == pytest.approx(float(gn), rel=5e-3, abs=1e-8), k
    stored = [k for k in names if f"{p}/grad/{k}" in z.files]
    assert len(stored) == (len(names) if objective == meta["full_grad"] and case in meta["full_grad_cases"] else 0)
    for k in stored:
        g, ref = named[k].grad.cpu().numpy(), z[f"{p}/grad/{k}"]
        np.testing.assert_allclose(g, ref, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(ref).max(), err_msg=k)


def run_curve(model, steps, Bc, Tc, n_ap, n_beh, total_steps, objectives):
    opt, sch = make_optimizer(model, total_steps)
    model.train()
    torch.manual_seed(1234)
    losses = []
    for s in range(steps):
        out = model(to_dev(O.make_mod_dict(O.synth_batch(Bc, Tc, n_ap, n_beh, seed=s), objectives[s])))
        out.loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(out.loss.detach())
    return [x.item() for x in losses]


@pytest.mark.parametrize("case", ["ASYM", "GELU"])
def test_loss_curve_tiny_50_steps_vs_reference_fixture(case):
    g = load_json("embedder_opts_curve.json")[case]
    model = build_model(case_config(case), g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    assert len(model.state_dict()) == g["n_state_keys"]
    losses = run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    print("max relative gap", float(np.max(np.abs(np.array(losses) / np.array(g["loss"]) - 1))))
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


# ---------------------------------------------------------------------------------------------- the fp64 restatement
def act_ref(name, u):
    if name == "softsign":
        return u / (1 + u.abs())
    if name in ("identity", "linear"):
        return u
    if name == "relu":
        return torch.relu(u)
    if name == "gelu":
        return F.gelu(u)
    if name in ("silu", "swish", "quick_gelu"):
        return u * torch.sigmoid((1.702 if name == "quick_gelu" else 1.0) * u)
    if name in ("gelu_new", "gelu_pytorch_tanh", "gelu_fast"):
        return 0.5 * u * (1 + torch.tanh(K_TANH * (u + 0.044715 * u ** 3)))
    assert name == "tanh", name
    return torch.tanh(u)


def embed_ref(mc):
    """The tokeniser of the reference (encoder_embeddings.py:44-61 and its decoder twin) restated for a model config `mc`, with the
    signature of oracle.mm_oracle.embed: the side's act, scale, pos and bias come from its own `embedder` section."""
    def embed(sd, p, inputs, ts, mod_idx, cfg, training, gen=None, dropout_fn=None, site_key=None):
        e = mc[p.split("_", 1)[0]]["embedder"]
        scale = cfg.hidden ** 0.5 if e["scale"] is None else e["scale"]
        x = F.linear(inputs, sd[p + ".token_embed.weight"], sd[p + ".token_embed.bias"] if e["bias"] else None)
        x = F.linear(act_ref(e["act"], x) * scale, sd[p + ".projection.weight"], sd[p + ".projection.bias"])
        B, T, _ = inputs.shape
        emb = sd[p + ".mod_emb.weight"][mod_idx][None, None, :].expand(B, T, -1).clone()
        if e["pos"]:
            emb = emb + sd[p + ".pos_embed.weight"][ts]
        return O.dropout(x, e["dropout"], training, dropout_fn, site_key), emb
    return embed


def engine_step_and_restatement(monkeypatch, mc, n_ap, n_beh, batch, objective, dtype, model_seed):
    """One training step of the HIP engine, then the fp64 restatement (on the GPU, plain torch) with the step's token masks and dropout
    multipliers, as tests/test_dropout_step_gpu.py::engine_step_and_oracle does for the softsign model."""
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
    sd = O.share_mod_emb({k: v.detach().double().clone() for k, v in model.state_dict().items()}, cfg)
    keys = O.trainable_keys(sd, cfg)
    for k in keys:
        sd[k].requires_grad_(True)
    ref_md = O.make_mod_dict(batch, objective)
    for m, d in ref_md.items():
        for k, v in list(d.items()):
            if isinstance(v, torch.Tensor):
                d[k] = v.cuda().double() if v.is_floating_point() else v.cuda()
        d["eval_mask"] = md[m]["inputs_mask"][:, :, None].to(torch.int64)          # the token masks the step ran with
    monkeypatch.setattr(O, "embed", embed_ref(mc))
    used = set()
    ref = O.forward(sd, ref_md, cfg, training=True, dropout_fn=DR.oracle_dropout_fn(mults, used))
    assert used == set(mults), sorted(set(mults) ^ used)
    grads = dict(zip(keys, torch.autograd.grad(ref["loss"], [sd[k] for k in keys])))
    named = {k: p.grad for k, p in model.named_parameters()}
    assert set(named) == set(keys)
    return out, named, ref, grads, eng


def bf16_stats(out, named, ref, grads):
    """Worst loss error, gradient cosine (tensors of >= 256 / < 256 elements) and norm ratio error over all tensors but key.bias (its
    true gradient is 0): tests/test_dropout_step_gpu.py::bf16_stats."""
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


ASYM = dict(enc_emb=dict(act="tanh", pos=False, bias=False, scale=None))
BF16_MODELS = {"softsign": {}, "ASYM": ASYM, "GELU": dict(enc_emb=dict(act="gelu"), dec_emb=dict(act="gelu"))}
# (B, T, n_ap, model_config keywords): the tiny size; the default widths (H 256, 668 neurons: the K = 668 / 1336 tokeniser GEMMs)
BF16_SIZES = {"tiny": (2, 8, 12, dict(H=32, heads=4, inter=64, n_enc=1, n_dec=1, max_F=8)), "default_widths": (4, 100, 668, dict(n_enc=1, n_dec=1))}


@pytest.mark.parametrize("size", list(BF16_SIZES))
@pytest.mark.parametrize("name", list(BF16_MODELS))
def test_bf16_step_vs_fp64_restatement(monkeypatch, name, size):
    """One bf16 training step (dropout 0) against the fp64 restatement at the bound tests/test_dropout_step_gpu.py::check_bf16 holds the
    softsign model to: loss within 2e-2, worst gradient cosine > 0.995 (> 0.98 under 256 elements), worst norm error < 5e-2.  `softsign`
    is the default model in the same run, the yardstick for what the saved bf16 pre-activation of the other activations costs."""
    B, T, n_ap, kw = BF16_SIZES[size]
    mc = sides(dropout=0.0, emb_dropout=0.0, **BF16_MODELS[name], **kw)
    batch = O.synth_batch(B, T, n_ap, 2, seed=6)
    out, named, ref, grads, eng = engine_step_and_restatement(monkeypatch, mc, n_ap, 2, batch, "token_masking", "bf16", 3)
    st = bf16_stats(out, named, ref, grads)
    print(f"bf16 {name} {size}: {st}")
    if name != "softsign":      # the forward stores z, the backward reads it: the plan's buffers say so
        want_z = {"ASYM": {"encoder/z/0", "encoder/z/1"}, "GELU": {f"{s}/z/{m}" for s in ("encoder", "decoder") for m in (0, 1)}}[name]
        assert {k for k in eng._last["b"] if "/z/" in k and not k.startswith("d/")} == want_z
    assert st["loss"] < 2e-2, st
    assert st["cos_big"] > 0.995 and st["cos_small"] > 0.98, st
    assert st["norm"] < 5e-2, st


# ---------------------------------------------------------------------------------------------- dropout, resume, graph replay
def test_fp32_dropout_step_without_position_tables(monkeypatch):
    """fp32, tiny, dropout 0.4 / embedder dropout 0.2, pos: false on both sides and a bias-free relu tokeniser on the decoder: the keep
    masks are read off the kernels (tests/dropout_refs.py) and fed to the fp64 restatement; loss, predictions and every gradient at the
    bounds of test_dropout_step_gpu.py::test_fp32_dropout_step_vs_oracle_fed_the_steps_masks."""
    kw = dict(H=32, heads=4, inter=64, n_enc=1, n_dec=1, max_F=8, dropout=0.4, emb_dropout=0.2)
    mc = sides(enc_emb=dict(pos=False), dec_emb=dict(pos=False, bias=False, act="relu"), **kw)
    batch = O.synth_batch(3, 8, 12, 2, seed=4, pad=[0, 3, 1])
    out, named, ref, grads, eng = engine_step_and_restatement(monkeypatch, mc, 12, 2, batch, "token_masking", "fp32", 0)
    assert len(eng.dropout_sites(3, 8)) == 4 + 3 + 5
    assert not any("pos_embed" in k for k in named) and "decoder_embeddings.ap.embedder.token_embed.bias" not in named
    assert out.loss.item() == pytest.approx(ref["loss"].item(), rel=2e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == int(ref["mod_n_examples"][m])
        assert out.mod_loss[m].item() == pytest.approx(ref["mod_loss"][m].item(), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), ref["mod_preds"][m].detach().cpu().numpy(), rtol=1e-4, atol=2e-5)
    for k, g in named.items():
        r = grads[k].cpu().numpy()
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(r).max(), err_msg=k)


def test_asym_case_resume_from_train_state_is_bit_identical(tmp_path):
    """The ASYM tiny model in fp32: 6 steps in one go == 3 steps, save_model + save_train_state, fresh objects restored from the files
    (load_train_state), 3 more steps."""
    from trainer.make import make_multimodal_trainer
    from multi_modal_foundation_model_amd.ddp import Accelerator
    from helpers import load_config
    Bc, Tc, n_ap, n_beh = 2, 8, 12, 2
    mc = case_config("ASYM", n_enc=2, n_dec=2)

    def batches(lo, hi):
        out = []
        for i in range(lo, hi):
            b = O.synth_batch(Bc, Tc, n_ap, n_beh, seed=i)
            b["eid"] = ["synthetic"] * Bc
            b["neuron_regions"] = [["XX"] * Bc for _ in range(n_ap)]
            out.append(b)
        return out

    def make(model, loader, log_dir):
        model.compute_dtype = "fp32"
        acc = Accelerator()
        model = acc.prepare(model)
        opt, sch = make_optimizer(model, 40, lr=1e-3)
        tr = make_multimodal_trainer(model=model, train_dataloader=loader, eval_dataloader=[], optimizer=opt, log_dir=str(log_dir),
                                     accelerator=acc, lr_scheduler=sch, avail_mod=["ap", "behavior"], config=load_config(),
                                     modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=True,
                                     num_neurons=[n_ap])
        return model, opt, sch, tr

    m0 = build_model(mc, n_ap, n_beh, seed=7); m0.engine_seed = 5
    m0, opt0, sch0, tr0 = make(m0, batches(0, 6), tmp_path / "a")
    random.seed(42); torch.manual_seed(99)
    tr0.train_epoch(0)
    want = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    m1 = build_model(mc, n_ap, n_beh, seed=7); m1.engine_seed = 5
    (tmp_path / "b").mkdir()
    m1, opt1, sch1, tr1 = make(m1, batches(0, 3), tmp_path / "b")
    random.seed(42); torch.manual_seed(99)
    tr1.train_epoch(0)
    tr1.save_model(name="last", epoch=0)
    del m1, opt1, sch1, tr1
    random.seed(0); torch.manual_seed(0)
    ck = torch.load(tmp_path / "b" / "model_last.pt", weights_only=False)
    keys = list(ck["model"].state_dict())
    assert "encoder_embeddings.ap.embedder.pos_embed.weight" not in keys and "decoder_embeddings.ap.embedder.pos_embed.weight" in keys
    assert "encoder_embeddings.ap.embedder.token_embed.bias" not in keys
    m2, opt2, sch2, tr2 = make(ck["model"], batches(3, 6), tmp_path / "b")
    assert tr2.load_train_state(name="last") == 0
    enc, dec = (m2._engine.cfg.side(s) for s in ("encoder", "decoder"))
    assert (enc.embed_act, enc.embed_pos, enc.embed_bias, dec.embed_act, dec.embed_pos, dec.embed_bias) == ("tanh", False, False, "softsign", True, True)
    tr2.train_epoch(1)
    assert list(m2.state_dict()) == list(want)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_asym_case_graph_replay_gives_the_eager_losses(monkeypatch):
    """The ASYM tiny model, 5 optimiser steps in fp32: with hipGraph replay (the plan runs eagerly once, is captured on the second step and
    replayed from the third) the losses are the ones of MMFM_GRAPH=0, bit for bit."""
    g = load_json("embedder_opts_curve.json")["ASYM"]
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MMFM_GRAPH", mode)
        model = build_model(case_config("ASYM"), g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
        res[mode] = run_curve(model, 5, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], ["token_masking"] * 5)
        plan = model._engine._last
        assert (set(plan["graphs"]) == {"fwd", "bwd"}) == (mode == "1") and plan["runs"]["fwd"] == 5
    print("eager", res["0"], "graph", res["1"])
    assert res["0"] == res["1"] and all(np.isfinite(res["0"]))
