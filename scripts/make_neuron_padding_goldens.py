#!/usr/bin/env python3
"""Generate the neuron-padding (space_attn_mask honoured) fixtures under tests/golden/ from the reference's own pieces.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.  Nothing of the mirror is imported.

The reference never reads space_attn_mask, so `ref_forward` calls its public pieces in the order mm.py:245-300 calls them - Masker,
encoder_embeddings[mod], forward_mask_encoder, decoder_embeddings[mod].forward_embed, forward_mask_decoder, forward_encoder,
decoder_proj_context, forward_decoder, out_proj - with two changes: the inputs of a modality that carries the mask have their padded
channels zeroed (behind the masker's call, which sees the batch as the loader left it and draws over all N channels), and the loss
is forward_loss's own expression with the channel mask as one more factor,
    loss_mod = (self.loss_mod[mod](preds, targets) * m[:, :, None] * v[:, None, :]).sum(),  n = (m[:, :, None] * v[:, None, :]).sum(),
m the [B, T] token mask (or, for an input-masking mode, the masker's [B, T, N] spike_mask in its place).

    python scripts/make_neuron_padding_goldens.py

neuron_padding_fwd_bwd.npz  per case of tests/neuron_padding.py CASES (tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0,
                            B = 3, T = 8, 12 neurons, 2 behaviours; model seed 7, data seed 3, masker seed 11 for torch and `random`):
                            loss, per-modality loss / n / preds / token mask / loss mask / staged inputs, every gradient norm, every
                            gradient tensor in full for FULL_GRAD; the batches and channel masks; parameter names and initial
                            parameters by hash.  The im_real_draw* cases run the masker at zero_ratio 0.5: it corrupts the inputs
                            itself, and the staged inputs are its output with the padded channels zeroed.
neuron_padding_curve.json   50 AdamW + OneCycle steps over three sessions of 12 / 9 / 6 neurons (step s: session s % 3, data seed s),
                            the objective sampled per step as the trainer samples it.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import neuron_padding as NP  # noqa: E402
from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)


def build_model(case=None):
    model = G.build_model(G.tiny_model_cfg(max_F=NP.TINY["max_F"]), NP.TINY["n_ap"], NP.TINY["n_beh"], NP.MODEL_SEED)
    NP.set_masker(model.masker, case)
    model.train()
    return model


def ref_forward(model, md, rec=None):
    """mm.py:245-300 with the channel mask honoured, see the module docstring.  rec: a dict that takes the masks and the staged inputs."""
    chan = {}
    for mod, d in md.items():
        reg = d["inputs_regions"] if mod == "ap" else None
        if d["masking_mode"]:
            model.masker.mode = d["masking_mode"]
            d["inputs"], d["spike_mask"] = model.masker(d["inputs"].clone(), reg)
            mask = torch.zeros_like(d["inputs_attn_mask"]) & d["inputs_attn_mask"]
        else:
            if d["eval_mask"] is None:
                _, mask = model.masker(d["inputs"].clone(), reg)
            else:
                mask = d["eval_mask"]
            mask = mask[:, :, 0] & d["inputs_attn_mask"]
        v = d.get("space_attn_mask")
        if v is not None:
            chan[mod] = v
            d["inputs"] = torch.where(v[:, None, :] != 0, d["inputs"], torch.zeros_like(d["inputs"]))
        d["inputs_mask"] = d["targets_mask"] = mask
        d["encoder_attn_mask"] = d["decoder_attn_mask"] = d["inputs_attn_mask"]
    enc = {mod: model.encoder_embeddings[mod](d) for mod, d in md.items() if mod in model.encoder_embeddings}
    encoder_tokens, encoder_emb, _, encoder_attn_mask, _ = model.forward_mask_encoder(enc)
    dec = {mod: model.decoder_embeddings[mod].forward_embed(d) for mod, d in md.items() if mod in model.decoder_embeddings}
    decoder_tokens, target_gts, decoder_emb, _, decoder_attn_mask, decoder_mod_mask = model.forward_mask_decoder(dec)
    x = model.forward_encoder(encoder_tokens + encoder_emb, encoder_attn_mask=encoder_attn_mask)
    context = model.decoder_proj_context(x) + encoder_emb
    y = model.forward_decoder(decoder_tokens + decoder_emb, context, encoder_attn_mask=encoder_attn_mask, decoder_attn_mask=decoder_attn_mask)
    dec = {mod: model.decoder_embeddings[mod].out_proj(model.mod_to_indx[mod], d, y, decoder_mod_mask, len(model.avail_mod))
           for mod, d in dec.items()}
    mod_loss, mod_n, mod_preds = {}, {}, {}
    for mod, d in dec.items():                        # forward_loss (mm.py:217-239) with v as one more factor
        targets = target_gts[mod]
        B, T, N = targets.size()
        w = d["spike_mask"] if "spike_mask" in d else d["targets_mask"].unsqueeze(-1).expand(B, T, N)
        if mod in chan:
            w = w * chan[mod][:, None, :]
        mod_loss[mod] = (model.loss_mod[mod](d["preds"], targets) * w).sum()
        mod_n[mod] = w.sum()
        mod_preds[mod] = d["preds"]
        if rec is not None:
            rec[mod] = dict(w=w, mask=md[mod]["inputs_mask"], inputs=md[mod]["inputs"].clone())
    return sum(mod_loss.values()) / sum(mod_n.values()), mod_loss, mod_n, mod_preds


def record_case(arrs, meta, case):
    model = build_model(case)
    G.init_by_hash(arrs, meta, case, model)
    batch, v = NP.case_batch(case)
    for mod, d in batch.items():
        for k, t in d.items():
            arrs[f"batch/{case}/{mod}/{k}"] = G.npify(t)
    arrs[f"batch/{case}/space_attn_mask"] = G.npify(v)
    torch.manual_seed(NP.MASKER_SEED)
    random.seed(NP.MASKER_SEED)
    rec = {}
    loss, mod_loss, mod_n, mod_preds = ref_forward(model, NP.case_mod_dict(case, batch, v), rec)
    loss.backward()
    arrs[f"{case}/loss"] = G.npify(loss)
    for mod in ("ap", "behavior"):
        arrs[f"{case}/mod_loss/{mod}"] = G.npify(mod_loss[mod])
        arrs[f"{case}/n/{mod}"] = G.npify(mod_n[mod])
        arrs[f"{case}/preds/{mod}"] = G.npify(mod_preds[mod])
        arrs[f"{case}/mask/{mod}"] = G.npify(rec[mod]["mask"])
        arrs[f"{case}/w/{mod}"] = G.npify(rec[mod]["w"]).astype(np.uint8)
        arrs[f"{case}/inputs/{mod}"] = G.npify(rec[mod]["inputs"])
    arrs[f"{case}/grad_norm"] = np.array([float(p.grad.double().norm()) for _, p in model.named_parameters()])
    if case in NP.FULL_GRAD:
        for k, p in model.named_parameters():
            arrs[f"{case}/grad/{k}"] = G.npify(p.grad)
    print("   ", case, float(loss), {m: int(n) for m, n in mod_n.items()})


def curve(steps=NP.CURVE_STEPS):
    model = build_model()
    opt, sch = G.make_opt(model, steps)
    random.seed(42)
    torch.manual_seed(1234)
    losses, objs = [], []
    for step in range(steps):
        obj = random.sample(list(G.OBJECTIVES), 1)[0]
        batch, v = NP.curve_batch(step)
        loss = ref_forward(model, NP.make_mod_dict(batch, v, obj))[0]
        loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(float(loss))
        objs.append(obj)
    print("    curve", losses[:2], "...", losses[-1])
    return dict(loss=losses, objective=objs, sessions=list(NP.CURVE_SESSIONS), model_seed=NP.MODEL_SEED, total_steps=steps, B=NP.TINY["B"])


if __name__ == "__main__":
    meta = dict(NP.TINY, H=32, heads=4, inter=64, model_seed=NP.MODEL_SEED, data_seed=NP.DATA_SEED, masker_seed=NP.MASKER_SEED,
                cases=list(NP.CASES), full_grad=list(NP.FULL_GRAD), state={}, params={}, init={})
    arrs = {}
    for case in NP.CASES:
        record_case(arrs, meta, case)
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("neuron_padding_fwd_bwd.npz", **arrs)
    G.save_json("neuron_padding_curve.json", curve())
