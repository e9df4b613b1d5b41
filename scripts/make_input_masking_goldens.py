#!/usr/bin/env python3
"""Generate the input-masking (mask_type: input) fixtures under tests/golden/ from the reference's own pieces.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.  Nothing of the mirror is imported.

The reference's own `MultiModal.forward` cannot run this branch: `mask` is never bound on it (mm.py:256-272).  So `ref_forward` calls
the reference's public pieces in the order mm.py:245-300 calls them - Masker, encoder_embeddings[mod], forward_mask_encoder,
decoder_embeddings[mod].forward_embed, forward_mask_decoder, forward_encoder, decoder_proj_context, forward_decoder, out_proj,
forward_loss - with the one missing line bound as `mask = zeros & inputs_attn_mask`, and leaves a modality without region information
alone under inter-region / intra-region (the reference's masker asserts there): inputs untouched, no draw, an all-zero spike_mask.

    python scripts/make_input_masking_goldens.py

input_masking_fwd_bwd.npz  per case of tests/input_masking.py CASES (tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0, B = 3,
                           T = 8, 12 neurons in 3 regions, 2 behaviours; model seed 7, data seed 3, masker seed 11 for torch and `random`):
                           loss, per-modality loss / n / preds / spike_mask (the target mask) / staged inputs (the corrupted inputs), the
                           corruption mask where zero_ratio is 1 (read off an all-ones probe on the same streams), every gradient norm;
                           every gradient tensor in full for FULL_GRAD; the batches; the parameter names and initial parameters by hash.
input_masking_curve.json   50 AdamW + OneCycle steps, the mode sampled per step from CURVE_MODES as the trainer samples it, step s on
                           the batch of data seed s.
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

import input_masking as IM  # noqa: E402
from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)


def build_model(case=None):
    model = G.build_model(G.tiny_model_cfg(max_F=IM.TINY["max_F"]), IM.TINY["n_ap"], IM.TINY["n_beh"], IM.MODEL_SEED)
    IM.set_masker(model.masker, case)
    model.train()
    return model


def probe_cm(model, x, reg):
    """The corruption mask of the masker's next call (zero_ratio 1: exactly the zeroed elements of an all-ones tensor), read on copies of
    the torch and `random` streams, which are put back."""
    st, rs = torch.get_rng_state(), random.getstate()
    out, _ = model.masker(torch.ones_like(x), reg)
    torch.set_rng_state(st)
    random.setstate(rs)
    return (out == 0).to(torch.uint8)


def ref_forward(model, md, mode, rec=None):
    """mm.py:245-300 on this branch, see the module docstring.  rec: a dict that takes the masks."""
    for mod, d in md.items():
        B, T, N = d["inputs"].shape
        reg = d["inputs_regions"] if mod == "ap" else None
        model.masker.mode = mode
        if mode in IM.REGION_MODES and reg is None:
            d["spike_mask"] = torch.zeros(B, T, N, dtype=torch.int64)
            cm = torch.zeros(B, T, N, dtype=torch.uint8)
        else:
            cm = probe_cm(model, d["inputs"], reg) if float(model.masker.zero_ratio) == 1.0 else None
            d["inputs"], d["spike_mask"] = model.masker(d["inputs"].clone(), reg)
        if rec is not None:
            rec[mod] = dict(cm=cm, tm=d["spike_mask"], inputs=d["inputs"].clone())
        mask = torch.zeros_like(d["inputs_attn_mask"]) & d["inputs_attn_mask"]
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
    return model.forward_loss(dec, target_gts)


def record_case(arrs, meta, case):
    model = build_model(case)
    G.init_by_hash(arrs, meta, case, model)
    batch = IM.case_batch(case)
    for mod, d in batch.items():
        for k, v in d.items():
            arrs[f"batch/{case}/{mod}/{k}"] = G.npify(v)
    torch.manual_seed(IM.MASKER_SEED)
    random.seed(IM.MASKER_SEED)
    rec = {}
    loss, mod_loss, mod_n, mod_preds, _ = ref_forward(model, IM.make_mod_dict(batch, IM.CASES[case]["mode"]), IM.CASES[case]["mode"], rec)
    loss.backward()
    arrs[f"{case}/loss"] = G.npify(loss)
    for mod in ("ap", "behavior"):
        arrs[f"{case}/mod_loss/{mod}"] = G.npify(mod_loss[mod])
        arrs[f"{case}/n/{mod}"] = G.npify(mod_n[mod])
        arrs[f"{case}/preds/{mod}"] = G.npify(mod_preds[mod])
        arrs[f"{case}/tm/{mod}"] = G.npify(rec[mod]["tm"]).astype(np.uint8)
        arrs[f"{case}/inputs/{mod}"] = G.npify(rec[mod]["inputs"])
        if rec[mod]["cm"] is not None:
            arrs[f"{case}/cm/{mod}"] = G.npify(rec[mod]["cm"])
    arrs[f"{case}/grad_norm"] = np.array([float(p.grad.double().norm()) for _, p in model.named_parameters()])
    if case in IM.FULL_GRAD:
        for k, p in model.named_parameters():
            arrs[f"{case}/grad/{k}"] = G.npify(p.grad)
    print("   ", case, float(loss), {m: int(v) for m, v in mod_n.items()})


def curve(steps=IM.CURVE_STEPS):
    model = build_model()
    opt, sch = G.make_opt(model, steps)
    random.seed(42)
    torch.manual_seed(1234)
    losses, modes = [], []
    for step in range(steps):
        mode = random.sample(IM.CURVE_MODES, 1)[0]
        loss = ref_forward(model, IM.make_mod_dict(IM.case_batch(seed=step), mode), mode)[0]
        loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(float(loss))
        modes.append(mode)
    print("    curve", losses[:2], "...", losses[-1])
    return dict(loss=losses, mode=modes, model_seed=IM.MODEL_SEED, total_steps=steps, B=IM.TINY["B"])


if __name__ == "__main__":
    meta = dict(IM.TINY, H=32, heads=4, inter=64, model_seed=IM.MODEL_SEED, data_seed=IM.DATA_SEED, masker_seed=IM.MASKER_SEED,
                cases=list(IM.CASES), full_grad=list(IM.FULL_GRAD), state={}, params={}, init={})
    arrs = {}
    for case in IM.CASES:
        record_case(arrs, meta, case)
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("input_masking_fwd_bwd.npz", **arrs)
    G.save_json("input_masking_curve.json", curve())
