#!/usr/bin/env python3
"""Generate the per-session layer (use_session) fixtures under tests/golden/ from the reference's own pieces.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.  Nothing of the mirror is imported.

The reference has no session layers.  `ref_forward` calls its public pieces, built with n_channel = P, in the order mm.py:245-300 calls
them - Masker (on the padded batch, as the loader left it), encoder_embeddings[mod], forward_mask_encoder,
decoder_embeddings[mod].forward_embed, forward_mask_decoder, forward_encoder, decoder_proj_context, forward_decoder, out_proj - with the
plain-torch restatement of the two layers (tests/session_stitch.py: per sample, the nn.Linear weights of the sample's session) in front
of the tokenisers and behind the head, and forward_loss's own expression with v[b, c] = c < n_s(b) as one more factor.

    python scripts/make_session_stitch_goldens.py

session_stitch_fwd_bwd.npz   per case of tests/session_stitch.py CASES and XCASES (modality segments T = (8, 5); input masking in the temporal and
                             neuron modes, the masker set as tests/input_masking.py sets it) (tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0, B 4,
                             T 8, N_max 12, P 8; model seed 7, data seed 3, masker seed 11): loss, per-modality loss / n / preds / token
                             mask, every gradient norm (NaN for a session absent from the batch: its .grad is None), the session layers'
                             gradients, and every gradient tensor for FULL_GRAD; the batch; parameter names and initial parameters by hash.
session_stitch_curve.json    50 AdamW + OneCycle steps with the three sessions taken in turn (step s: session s % 3, data seed s), then 17
                             optimiser steps of 3 micro-batches each (micro-batch j: session j, loss / 3), the objective sampled per
                             (micro-)batch as the trainer samples it.
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

import session_stitch as R  # noqa: E402
from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

T_ = R.TINY
SIZES = list(R.SESSIONS.values())


class Stitched(torch.nn.Module):
    """The reference model at n_channel = P with the session layers created behind everything it creates."""

    def __init__(self, bias=True):
        super().__init__()
        self.model = G.build_model(G.tiny_model_cfg(max_F=T_["max_F"]), T_["P"], T_["n_beh"], R.MODEL_SEED)
        self.layers = R.RefLayers(SIZES, T_["P"], bias)

    def named(self):
        """Parameters under the names the mirror gives them."""
        return [(k.split(".", 1)[1], p) for k, p in self.named_parameters()]


def ref_forward(st, md, eids):
    model, sid = st.model, [R.EIDS.index(e) for e in eids]
    for mod, d in md.items():
        reg = d["inputs_regions"] if mod == "ap" else None
        if d["masking_mode"]:             # input masking, as upstream evidently meant the branch (mm.py:256-272): no token is masked
            model.masker.mode = d["masking_mode"]
            d["inputs"], d["spike_mask"] = model.masker(d["inputs"].clone(), reg)
            mask = torch.zeros_like(d["inputs_attn_mask"]) & d["inputs_attn_mask"]
        else:
            if d["eval_mask"] is None:
                _, mask = model.masker(d["inputs"].clone(), reg)      # on the padded batch: the generator stream is the unstitched model's
            else:
                mask = d["eval_mask"]
            mask = mask[:, :, 0] & d["inputs_attn_mask"]
        d["inputs_mask"] = d["targets_mask"] = mask
        d["encoder_attn_mask"] = d["decoder_attn_mask"] = d["inputs_attn_mask"]
    N, padded = md["ap"]["inputs"].shape[-1], md["ap"]["targets"]
    md["ap"]["inputs"] = R.read_in(md["ap"]["inputs"], sid, SIZES, *st.layers.tensors("in"))
    md["ap"]["targets"] = torch.zeros_like(md["ap"]["inputs"])
    enc = {mod: model.encoder_embeddings[mod](d) for mod, d in md.items()}
    encoder_tokens, encoder_emb, _, encoder_attn_mask, _ = model.forward_mask_encoder(enc)
    dec = {mod: model.decoder_embeddings[mod].forward_embed(d) for mod, d in md.items()}
    decoder_tokens, target_gts, decoder_emb, _, decoder_attn_mask, decoder_mod_mask = model.forward_mask_decoder(dec)
    x = model.forward_encoder(encoder_tokens + encoder_emb, encoder_attn_mask=encoder_attn_mask)
    context = model.decoder_proj_context(x) + encoder_emb
    y = model.forward_decoder(decoder_tokens + decoder_emb, context, encoder_attn_mask=encoder_attn_mask, decoder_attn_mask=decoder_attn_mask)
    dec = {mod: model.decoder_embeddings[mod].out_proj(model.mod_to_indx[mod], d, y, decoder_mod_mask, len(model.avail_mod)) for mod, d in dec.items()}
    mod_loss, mod_n, mod_preds = {}, {}, {}
    for mod, d in dec.items():                        # forward_loss (mm.py:217-239), with v as one more factor for the stitched modality
        preds, targets = d["preds"], target_gts[mod]
        if mod == "ap":
            preds, targets = R.read_out(preds, sid, SIZES, *st.layers.tensors("out"), N), padded
        B, T, C = targets.size()
        w = md[mod]["spike_mask"] if "spike_mask" in md[mod] else d["targets_mask"].unsqueeze(-1).expand(B, T, C)
        if mod == "ap":
            w = w * R.channel_mask(sid, SIZES, N)[:, None, :]
        mod_loss[mod] = (model.loss_mod[mod](preds, targets) * w).sum()
        mod_n[mod] = w.sum()
        mod_preds[mod] = preds
    return sum(mod_loss.values()) / sum(mod_n.values()), mod_loss, mod_n, mod_preds


def mod_dict(batch, obj, eids):
    md = G.make_mod_dict(batch, obj)
    md["ap"]["eid"] = eids
    return md


def record_case(arrs, meta, case, batch):
    if case in R.XCASES:
        eids, bias = R.XEIDS, True
    else:
        eids, obj, bias, _ = R.CASES[case]
    st = Stitched(bias)
    st.train()
    if case in R.XCASES and R.XCASES[case].get("mode"):
        import input_masking as IM
        IM.set_masker(st.model.masker, R.XCASES[case]["mode"])
    named = st.named()
    import hashlib
    meta["params"][case] = [k for k, _ in named]
    meta["init"][case] = {}
    for k, v in named:
        a = G.npify(v)
        h = hashlib.sha256(str((a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()[:16]
        arrs[f"init/{h}"] = a
        meta["init"][case][k] = h
    torch.manual_seed(R.MASKER_SEED)
    random.seed(R.MASKER_SEED)
    md = R.xcase_mod_dict(case, R.xcase_batch(case)) if case in R.XCASES else mod_dict(R.case_batch(batch, case), obj, eids)
    loss, mod_loss, mod_n, mod_preds = ref_forward(st, md, eids)
    loss.backward()
    arrs[f"{case}/loss"] = G.npify(loss)
    for mod in ("ap", "behavior"):
        arrs[f"{case}/mod_loss/{mod}"] = G.npify(mod_loss[mod])
        arrs[f"{case}/n/{mod}"] = G.npify(mod_n[mod])
        arrs[f"{case}/preds/{mod}"] = G.npify(mod_preds[mod])
        arrs[f"{case}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
    arrs[f"{case}/grad_norm"] = np.array([float("nan") if p.grad is None else float(p.grad.double().norm()) for _, p in named])
    for k, p in named:
        if p.grad is not None and (case in R.FULL_GRAD or k.startswith("session_")):
            arrs[f"{case}/grad/{k}"] = G.npify(p.grad)
    print("   ", case, float(loss), {m: int(n) for m, n in mod_n.items()})


def curves():
    out = {}
    for name, steps, micro in (("turns", R.CURVE_STEPS, 1), ("accum", R.ACCUM_STEPS, R.ACCUM)):
        st = Stitched(True)
        st.train()
        opt, sch = G.make_opt(st, steps)
        random.seed(42)
        torch.manual_seed(1234)
        losses, objs = [], []
        for step in range(steps):
            for j in range(micro):
                i = step * micro + j
                obj = random.sample(list(G.OBJECTIVES), 1)[0]
                eids = [R.EIDS[i % 3]] * T_["B"]
                batch = G.synth_batch(T_["B"], T_["T"], T_["N_max"], T_["n_beh"], seed=i)
                batch["spikes_data"] = R.pad_batch(batch["spikes_data"], eids)
                loss = ref_forward(st, mod_dict(batch, obj, eids), eids)[0]
                (loss / micro).backward()
                losses.append(float(loss))
                objs.append(obj)
            opt.step()
            sch.step()
            opt.zero_grad()
        print("    curve", name, losses[:2], "...", losses[-1])
        out[name] = dict(loss=losses, objective=objs, steps=steps, micro=micro)
    return dict(out, sessions=dict(R.SESSIONS), model_seed=R.MODEL_SEED, **T_)


if __name__ == "__main__":
    meta = dict(T_, H=32, heads=4, inter=64, sessions=dict(R.SESSIONS), model_seed=R.MODEL_SEED, data_seed=R.DATA_SEED,
                masker_seed=R.MASKER_SEED, pad=R.PAD, cases=list(R.CASES) + list(R.XCASES), full_grad=list(R.FULL_GRAD), params={}, init={})
    arrs = {}
    batch = G.synth_batch(T_["B"], T_["T"], T_["N_max"], T_["n_beh"], seed=R.DATA_SEED)
    for k, v in batch.items():
        arrs[f"batch/{k}"] = G.npify(v)
    for case in list(R.CASES) + list(R.XCASES):
        record_case(arrs, meta, case, batch)
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("session_stitch_fwd_bwd.npz", **arrs)
    G.save_json("session_stitch_curve.json", curves())
