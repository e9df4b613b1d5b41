#!/usr/bin/env python3
"""Generate the per-sample token-masking fixtures under tests/golden/ by running the reference with each sample's own masked tokens zeroed.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.  Nothing of the mirror is imported.

The reference's forward_mask_encoder / forward_mask_decoder zero the token rows at argwhere(mask[0] == 1) in every sample.  `per_sample`
wraps the two methods of the reference's own MultiModal without restating them: it calls cat_encoder_tensors / cat_decoder_tensors for
the un-zeroed tokens (the concatenation is pure: torch.cat copies, and the original method concatenates again for itself), calls the
original method for everything else - the embeddings, the masks, the attention masks, the targets - and returns
tokens * (mask != 1)[..., None]  in place of its tokens.  Everything else is the reference's forward as it stands: the loss and
n_examples use each sample's own mask, as they always did, and the masker's calls and generator stream are untouched.

    python scripts/make_per_sample_mask_goldens.py

per_sample_mask_fwd_bwd.npz  per case of tests/per_sample_mask.py CASES (tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0,
                             B = 3, model seed 7, data seed 3, masker seed 11; explicit eval masks but for DRAWN) its objectives, what
                             oracle.make_goldens.record_step stores; every gradient tensor in full for PAD / token_masking; the case's
                             batch; parameter names, state-dict keys and the initial parameters by hash; for EVAL_CASES one eval-mode
                             forward under the case's masks.  One modal_filter case (FILTER: encoder spikes, decoder behaviour).
per_sample_mask_curve.json   50 AdamW + OneCycle steps by oracle.make_goldens.run_curve's recipe (the objective sampled per step), B = 3.
"""
import json
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import per_sample_mask as P  # noqa: E402
from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)


def per_sample(model):
    """The reference model with every sample's own masked tokens zeroed on both sides (module docstring)."""
    enc, dec = model.forward_mask_encoder, model.forward_mask_decoder

    def forward_mask_encoder(mod_dict):
        tokens = model.cat_encoder_tensors(mod_dict)[0]
        _, emb, mask, attn, mod_mask = enc(mod_dict)
        return tokens * (mask != 1)[..., None], emb, mask, attn, mod_mask

    def forward_mask_decoder(mod_dict):
        tokens = model.cat_decoder_tensors(mod_dict)[0]
        _, gts, emb, mask, attn, mod_mask = dec(mod_dict)
        return tokens * (mask != 1)[..., None], gts, emb, mask, attn, mod_mask
    model.forward_mask_encoder, model.forward_mask_decoder = forward_mask_encoder, forward_mask_decoder
    return model


def tiny_cfg(sw):
    return G.tiny_model_cfg(max_F=P.TINY["max_F"], sep=bool(sw.get("sep")), causal=bool(sw.get("causal")))


def record(arrs, meta, case, model, objectives):
    """What oracle.make_goldens.record_step stores, on the case's mod_dict (tests/per_sample_mask.py mod_dict stands in for
    make_mod_dict), with every gradient tensor for the full-gradient case."""
    model.train()
    G.init_by_hash(arrs, meta, case, model)
    for mod, d in P.case_batch(case).items():
        for k, v in d.items():
            arrs[f"batch/{case}/{mod}/{k}"] = G.npify(v)
    for obj in objectives:
        full = obj == P.FULL_GRAD and case in P.FULL_GRAD_CASES
        with mock.patch.object(G, "make_mod_dict", lambda _batch, o: P.mod_dict(case, o)):
            G.record_step(arrs, model, None, f"{case}/{obj}", obj, lambda k: full)
        meta["cases"].append(f"{case}/{obj}")


def record_case(case, arrs, meta):
    sw = P.CASES[case]
    model = per_sample(G.build_model(tiny_cfg(sw), P.TINY["n_ap"], P.TINY["n_beh"], seed=P.MODEL_SEED))
    record(arrs, meta, case, model, sw.get("objectives", ("token_masking",)))
    if sw["masks"] is None:         # the masker's draw must make the two modes differ: sample 0's mask is not every sample's
        m = arrs[f"{case}/token_masking/mask/ap"]
        assert any((m[b] != m[0]).any() for b in range(1, m.shape[0])), "the draw gave every sample the same mask"
    if case in P.EVAL_CASES:
        model.eval()
        with torch.no_grad():
            out = model(P.mod_dict(case, "token_masking"))
        arrs[f"{case}/eval/loss"] = G.npify(out.loss)
        for mod in P.MODS:
            arrs[f"{case}/eval/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
            arrs[f"{case}/eval/n/{mod}"] = G.npify(out.mod_n_examples[mod])
            arrs[f"{case}/eval/preds/{mod}"] = G.npify(out.mod_preds[mod])
        print("   ", case, "eval", float(out.loss))


def record_filter(arrs, meta):
    """The modal_filter case (tests/per_sample_mask.py FILTER): the reference built with the tokeniser dicts of train_multi_modal.py under
    the filter (the encoder's tokenisers, then the decoder's: construction order = RNG contract); records over the decoder's modalities."""
    f = P.FILTER
    case = f["case"]
    cfg = tiny_cfg(f)
    chan = dict(ap=P.TINY["n_ap"], behavior=P.TINY["n_beh"])
    torch.manual_seed(P.MODEL_SEED)
    enc = {m: G.EncoderEmbedding(hidden_size=cfg.encoder.transformer.hidden_size, n_channel=chan[m], config=cfg.encoder) for m in f["input"]}
    dec = {m: G.DecoderEmbedding(hidden_size=cfg.decoder.transformer.hidden_size, n_channel=chan[m], output_channel=chan[m],
                                 config=cfg.decoder) for m in f["output"]}
    model = per_sample(G.MultiModal(enc, dec, avail_mod=list(P.MODS), config=cfg, share_modality_embeddings=True))
    model.train()
    G.init_by_hash(arrs, meta, case, model)
    for mod, d in P.case_batch(case).items():
        for k, v in d.items():
            arrs[f"batch/{case}/{mod}/{k}"] = G.npify(v)
    for obj in f["objectives"]:
        p = f"{case}/{obj}"
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        md = P.mod_dict(case, obj)
        out = model(md)
        assert list(out.mod_loss) == f["output"]
        out.loss.backward()
        arrs[f"{p}/loss"] = G.npify(out.loss)
        for mod in out.mod_loss:
            arrs[f"{p}/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
            arrs[f"{p}/n/{mod}"] = G.npify(out.mod_n_examples[mod])
            arrs[f"{p}/preds/{mod}"] = G.npify(out.mod_preds[mod])
        for mod in P.MODS:
            arrs[f"{p}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
        arrs[f"{p}/grad_norm"] = np.array([float(prm.grad.double().norm()) for _, prm in model.named_parameters()])
        meta["cases"].append(p)
        print("   ", p, float(out.loss.detach()))


def curve():
    c = P.CURVE
    model = per_sample(G.build_model(G.tiny_model_cfg(max_F=P.TINY["max_F"]), c["n_ap"], c["n_beh"], seed=P.MODEL_SEED))
    l, o = G.run_curve(model, c["steps"], c["B"], c["T"], c["n_ap"], c["n_beh"], total_steps=c["steps"])
    print("    curve", l[:2], "...", l[-1])
    return dict(loss=l, objective=o, model_seed=P.MODEL_SEED, total_steps=c["steps"], **{k: c[k] for k in ("B", "T", "n_ap", "n_beh")})


if __name__ == "__main__":
    meta = dict(**P.TINY, H=32, heads=4, inter=64, model_seed=P.MODEL_SEED, data_seed=P.DATA_SEED, masker_seed=11, cases=[],
                switches={k: {kk: vv for kk, vv in v.items() if kk != "objectives"} for k, v in P.CASES.items()}, full_grad=P.FULL_GRAD,
                full_grad_cases=list(P.FULL_GRAD_CASES), eval_cases=list(P.EVAL_CASES),
                modal_filter=dict(P.FILTER, objectives=list(P.FILTER["objectives"])), state={}, params={}, init={})
    arrs = {}
    for case in P.CASES:
        record_case(case, arrs, meta)
    record_filter(arrs, meta)
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("per_sample_mask_fwd_bwd.npz", **arrs)
    G.save_json("per_sample_mask_curve.json", curve())
