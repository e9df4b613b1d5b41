#!/usr/bin/env python3
"""Generate the modal_filter fixtures under tests/golden/ by importing the reference with filtered tokeniser dicts.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_modal_filter_goldens.py

modal_filter_fwd_bwd.npz  per case (CASES below: the modalities the encoder / the decoder gets tokenisers for, the decoder mask switches
                          and share_modality_embeddings, on the tiny config H = 32 / 4 heads / inter 64 / dropout 0 with the seeds and
                          batch of side_config_fwd_bwd.npz) x the three objectives: loss and per-decoder-modality n always; where the
                          objective masks something in the decoder's modalities also per-decoder-modality loss / preds, EVERY
                          modality's mask and the norm of every gradient (order: meta params).  An objective that masks nothing there
                          gives loss = NaN with n = 0 upstream (meta nan lists those case/objective pairs): nothing else is stored.
                          Every gradient tensor in full for the FULL_GRAD objective of the FULL_GRAD_CASES; the state dict's keys and
                          shapes in order (meta state), the parameter names (meta params) and the initial parameters in full
                          (init/<hash>, one array per distinct content; meta init: case -> key -> hash).  meta switches holds CASES
                          itself: the tests build their models from it.
modal_filter_curve.json   50-step tiny curves (run_curve: the objective is sampled per step and none is skipped) for DEC and UNSHARED.
                          DEC's first `encoding` step is NaN upstream and AdamW carries the NaN into every parameter, so every later
                          step is NaN too: `nan` lists, per step, whether the reference's loss is NaN.
"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

FULL_GRAD = "token_masking"
FULL_GRAD_CASES = ("DEC", "UNSHARED")
MODEL_SEED, DATA_SEED = 7, 3
BOTH = ["ap", "behavior"]

# case -> input / output: modal_filter; sep / causal: decoder_sep_mask / decoder_causal_mask; share: share_modality_embeddings
CASES = {
    "DEC": dict(input=["ap"], output=["behavior"]),
    "ENC": dict(input=["behavior"], output=["ap"]),
    "AP": dict(input=["ap"], output=["ap"]),
    "BEH": dict(input=["behavior"], output=["behavior"]),
    "DEC_MASKS": dict(input=["ap"], output=["behavior"], sep=True, causal=True),
    "UNSHARED": dict(input=BOTH, output=BOTH, share=False),
}


def build_model(case):
    """oracle/make_goldens.py build_model with the tokeniser dicts of train_multi_modal.py under a modal_filter: the encoder's
    tokenisers for modal_filter["input"], then the decoder's for modal_filter["output"] (construction order = RNG contract)."""
    sw = CASES[case]
    cfg = G.tiny_model_cfg(sep=sw.get("sep", False), causal=sw.get("causal", False))
    chan = dict(ap=G.TINY["n_ap"], behavior=G.TINY["n_beh"])
    torch.manual_seed(MODEL_SEED)
    enc = {mod: G.EncoderEmbedding(hidden_size=cfg.encoder.transformer.hidden_size, n_channel=chan[mod], config=cfg.encoder)
           for mod in sw["input"]}
    dec = {mod: G.DecoderEmbedding(hidden_size=cfg.decoder.transformer.hidden_size, n_channel=chan[mod], output_channel=chan[mod],
                                   config=cfg.decoder) for mod in sw["output"]}
    return G.MultiModal(enc, dec, avail_mod=list(BOTH), config=cfg, share_modality_embeddings=sw.get("share", True))


def record_step(arrs, meta, model, batch, case, obj, keep_grad):
    """oracle/make_goldens.py record_step over the decoder's modalities; a NaN step (nothing masked in them) keeps loss and n only."""
    p = f"{case}/{obj}"
    model.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    md = G.make_mod_dict(batch, obj)
    out = model(md)
    assert list(out.mod_loss) == [m for m in BOTH if m in CASES[case]["output"]]
    arrs[f"{p}/loss"] = G.npify(out.loss)
    for mod in out.mod_n_examples:
        arrs[f"{p}/n/{mod}"] = G.npify(out.mod_n_examples[mod])
    if math.isnan(out.loss.item()):
        assert sum(int(n) for n in out.mod_n_examples.values()) == 0
        meta["nan"].append(p)
        print("   ", p, "NaN (n = 0)")
        return
    out.loss.backward()
    for mod in out.mod_loss:
        arrs[f"{p}/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
        arrs[f"{p}/preds/{mod}"] = G.npify(out.mod_preds[mod])
    for mod in BOTH:
        arrs[f"{p}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
    arrs[f"{p}/grad_norm"] = np.array([float(prm.grad.double().norm()) for _, prm in model.named_parameters()])
    for k, prm in model.named_parameters():
        if keep_grad:
            arrs[f"{p}/grad/{k}"] = G.npify(prm.grad)
    print("   ", p, float(out.loss))


def fx_fwd_bwd():
    meta = dict(**G.TINY, H=32, heads=4, inter=64, max_F=8, model_seed=MODEL_SEED, data_seed=DATA_SEED, cases=[], nan=[],
                switches=CASES, full_grad=FULL_GRAD, full_grad_cases=list(FULL_GRAD_CASES), state={}, params={}, init={})
    arrs = {}
    batch = G.synth_batch(seed=DATA_SEED, **G.TINY)
    for k, v in batch.items():
        arrs[f"batch/{k}"] = G.npify(v)
    for case in CASES:
        model = build_model(case)
        model.train()
        G.init_by_hash(arrs, meta, case, model)
        print(case, "parameters / state keys", len(meta["params"][case]), "/", len(meta["state"][case]))
        for obj in G.OBJECTIVES:
            record_step(arrs, meta, model, batch, case, obj, obj == FULL_GRAD and case in FULL_GRAD_CASES)
            meta["cases"].append(f"{case}/{obj}")
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("modal_filter_fwd_bwd.npz", **arrs)


def fx_curve():
    res = {}
    for case in ("DEC", "UNSHARED"):
        model = build_model(case)
        rec = G.tiny_curve(model, case, model_seed=MODEL_SEED)
        rec["nan"] = [math.isnan(x) for x in rec["loss"]]
        rec["loss"] = [None if math.isnan(x) else x for x in rec["loss"]]        # (JSON has no NaN: `nan` says which steps are)
        res[case] = dict(rec, n_state_keys=len(model.state_dict()))
    G.save_json("modal_filter_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
