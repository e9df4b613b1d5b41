#!/usr/bin/env python3
"""Generate the head-dim-128 fixtures under tests/golden/ by importing the reference with `hidden_size` 256 / `n_heads` 2.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_dh128_goldens.py

dh128_fwd_bwd.npz  H = 256, 2 heads (dh 128), inter 512, one encoder and one decoder layer, 12 + 2 channels, T = max_F = 20, B = 3 (sample 1
                   right-padded by 3 bins), dropout 0, token_masking; per decoder mask setting (dense, causal, causal_sep): loss,
                   per-modality loss sums / n / preds / masks, and the gradient of every parameter: its fp64 norm and sum, the tensor in
                   full up to SAMPLE elements, otherwise SAMPLE elements at a fixed stride (the model has 1.5 M parameters: three full
                   gradients are 18 MB, a committed file stays under 1 MiB).  The initial state dict (one per file: the mask switches
                   create no parameter) by key, shape, fp64 sum and norm, small tensors in full: the tests rebuild it from the seed.
dh128_curve.json   50 AdamW steps (run_curve) of the dense model: loss per step, objectives, the norm of every final parameter
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

CFG = dict(H=256, heads=2, inter=512, n_enc=1, n_dec=1, max_F=20)
B, T, N_AP, N_BEH = 3, 20, 12, 2
PAD = [0, 3, 0]
MODEL_SEED, DATA_SEED, MASK_SEED = 7, 3, 11
CASES = {"dense": dict(), "causal": dict(causal=True), "causal_sep": dict(causal=True, sep=True)}
OBJECTIVE = "token_masking"
SAMPLE = 1024


def sample(a):
    """The whole tensor up to SAMPLE elements, else SAMPLE elements at stride numel // SAMPLE from element 0 (flattened)."""
    f = np.ascontiguousarray(a).reshape(-1)
    return f if f.size <= SAMPLE else f[::f.size // SAMPLE][:SAMPLE].copy()


def fx_fwd_bwd():
    arrs = {}
    meta = dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, pad=PAD, model_seed=MODEL_SEED, data_seed=DATA_SEED, mask_seed=MASK_SEED,
                objective=OBJECTIVE, sample=SAMPLE, cases={k: dict(causal=bool(v.get("causal", False)), sep=bool(v.get("sep", False)))
                                                            for k, v in CASES.items()}, state=[], params=[], **CFG)
    batch = G.synth_batch(B, T, N_AP, N_BEH, seed=DATA_SEED, pad=PAD)
    for k, v in batch.items():
        arrs[f"batch/{k}"] = G.npify(v)
    for case, kw in CASES.items():
        model = G.build_model(G.tiny_model_cfg(dropout=0.0, emb_dropout=0.0, **CFG, **kw), N_AP, N_BEH, seed=MODEL_SEED)
        model.train()
        state = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        if not meta["state"]:
            meta["state"], meta["params"] = state, [k for k, _ in model.named_parameters()]
            for k, v in model.state_dict().items():
                arrs[f"init/{k}"] = sample(G.npify(v))
                arrs[f"init_stat/{k}"] = np.array([float(v.double().sum()), float(v.double().norm())])
        assert state == meta["state"]
        torch.manual_seed(MASK_SEED)
        md = G.make_mod_dict(batch, OBJECTIVE)
        out = model(md)
        out.loss.backward()
        arrs[f"{case}/loss"] = G.npify(out.loss)
        for mod in ("ap", "behavior"):
            arrs[f"{case}/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
            arrs[f"{case}/n/{mod}"] = G.npify(out.mod_n_examples[mod])
            arrs[f"{case}/preds/{mod}"] = G.npify(out.mod_preds[mod])
            arrs[f"{case}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
        for k, prm in model.named_parameters():
            g = prm.grad
            arrs[f"{case}/grad/{k}"] = sample(G.npify(g))
            arrs[f"{case}/grad_stat/{k}"] = np.array([float(g.double().sum()), float(g.double().norm())])
        print("   ", case, float(out.loss.detach()))
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("dh128_fwd_bwd.npz", **arrs)


def fx_curve():
    model = G.build_model(G.tiny_model_cfg(dropout=0.0, emb_dropout=0.0, **CFG), N_AP, N_BEH, seed=MODEL_SEED)
    res = dict(G.tiny_curve(model, "dh128", model_seed=MODEL_SEED, B=B, T=T, n_ap=N_AP, n_beh=N_BEH),
               n_state_keys=len(model.state_dict()), final_norm={k: float(v.double().norm()) for k, v in model.state_dict().items()}, **CFG)
    G.save_json("dh128_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
