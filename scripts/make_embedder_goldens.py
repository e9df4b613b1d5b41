#!/usr/bin/env python3
"""Generate the embedder-option fixtures under tests/golden/ by importing the reference with `embedder.act`, `pos` and `bias` set.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_embedder_goldens.py

embedder_opts_fwd_bwd.npz  per case (CASES below: what each side's `embedder` section is updated with on top of the tiny config,
                           H = 32 / 4 heads / inter 64 / dropout 0, of side_config_fwd_bwd.npz, same seeds and batch) x the three
                           objectives: loss, per-modality n / loss / preds / masks and the norm of every gradient (order: meta params);
                           every gradient tensor in full for the FULL_GRAD objective of the FULL_GRAD_CASES; the state dict's keys and
                           shapes in order (meta state) and the initial parameters in full (init/<hash>, one array per distinct content;
                           meta init: case -> key -> hash).  meta switches holds CASES itself: the tests build their configs from it.
embedder_opts_curve.json   50-step tiny curves (run_curve) for ASYM and for GELU
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)
from utils.config_utils import DictConfig  # noqa: E402  (reference)

B, T, N_AP, N_BEH = 2, 8, 12, 2
FULL_GRAD = "token_masking"
FULL_GRAD_CASES = ("ASYM", "SCALE")      # with every case's gradients in full the file exceeds the 1 MiB a committed file may have


def _both(**emb):
    return dict(encoder=dict(embedder=dict(emb)), decoder=dict(embedder=dict(emb)))


# case -> side -> section -> keys the tiny config is updated with
CASES = {
    "IDENTITY": _both(act="identity"),
    "RELU": _both(act="relu"),
    "GELU": _both(act="gelu"),
    "SILU": _both(act="silu"),
    "QUICK_GELU": _both(act="quick_gelu"),
    "GELU_NEW": _both(act="gelu_new"),
    "TANH": _both(act="tanh"),
    "POS_OFF": _both(pos=False),
    "BIAS_OFF": _both(bias=False),
    "POS_BIAS_OFF": _both(pos=False, bias=False),
    "ASYM": dict(encoder=dict(embedder=dict(act="tanh", pos=False, bias=False, scale=None)), decoder=dict(embedder={})),
    "SCALE": _both(act="silu", scale=0.7),
}


def with_sides(mcfg, case):
    m = G.plain(mcfg)
    for side, secs in CASES[case].items():
        for sec, upd in secs.items():
            m[side][sec].update(upd)
    return DictConfig(m)


def fx_fwd_bwd():
    arrs = {}
    meta = dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                switches=CASES, full_grad=FULL_GRAD, full_grad_cases=list(FULL_GRAD_CASES), state={}, params={}, init={})
    batch = G.synth_batch(B, T, N_AP, N_BEH, seed=3)
    for k, v in batch.items():
        arrs[f"batch/{k}"] = G.npify(v)
    for case in CASES:
        model = G.build_model(with_sides(G.tiny_model_cfg(), case), N_AP, N_BEH, seed=7)
        model.train()
        meta["state"][case] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        meta["params"][case] = [k for k, _ in model.named_parameters()]
        meta["init"][case] = {}
        for k, v in model.state_dict().items():       # cases that draw the same stream share their tensors: one array per content
            a = G.npify(v)
            h = hashlib.sha256(str((a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()[:16]
            arrs[f"init/{h}"] = a
            meta["init"][case][k] = h
        for obj in ("encoding", "decoding", "token_masking"):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(11)
            md = G.make_mod_dict(batch, obj)
            out = model(md)
            out.loss.backward()
            p = f"{case}/{obj}"
            arrs[f"{p}/loss"] = G.npify(out.loss)
            for mod in ("ap", "behavior"):
                arrs[f"{p}/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
                arrs[f"{p}/n/{mod}"] = G.npify(out.mod_n_examples[mod])
                arrs[f"{p}/preds/{mod}"] = G.npify(out.mod_preds[mod])
                arrs[f"{p}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
            arrs[f"{p}/grad_norm"] = np.array([float(prm.grad.double().norm()) for _, prm in model.named_parameters()])
            if obj == FULL_GRAD and case in FULL_GRAD_CASES:
                for k, prm in model.named_parameters():
                    arrs[f"{p}/grad/{k}"] = G.npify(prm.grad)
            meta["cases"].append(p)
            print("   ", p, float(out.loss))
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("embedder_opts_fwd_bwd.npz", **arrs)


def fx_curve():
    res = {}
    for case in ("ASYM", "GELU"):
        model = G.build_model(with_sides(G.tiny_model_cfg(), case), N_AP, N_BEH, seed=7)
        l, o = G.run_curve(model, 50, B, T, N_AP, N_BEH, total_steps=50)
        res[case] = dict(loss=l, objective=o, model_seed=7, B=B, T=T, n_ap=N_AP, n_beh=N_BEH, total_steps=50,
                         n_state_keys=len(model.state_dict()))
        print("    tiny curve", case, l[:2], "...", l[-1])
    G.save_json("embedder_opts_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
