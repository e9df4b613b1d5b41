#!/usr/bin/env python3
"""Generate the bias-free-linear fixtures under tests/golden/ by importing the reference with `transformer.attention_bias` /
`transformer.mlp_bias` switched off.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_linear_bias_goldens.py

linear_bias_fwd_bwd.npz  per case - FT, TF, FF = (attention_bias, mlp_bias) on both sides, FF_TT = encoder (F, F) with decoder (T, T) -
                         the tiny config (H = 32) of mlp_act_fwd_bwd.npz with its seeds and batch x the three objectives: loss,
                         per-modality n / loss / preds / masks and the norm of every gradient (order: meta params); every gradient tensor
                         in full for the FULL_GRAD objective; the state dict's keys and shapes in order (meta state) and the initial
                         parameters in full (nn.Linear(bias=False) draws no bias, so everything created after it sees a shifted stream)
linear_bias_curve.json   50-step tiny curves (run_curve) for FF under LayerNorm and FF under use_scalenorm: true
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)
from utils.config_utils import DictConfig  # noqa: E402  (reference)

B, T, N_AP, N_BEH = 2, 8, 12, 2
# case -> ((encoder attention_bias, mlp_bias), (decoder attention_bias, mlp_bias))
CASES = {"FT": ((False, True), (False, True)), "TF": ((True, False), (True, False)), "FF": ((False, False), (False, False)),
         "FF_TT": ((False, False), (True, True))}
FULL_GRAD = "token_masking"


def with_bias(mcfg, case, scalenorm=False):
    m = G.plain(mcfg)
    for side, (ab, mb) in zip(("encoder", "decoder"), CASES[case]):
        m[side]["transformer"].update(attention_bias=ab, mlp_bias=mb, use_scalenorm=scalenorm)
    return DictConfig(m)


def fx_fwd_bwd():
    arrs = {}
    meta = dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                switches={k: [list(v[0]), list(v[1])] for k, v in CASES.items()}, full_grad=FULL_GRAD, state={}, params={})
    batch = G.synth_batch(B, T, N_AP, N_BEH, seed=3)
    for k, v in batch.items():
        arrs[f"batch/{k}"] = G.npify(v)
    for case in CASES:
        model = G.build_model(with_bias(G.tiny_model_cfg(), case), N_AP, N_BEH, seed=7)
        model.train()
        meta["state"][case] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        meta["params"][case] = [k for k, _ in model.named_parameters()]
        for k, v in model.state_dict().items():
            arrs[f"{case}/init/{k}"] = G.npify(v)
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
            if obj == FULL_GRAD:
                for k, prm in model.named_parameters():
                    arrs[f"{p}/grad/{k}"] = G.npify(prm.grad)
            meta["cases"].append(p)
            print("   ", p, float(out.loss))
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("linear_bias_fwd_bwd.npz", **arrs)


def fx_curve():
    res = {}
    for name, sn in (("FF/layernorm", False), ("FF/scalenorm", True)):
        model = G.build_model(with_bias(G.tiny_model_cfg(), "FF", scalenorm=sn), N_AP, N_BEH, seed=7)
        l, o = G.run_curve(model, 50, B, T, N_AP, N_BEH, total_steps=50)
        res[name] = dict(loss=l, objective=o, model_seed=7, B=B, T=T, n_ap=N_AP, n_beh=N_BEH, total_steps=50, scalenorm=sn,
                         n_state_keys=len(model.state_dict()))
        print("    tiny curve", name, l[:2], "...", l[-1])
    G.save_json("linear_bias_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
