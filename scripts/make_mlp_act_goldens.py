#!/usr/bin/env python3
"""Generate the MLP-activation fixtures under tests/golden/ by importing the reference with `transformer.act` set on both sides.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_mlp_act_goldens.py

mlp_act_fwd_bwd.npz  per activation (relu, silu, quick_gelu, gelu_new): the tiny config (H = 32) x the three objectives: batch,
                     loss, per-modality n / loss / preds / masks and the norm of every gradient (order: meta params); every gradient
                     tensor in full for the FULL_GRAD objective of each activation; the initial state dict as a digest per tensor
                     (sha256 of the fp32 bytes (first 16 hex digits), shape, sum)
mlp_act_curve.json   a 50-step tiny curve per activation (run_curve) and default-size scalars (H = 256, 668 + 2 channels, dropout 0,
                     B = 16) for relu and silu
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
ACTS = ("relu", "silu", "quick_gelu", "gelu_new")
DEFAULT_ACTS = ("relu", "silu")
FULL_GRAD = "token_masking"        # the objective whose gradients are kept in full, per activation (the fixture stays small)


def with_act(mcfg, act):
    m = G.plain(mcfg)
    for side in ("encoder", "decoder"):
        m[side]["transformer"]["act"] = act
    return DictConfig(m)


def fx_fwd_bwd():
    arrs = {}
    meta = dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                acts=list(ACTS), full_grad=FULL_GRAD, init={}, params={})
    batch = G.synth_batch(B, T, N_AP, N_BEH, seed=3)
    for k, v in batch.items():
        arrs[f"batch/{k}"] = G.npify(v)
    for act in ACTS:
        model = G.build_model(with_act(G.tiny_model_cfg(), act), N_AP, N_BEH, seed=7)
        model.train()
        meta["init"][act] = [dict(key=k, shape=list(v.shape), dtype=str(v.dtype), sum=float(v.double().sum()),
                                  sha256=hashlib.sha256(G.npify(v).tobytes()).hexdigest()[:16]) for k, v in model.state_dict().items()]
        meta["params"][act] = [k for k, _ in model.named_parameters()]
        for obj in ("encoding", "decoding", "token_masking"):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(11)
            md = G.make_mod_dict(batch, obj)
            out = model(md)
            out.loss.backward()
            p = f"{act}/{obj}"
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
    G.save_npz("mlp_act_fwd_bwd.npz", **arrs)


def fx_curve():
    res = {"tiny": {}, "default": {}}
    for act in ACTS:
        model = G.build_model(with_act(G.tiny_model_cfg(), act), N_AP, N_BEH, seed=7)
        l, o = G.run_curve(model, 50, B, T, N_AP, N_BEH, total_steps=50)
        res["tiny"][act] = dict(loss=l, objective=o, model_seed=7, B=B, T=T, n_ap=N_AP, n_beh=N_BEH, total_steps=50)
        print("    tiny curve", act, l[:2], "...", l[-1])
    for act in DEFAULT_ACTS:
        cfg = G.plain(G.ref_config()["model"])
        for side in ("encoder", "decoder"):
            cfg[side]["embedder"]["dropout"] = 0.0
            cfg[side]["transformer"]["dropout"] = 0.0
        model = G.build_model(with_act(DictConfig(cfg), act), 668, 2, seed=42)
        model.eval()
        batch = G.default_batch()
        res["default"][act] = {}
        for obj in ("encoding", "decoding", "token_masking"):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            out = model(G.make_mod_dict(batch, obj))
            out.loss.backward()
            res["default"][act][obj] = dict(
                loss=float(out.loss), mod_loss={m: float(v) for m, v in out.mod_loss.items()},
                n={m: int(v) for m, v in out.mod_n_examples.items()},
                pred_abssum={m: float(v.double().abs().sum()) for m, v in out.mod_preds.items()},
                grad_norm={k: float(p.grad.double().norm()) for k, p in model.named_parameters()})
            print("    default", act, obj, res["default"][act][obj]["loss"])
    G.save_json("mlp_act_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
