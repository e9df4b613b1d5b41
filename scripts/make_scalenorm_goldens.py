#!/usr/bin/env python3
"""Generate the ScaleNorm fixtures under tests/golden/ by importing the reference with `use_scalenorm: true` on both sides.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_scalenorm_goldens.py

scalenorm_fwd_bwd.npz  tiny config (H = 32), variants base / pad / sep / deep x the three objectives: batch, loss, per-modality
                       n / loss / preds / masks, each `.scale` gradient and the norm of every gradient (order: meta params); every gradient tensor in
                       full for the FULL_GRAD cases; the initial state dict as a digest per tensor (sha256 of the fp32 bytes,
                       (first 16 hex digits), shape, sum) - the model is rebuilt from its seed, and the digest pins that rebuild bit for bit
scalenorm_curve.json   a 50-step tiny curve (run_curve) and default-size scalars (H = 256, 668 + 2 channels, dropout 0, B = 16)
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
FULL_GRAD = ("base/token_masking",)        # cases that keep every gradient tensor (the fixture stays small)
VARIANTS = [("base", dict(), None, None), ("pad", dict(), [0, 2], [0, 3]), ("sep", dict(sep=True), [0, 2], None),
            ("deep", dict(n_enc=2, n_dec=2), None, None)]


def with_scalenorm(mcfg):
    m = G.plain(mcfg)
    for side in ("encoder", "decoder"):
        m[side]["transformer"]["use_scalenorm"] = True
    return DictConfig(m)


def fx_fwd_bwd():
    arrs = {}
    meta = dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                variants={v: kw for v, kw, _, _ in VARIANTS}, full_grad=list(FULL_GRAD), init={}, params={})
    for vname, kw, pad, shift in VARIANTS:
        model = G.build_model(with_scalenorm(G.tiny_model_cfg(**kw)), N_AP, N_BEH, seed=7)
        model.train()
        meta["init"][vname] = [dict(key=k, shape=list(v.shape), dtype=str(v.dtype), sum=float(v.double().sum()),
                                    sha256=hashlib.sha256(G.npify(v).tobytes()).hexdigest()[:16]) for k, v in model.state_dict().items()]
        batch = G.synth_batch(B, T, N_AP, N_BEH, seed=3, pad=pad, ts_shift=shift)
        for k, v in batch.items():
            arrs[f"{vname}/batch/{k}"] = G.npify(v)
        for obj in ("encoding", "decoding", "token_masking"):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(11)
            md = G.make_mod_dict(batch, obj)
            out = model(md)
            out.loss.backward()
            p = f"{vname}/{obj}"
            arrs[f"{p}/loss"] = G.npify(out.loss)
            for mod in ("ap", "behavior"):
                arrs[f"{p}/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
                arrs[f"{p}/n/{mod}"] = G.npify(out.mod_n_examples[mod])
                arrs[f"{p}/preds/{mod}"] = G.npify(out.mod_preds[mod])
                arrs[f"{p}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
            meta["params"][vname] = [k for k, _ in model.named_parameters()]
            arrs[f"{p}/grad_norm"] = np.array([float(prm.grad.double().norm()) for _, prm in model.named_parameters()])
            for k, prm in model.named_parameters():
                if p in FULL_GRAD or k.endswith(".scale"):
                    arrs[f"{p}/grad/{k}"] = G.npify(prm.grad)
            meta["cases"].append(p)
            print("   ", p, float(out.loss))
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("scalenorm_fwd_bwd.npz", **arrs)


def fx_curve():
    res = {}
    model = G.build_model(with_scalenorm(G.tiny_model_cfg()), N_AP, N_BEH, seed=7)
    l, o = G.run_curve(model, 50, B, T, N_AP, N_BEH, total_steps=50)
    res["tiny"] = dict(loss=l, objective=o, model_seed=7, B=B, T=T, n_ap=N_AP, n_beh=N_BEH, total_steps=50)
    print("    tiny curve:", l[:2], "...", l[-1])
    cfg = G.plain(G.ref_config()["model"])
    for side in ("encoder", "decoder"):
        cfg[side]["embedder"]["dropout"] = 0.0
        cfg[side]["transformer"]["dropout"] = 0.0
    model = G.build_model(with_scalenorm(DictConfig(cfg)), 668, 2, seed=42)
    model.eval()
    batch = G.default_batch()
    res["default"] = {}
    for obj in ("encoding", "decoding", "token_masking"):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        out = model(G.make_mod_dict(batch, obj))
        out.loss.backward()
        res["default"][obj] = dict(
            loss=float(out.loss), mod_loss={m: float(v) for m, v in out.mod_loss.items()},
            n={m: int(v) for m, v in out.mod_n_examples.items()},
            pred_abssum={m: float(v.double().abs().sum()) for m, v in out.mod_preds.items()},
            grad_norm={k: float(p.grad.double().norm()) for k, p in model.named_parameters()})
        print("    default", obj, res["default"][obj]["loss"])
    G.save_json("scalenorm_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
