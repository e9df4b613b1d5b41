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
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

B, T, N_AP, N_BEH = 2, 8, 12, 2
FULL_GRAD = ("base/token_masking",)        # cases that keep every gradient tensor (the fixture stays small)
VARIANTS = [("base", dict(), None, None), ("pad", dict(), [0, 2], [0, 3]), ("sep", dict(sep=True), [0, 2], None),
            ("deep", dict(n_enc=2, n_dec=2), None, None)]


def with_scalenorm(mcfg):
    return G.with_sides(mcfg, {side: dict(transformer=dict(use_scalenorm=True)) for side in ("encoder", "decoder")})


def fx_fwd_bwd():
    arrs = {}
    meta = dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                variants={v: kw for v, kw, _, _ in VARIANTS}, full_grad=list(FULL_GRAD), init={}, params={})
    for vname, kw, pad, shift in VARIANTS:
        model = G.build_model(with_scalenorm(G.tiny_model_cfg(**kw)), N_AP, N_BEH, seed=7)
        model.train()
        meta["init"][vname] = G.init_digest(model)
        meta["params"][vname] = [k for k, _ in model.named_parameters()]
        batch = G.synth_batch(B, T, N_AP, N_BEH, seed=3, pad=pad, ts_shift=shift)
        for k, v in batch.items():
            arrs[f"{vname}/batch/{k}"] = G.npify(v)
        for obj in G.OBJECTIVES:
            p = f"{vname}/{obj}"
            G.record_step(arrs, model, batch, p, obj, lambda k: p in FULL_GRAD or k.endswith(".scale"))
            meta["cases"].append(p)
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("scalenorm_fwd_bwd.npz", **arrs)


def fx_curve():
    res = {}
    res["tiny"] = G.tiny_curve(G.build_model(with_scalenorm(G.tiny_model_cfg()), N_AP, N_BEH, seed=7), "scalenorm")
    res["default"] = G.default_scalars(G.build_model(with_scalenorm(G.no_dropout_default_cfg()), 668, 2, seed=42))
    for obj, r in res["default"].items():
        print("    default", obj, r["loss"])
    G.save_json("scalenorm_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
