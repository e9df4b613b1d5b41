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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

ACTS = ("relu", "silu", "quick_gelu", "gelu_new")
DEFAULT_ACTS = ("relu", "silu")
FULL_GRAD = "token_masking"        # the objective whose gradients are kept in full, per activation (the fixture stays small)


def with_act(mcfg, act):
    return G.with_sides(mcfg, {side: dict(transformer=dict(act=act)) for side in ("encoder", "decoder")})


def record_init(arrs, meta, act, model):
    meta["init"][act] = G.init_digest(model)
    meta["params"][act] = [k for k, _ in model.named_parameters()]


def fx_fwd_bwd():
    meta = dict(**G.TINY, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                acts=list(ACTS), full_grad=FULL_GRAD, init={}, params={})
    G.fx_case_fwd_bwd("mlp_act_fwd_bwd.npz", ACTS, lambda act: with_act(G.tiny_model_cfg(), act), meta, record_init)


def fx_curve():
    res = {"tiny": {}, "default": {}}
    for act in ACTS:
        res["tiny"][act] = G.tiny_curve(G.build_model(with_act(G.tiny_model_cfg(), act), 12, 2, seed=7), act)
    for act in DEFAULT_ACTS:
        res["default"][act] = G.default_scalars(G.build_model(with_act(G.no_dropout_default_cfg(), act), 668, 2, seed=42))
        for obj, r in res["default"][act].items():
            print("    default", act, obj, r["loss"])
    G.save_json("mlp_act_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
