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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

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


def config_of(case):
    return G.with_sides(G.tiny_model_cfg(), CASES[case])


def fx_fwd_bwd():
    meta = dict(**G.TINY, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                switches=CASES, full_grad=FULL_GRAD, full_grad_cases=list(FULL_GRAD_CASES), state={}, params={}, init={})
    G.fx_case_fwd_bwd("embedder_opts_fwd_bwd.npz", CASES, config_of, meta, G.init_by_hash)


def fx_curve():
    res = {}
    for case in ("ASYM", "GELU"):
        model = G.build_model(config_of(case), 12, 2, seed=7)
        res[case] = dict(G.tiny_curve(model, case), n_state_keys=len(model.state_dict()))
    G.save_json("embedder_opts_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
