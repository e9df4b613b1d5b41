#!/usr/bin/env python3
"""Generate the per-side-config fixtures under tests/golden/ by importing the reference with `encoder.*` and `decoder.*` sections
that differ.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_side_config_goldens.py

side_config_fwd_bwd.npz  per case (CASES below: what each side's `transformer` / `embedder` section is updated with on top of the tiny
                         config, H = 32 / 4 heads / inter 64 / dropout 0, of linear_bias_fwd_bwd.npz, same seeds and batch) x the three
                         objectives: loss, per-modality n / loss / preds / masks and the norm of every gradient (order: meta params);
                         every gradient tensor in full for the FULL_GRAD objective of the FULL_GRAD_CASES; the state dict's keys and
                         shapes in order (meta state) and the initial parameters in full (init/<hash>, one array per distinct content;
                         meta init: case -> key -> hash).  meta switches holds CASES itself: the tests build their configs from it.
side_config_curve.json   50-step tiny curves (run_curve) for ALL and for HEADS
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

FULL_GRAD = "token_masking"
FULL_GRAD_CASES = ("ALL",)      # with every case's gradients in full the file exceeds the 1 MiB a committed file may have


def _t(enc=None, dec=None):
    return dict(encoder=dict(transformer=enc or {}), decoder=dict(transformer=dec or {}))


# case -> side -> section -> keys the tiny config is updated with
CASES = {
    "HEADS": _t(dict(n_heads=4), dict(n_heads=2)),
    "INTER": _t(dict(inter_size=64), dict(inter_size=128)),
    "DROP0": dict(encoder=dict(transformer=dict(dropout=0.0), embedder=dict(dropout=0.0)),
                  decoder=dict(transformer=dict(dropout=0.0), embedder=dict(dropout=0.0))),
    "NORM": _t(dict(use_scalenorm=True), dict(use_scalenorm=False)),
    "NORM_R": _t(dict(use_scalenorm=False), dict(use_scalenorm=True)),
    "ACT": _t(dict(act="gelu"), dict(act="silu")),
    "EMB": dict(encoder=dict(embedder=dict(mult=2, scale=1, max_F=8)), decoder=dict(embedder=dict(mult=3, scale=None, max_F=16))),
}
CASES["ALL"] = {side: {sec: {k: v for c in CASES.values() for k, v in c[side].get(sec, {}).items()} for sec in ("transformer", "embedder")}
                for side in ("encoder", "decoder")}
CASES["ALL"]["encoder"]["transformer"]["use_scalenorm"] = True          # NORM's direction (NORM_R is the reverse of it)
CASES["ALL"]["decoder"]["transformer"]["use_scalenorm"] = False


def config_of(case):
    return G.with_sides(G.tiny_model_cfg(), CASES[case])


def fx_fwd_bwd():
    meta = dict(**G.TINY, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                switches=CASES, full_grad=FULL_GRAD, full_grad_cases=list(FULL_GRAD_CASES), state={}, params={}, init={})
    G.fx_case_fwd_bwd("side_config_fwd_bwd.npz", CASES, config_of, meta, G.init_by_hash)


def fx_curve():
    res = {}
    for case in ("ALL", "HEADS"):
        model = G.build_model(config_of(case), 12, 2, seed=7)
        res[case] = dict(G.tiny_curve(model, case), n_state_keys=len(model.state_dict()))
    G.save_json("side_config_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
