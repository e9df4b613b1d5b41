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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

# case -> ((encoder attention_bias, mlp_bias), (decoder attention_bias, mlp_bias))
CASES = {"FT": ((False, True), (False, True)), "TF": ((True, False), (True, False)), "FF": ((False, False), (False, False)),
         "FF_TT": ((False, False), (True, True))}
FULL_GRAD = "token_masking"


def with_bias(case, scalenorm=False):
    return G.with_sides(G.tiny_model_cfg(), {side: dict(transformer=dict(attention_bias=ab, mlp_bias=mb, use_scalenorm=scalenorm))
                                             for side, (ab, mb) in zip(("encoder", "decoder"), CASES[case])})


def record_init(arrs, meta, case, model):
    meta["state"][case] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    meta["params"][case] = [k for k, _ in model.named_parameters()]
    for k, v in model.state_dict().items():
        arrs[f"{case}/init/{k}"] = G.npify(v)


def fx_fwd_bwd():
    meta = dict(**G.TINY, H=32, heads=4, inter=64, max_F=8, model_seed=7, data_seed=3, cases=[],
                switches={k: [list(v[0]), list(v[1])] for k, v in CASES.items()}, full_grad=FULL_GRAD, state={}, params={})
    G.fx_case_fwd_bwd("linear_bias_fwd_bwd.npz", CASES, with_bias, meta, record_init)


def fx_curve():
    res = {}
    for name, sn in (("FF/layernorm", False), ("FF/scalenorm", True)):
        model = G.build_model(with_bias("FF", scalenorm=sn), 12, 2, seed=7)
        res[name] = dict(G.tiny_curve(model, name), scalenorm=sn, n_state_keys=len(model.state_dict()))
    G.save_json("linear_bias_curve.json", res)


if __name__ == "__main__":
    fx_fwd_bwd()
    fx_curve()
