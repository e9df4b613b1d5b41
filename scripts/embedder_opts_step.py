"""Training-step time of the default config (H = 256, 668 + 2 channels, T = 100) in bf16, dropout on, next to two models with non-default
embedder options - `act: gelu` on both sides (the forward writes the token_embed pre-activation z, the backward reads it) and
`pos: false` on both sides (no position tables) - in the same process on the same device: the models alternate in rounds so that clock /
thermal drift hits all alike.  Also reports each plan's C calls (= kernel launches of the step plan, one per entry).

    python scripts/embedder_opts_step.py [B=1024] [out.json] [default|all]

`default` measures the default model alone, with the loop of scripts/side_config_step.py default: run it on this commit and that script
on the parent commit in one session to compare the two.
"""
import os
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch
from multi_modal_foundation_model_amd.builders import model_config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
WHICH = sys.argv[3] if len(sys.argv) > 3 else "all"
T, STEPS, ROUNDS = 100, 10, 5


def make(emb):
    mc = model_config()
    for side in ("encoder", "decoder"):
        mc[side]["embedder"].update(emb)
    return make_runner(mc, 668, 2, B, T)


CONFIGS = {"default": {}}
if WHICH == "all":
    CONFIGS.update(act_gelu=dict(act="gelu"), pos_off=dict(pos=False))
runs = {name: make(kw) for name, kw in CONFIGS.items()}
time_rounds(runs, STEPS, ROUNDS)
res = dict(B=B, T=T, MMFM_FUSED=os.environ.get("MMFM_FUSED"), dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS,
           fused_mask=runs["default"]["model"]._engine._fused_mask(B * 2 * T), device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = summarise(r, spread=True, parameters=True)
for name in runs:
    if name != "default":
        res[name + "_over_default"] = res[name]["ms_per_step_median"] / res["default"]["ms_per_step_median"]
emit(res, OUT)
