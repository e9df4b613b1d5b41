"""Training-step time of the default config (H = 256, 668 + 2 channels, T = 100) in bf16 with the MLP activation (transformer.act)
gelu, relu, silu and gelu_new, in the same process on the same device: the models alternate in rounds so that clock / thermal drift
hits all alike.  Also reports each plan's C calls (= kernel launches of the step plan, one per entry), which must agree.

    python scripts/mlp_act_step.py [B=1024] [out.json] [H=256]

H = 512 (inter 1024) runs the un-fused MLP through the 256-tile GEMM (csrc/gemm_big.hip); MMFM_FUSED=0 the un-fused path at H = 256.
"""
import os
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch
from multi_modal_foundation_model_amd.builders import model_config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
H = int(sys.argv[3]) if len(sys.argv) > 3 else 256
T, STEPS, ROUNDS = 100, 10, 5
ACTS = ("gelu", "relu", "silu", "gelu_new")

runs = {act: make_runner(model_config(act=act, H=H, inter=2 * H), 668, 2, B, T) for act in ACTS}
time_rounds(runs, STEPS, ROUNDS)
res = dict(B=B, T=T, H=H, inter=2 * H, MMFM_FUSED=os.environ.get("MMFM_FUSED"), dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS,
           fused_mask=runs["gelu"]["model"]._engine._fused_mask(B * 2 * T), device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = summarise(r)
res["over_gelu"] = {act: res[act]["ms_per_step_median"] / res["gelu"]["ms_per_step_median"] for act in ACTS}
emit(res, OUT)
