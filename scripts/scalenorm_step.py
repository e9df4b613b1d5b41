"""Training-step time of the default config (H = 256, 668 + 2 channels, T = 100) in bf16 as a LayerNorm model and as a ScaleNorm model
(use_scalenorm: true), in the same process on the same device: the two models alternate in rounds so that clock / thermal drift
hits both alike.  Also reports each plan's C calls (= kernel launches of the step plan, one per entry; a few entries launch a
second kernel, identically in both models).

    python scripts/scalenorm_step.py [B=1024] [out.json]
"""
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch
from multi_modal_foundation_model_amd.builders import model_config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
T, STEPS, ROUNDS = 100, 10, 5

runs = {name: make_runner(model_config(scalenorm=sn), 668, 2, B, T) for name, sn in (("layernorm", False), ("scalenorm", True))}
time_rounds(runs, STEPS, ROUNDS)
res = dict(B=B, T=T, dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS,
           fused_mask=runs["scalenorm"]["model"]._engine._fused_mask(B * 2 * T), device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = summarise(r)
res["scalenorm_over_layernorm"] = res["scalenorm"]["ms_per_step_median"] / res["layernorm"]["ms_per_step_median"]
emit(res, OUT)
