"""Training-step time of the default config (H = 256, 668 + 2 channels, T = 100, L = 200) in bf16 with dropout on, for the decoder
attention-mask switches of mm.yaml: dense (both off), decoder_causal_mask, decoder_sep_mask and both, in the same process on the same
device: the models alternate in rounds so that clock / thermal drift hits all alike.  Also reports each plan's C calls (= kernel
launches of the step plan, one per entry).  The runner and the timing loop are scripts/step_timer.py.

    python scripts/decoder_mask_step.py [B=1024] [out.json]
"""
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch
from multi_modal_foundation_model_amd.builders import model_config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
T, STEPS, ROUNDS = 100, 10, 5
MASKS = {"dense": dict(), "causal": dict(causal=True), "sep": dict(sep=True), "causal_sep": dict(causal=True, sep=True)}

runs = {name: make_runner(model_config(**kw), 668, 2, B, T) for name, kw in MASKS.items()}
time_rounds(runs, STEPS, ROUNDS)
res = dict(B=B, T=T, dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS, device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = summarise(r)
res["over_dense"] = {name: res[name]["ms_per_step_median"] / res["dense"]["ms_per_step_median"] for name in MASKS}
emit(res, OUT)
