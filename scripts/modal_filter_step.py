"""Training-step time of the default config (H = 256, 668 + 2 channels, T = 100) in bf16, dropout on, next to the two unimodal baselines of
the reference's `modal_filter` - DEC, spikes -> behaviour (encoder tokeniser for `ap`, decoder tokeniser and head for `behavior`), and
ENC, behaviour -> spikes - in the same process on the same device: the models alternate in rounds so that clock / thermal drift hits all
alike.  A filtered model's sequences are T long, not 2 T, so its step is not comparable with the default's; it is recorded with its plan's
C calls (= kernel launches of the step plan, one per entry).  Each model steps on an objective that masks something in its decoder's
modalities (default and ENC: encoding, DEC: decoding).

    python scripts/modal_filter_step.py [B=1024] [out.json] [default|all]

`default` measures the default model alone, with the loop of scripts/embedder_opts_step.py default: run it on this commit and that script
on the parent commit in one session to compare the two.
"""
import os
import sys

from step_timer import O, emit, summarise, time_rounds, to_dev, torch, warm_runner
from multi_modal_foundation_model_amd.builders import build_model, model_config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
WHICH = sys.argv[3] if len(sys.argv) > 3 else "all"
T, STEPS, ROUNDS = 100, 10, 5


def make(modal_filter, objective):
    model = build_model(model_config(), 668, 2, seed=42, modal_filter=modal_filter)
    model.compute_dtype = "bf16"
    model.cuda().train()
    return warm_runner(model, to_dev(O.make_mod_dict(O.synth_batch(B, T, 668, 2, seed=0), objective), targets=False))


CONFIGS = {"default": (None, "encoding")}
if WHICH == "all":
    CONFIGS.update(DEC=(dict(input=["ap"], output=["behavior"]), "decoding"), ENC=(dict(input=["behavior"], output=["ap"]), "encoding"))
runs = {name: make(*cfg) for name, cfg in CONFIGS.items()}
time_rounds(runs, STEPS, ROUNDS)
res = dict(B=B, T=T, MMFM_FUSED=os.environ.get("MMFM_FUSED"), dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS,
           fused_mask=runs["default"]["model"]._engine._fused_mask(B * 2 * T), device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = summarise(r, spread=True, parameters=True)
    res[name]["rows"] = r["model"]._engine._last["R"]
emit(res, OUT)
