"""Training-step time of BASELINE configs[4]'s model (H = 512, 8 heads: dh = 64, inter 1024, ap + behavior + lfp, T = 200, L = 600) in
bf16 with dropout on, for the decoder attention-mask switches of mm.yaml: dense (both off), decoder_causal_mask, decoder_sep_mask and
both, in the same process on the same device: the models alternate in rounds so that clock / thermal drift hits all alike.  Also
reports each plan's C calls (= kernel launches of the step plan, one per entry).  Public model API only: with scripts/step_timer.py beside it
the same file measures any commit of this repository (MMFM_LIB selects another build of the library).

    python scripts/decoder_mask_step_dh64.py [B=256] [out.json]
"""
import sys

from step_timer import O, emit, summarise, time_rounds, to_dev, torch, warm_runner
from multi_modal_foundation_model_amd.builders import build_model_mods, model_config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
OUT = sys.argv[2] if len(sys.argv) > 2 else None
T, STEPS, ROUNDS = 200, 10, 5
MODS = [("ap", 668), ("behavior", 2), ("lfp", 128)]
MASKS = {"dense": dict(), "causal": dict(causal=True), "sep": dict(sep=True), "causal_sep": dict(causal=True, sep=True)}


def make(kw):
    model = build_model_mods(model_config(H=512, heads=8, inter=1024, max_F=T, n_modality=3, **kw), MODS, seed=42)
    model.loss_mod["lfp"] = "mse"
    model.compute_dtype = "bf16"
    model.cuda().train()
    return warm_runner(model, to_dev(O.make_mod_dict_mods(O.synth_batch_mods(B, T, MODS, seed=0), MODS, "ap")))


runs = {name: make(kw) for name, kw in MASKS.items()}
time_rounds(runs, STEPS, ROUNDS)
res = dict(B=B, T=T, L=len(MODS) * T, H=512, heads=8, dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS, device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = summarise(r)
res["over_dense"] = {name: res[name]["ms_per_step_median"] / res["dense"]["ms_per_step_median"] for name in MASKS}
emit(res, OUT)
