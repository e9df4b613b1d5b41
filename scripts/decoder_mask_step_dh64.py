"""Training-step time of BASELINE configs[4]'s model (H = 512, 8 heads: dh = 64, inter 1024, ap + behavior + lfp, T = 200, L = 600) in
bf16 with dropout on, for the decoder attention-mask switches of mm.yaml: dense (both off), decoder_causal_mask, decoder_sep_mask and
both, in the same process on the same device: the models alternate in rounds so that clock / thermal drift hits all alike.  Also
reports each plan's C calls (= kernel launches of the step plan, one per entry).  Public model API only, so the same file measures any
commit of this repository (MMFM_LIB selects another build of the library).

    python scripts/decoder_mask_step_dh64.py [B=256] [out.json]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi_modal_foundation_model_amd", "src"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

from multi_modal_foundation_model_amd.builders import build_model_mods, make_optimizer, model_config  # noqa: E402
from oracle import mm_oracle as O  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
OUT = sys.argv[2] if len(sys.argv) > 2 else None
T, STEPS, ROUNDS = 200, 10, 5
MODS = [("ap", 668), ("behavior", 2), ("lfp", 128)]
MASKS = {"dense": dict(), "causal": dict(causal=True), "sep": dict(sep=True), "causal_sep": dict(causal=True, sep=True)}


def to_dev(md):
    for d in md.values():
        for k, v in list(d.items()):
            if isinstance(v, torch.Tensor):
                d[k] = v.cuda()
        d["targets_modality"] = d["inputs_modality"]
        d["targets_timestamp"] = d["inputs_timestamp"]
    return md


def make(kw):
    model = build_model_mods(model_config(H=512, heads=8, inter=1024, max_F=T, n_modality=3, **kw), MODS, seed=42)
    model.loss_mod["lfp"] = "mse"
    model.compute_dtype = "bf16"
    model.cuda().train()
    opt, sch = make_optimizer(model, 10000)
    md = to_dev(O.make_mod_dict_mods(O.synth_batch_mods(B, T, MODS, seed=0), MODS, "ap"))

    def step():
        out = model({m: dict(d) for m, d in md.items()})
        out.loss.backward()
        opt.step(); sch.step(); opt.zero_grad()
        return out.loss
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    plan = model._engine._last
    calls = dict(fwd=len(plan["fwd"]), bwd=sum(len(seg) for _, seg in plan["bwd"]))
    return dict(model=model, step=step, calls=calls, ms=[])


runs = {name: make(kw) for name, kw in MASKS.items()}
for _ in range(ROUNDS):
    for name, r in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            loss = r["step"]()
        torch.cuda.synchronize()
        r["ms"].append((time.perf_counter() - t0) / STEPS * 1e3)
        r["loss"] = float(loss)
res = dict(B=B, T=T, L=len(MODS) * T, H=512, heads=8, dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS, device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = dict(ms_per_step_median=statistics.median(r["ms"]), ms_per_step_rounds=r["ms"], plan_calls=r["calls"], last_loss=r["loss"])
res["over_dense"] = {name: res[name]["ms_per_step_median"] / res["dense"]["ms_per_step_median"] for name in MASKS}
print(json.dumps(res, indent=1))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
