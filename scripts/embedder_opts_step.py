"""Training-step time of the default config (H = 256, 668 + 2 channels, T = 100) in bf16, dropout on, next to two models with non-default
embedder options - `act: gelu` on both sides (the forward writes the token_embed pre-activation z, the backward reads it) and
`pos: false` on both sides (no position tables) - in the same process on the same device: the models alternate in rounds so that clock /
thermal drift hits all alike.  Also reports each plan's C calls (= kernel launches of the step plan, one per entry).

    python scripts/embedder_opts_step.py [B=1024] [out.json] [default|all]

`default` measures the default model alone, with the loop of scripts/side_config_step.py default: run it on this commit and that script
on the parent commit in one session to compare the two.
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

from multi_modal_foundation_model_amd.builders import build_model, make_optimizer, model_config  # noqa: E402
from oracle import mm_oracle as O  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
WHICH = sys.argv[3] if len(sys.argv) > 3 else "all"
T, STEPS, ROUNDS = 100, 10, 5


def to_dev(md):
    for d in md.values():
        for k, v in list(d.items()):
            if isinstance(v, torch.Tensor):
                d[k] = v.cuda()
    return md


def make(emb):
    mc = model_config()
    for side in ("encoder", "decoder"):
        mc[side]["embedder"].update(emb)
    model = build_model(mc, 668, 2, seed=42)
    model.compute_dtype = "bf16"
    model.cuda().train()
    opt, sch = make_optimizer(model, 10000)
    md = to_dev(O.make_mod_dict(O.synth_batch(B, T, 668, 2, seed=0), "encoding"))

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
    return dict(model=model, step=step, calls=calls, ms=[], params=sum(p.numel() for p in model.parameters()))


CONFIGS = {"default": {}}
if WHICH == "all":
    CONFIGS.update(act_gelu=dict(act="gelu"), pos_off=dict(pos=False))
runs = {name: make(kw) for name, kw in CONFIGS.items()}
for _ in range(ROUNDS):
    for name, r in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            loss = r["step"]()
        torch.cuda.synchronize()
        r["ms"].append((time.perf_counter() - t0) / STEPS * 1e3)
        r["loss"] = float(loss)
res = dict(B=B, T=T, MMFM_FUSED=os.environ.get("MMFM_FUSED"), dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS,
           fused_mask=runs["default"]["model"]._engine._fused_mask(B * 2 * T), device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = dict(ms_per_step_median=statistics.median(r["ms"]), ms_per_step_rounds=r["ms"], ms_per_step_spread=max(r["ms"]) - min(r["ms"]),
                     plan_calls=r["calls"], parameters=r["params"], last_loss=r["loss"])
for name in runs:
    if name != "default":
        res[name + "_over_default"] = res[name]["ms_per_step_median"] / res["default"]["ms_per_step_median"]
print(json.dumps(res, indent=1))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
