"""Training-step time around head dim 128, bf16, dropout on, one process per comparison.

    python scripts/dh128_step.py default [B=1024] [out.json]
        the default config (H = 256, 8 heads, 668 + 2 channels, T = 100): ms / step and the plan's C calls (81 + 222).  Run it on this
        commit's library and on the parent commit's in one session to compare the two.
    python scripts/dh128_step.py dh128 [B=64] [out.json]
        hidden 1024, 8 heads (dh 128), inter 2048, 5 + 5 layers, T = 100, two modalities (L = 200): the keep-bit kernels
        (csrc/attention_long.hip) next to MMFM_ATTN_KEEPBITS=0 (the general tiled kernels of csrc/attention_bf16.hip), the two models
        alternating in rounds; per model the step time, the attention kernels' device time per step (torch.profiler, kernels whose name
        contains "attn") and their achieved TF/s on the algorithmic 4 (forward) + 10 (backward) B heads L^2 dh flops per attention site.
"""
import os
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch
from multi_modal_foundation_model_amd.builders import model_config

MODE = sys.argv[1] if len(sys.argv) > 1 else "default"
B = int(sys.argv[2]) if len(sys.argv) > 2 else (1024 if MODE == "default" else 64)
OUT = sys.argv[3] if len(sys.argv) > 3 else None
T, STEPS, ROUNDS = 100, 10, 5
N_AP, N_BEH = (668, 2) if MODE == "default" else (96, 2)
WIDE = dict(H=1024, heads=8, inter=2048, n_enc=5, n_dec=5)


def make(kw, keepbits):
    def export():
        os.environ["MMFM_ATTN_KEEPBITS"] = keepbits          # read whenever the engine builds a step plan: set again before every step
    export()
    r = make_runner(model_config(**kw), N_AP, N_BEH, B, T, pre_step=export)
    sites = [s for s in r["model"]._engine.dropout_sites(B, T) if s["kind"] == "attn"]
    return dict(r, sites=len(sites), dh=sites[0]["dh"] if sites else None)


def keepbit_workspaces(r):
    """Asked after the timed rounds: what the plan that ran them handed to the attention sites."""
    return all(s["keepbits"] is not None for s in r["model"]._engine.dropout_sites(B, T) if s["kind"] == "attn")


def attention_ms(step, n=3):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            step()
        torch.cuda.synchronize()
    us = sum(getattr(e, "device_time_total", 0.0) for e in prof.key_averages() if "attn" in e.key)
    return us / n / 1e3


if MODE == "default":
    runs = {"default": make({}, "1")}
else:
    runs = {"keepbits": make(WIDE, "1"), "general": make(WIDE, "0")}
time_rounds(runs, STEPS, ROUNDS)
res = dict(mode=MODE, B=B, T=T, L=2 * T, dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS, device=torch.cuda.get_device_name(0))
for name, r in runs.items():
    res[name] = dict(summarise(r, spread=True), attention_sites=r["sites"], dh=r["dh"], keepbit_workspaces=keepbit_workspaces(r))
    if MODE != "default":
        att = attention_ms(r["step"])
        flops = 14.0 * B * WIDE["heads"] * (2 * T) ** 2 * r["dh"] * r["sites"]
        res[name].update(attention_ms_per_step=att, attention_tflops=flops / (att * 1e-3) / 1e12 if att > 0 else None)
if MODE != "default":
    assert res["keepbits"]["keepbit_workspaces"] and not res["general"]["keepbit_workspaces"], "the two runs took the same attention path"
    res["keepbits_over_general"] = res["keepbits"]["ms_per_step_median"] / res["general"]["ms_per_step_median"]
emit(res, OUT)
