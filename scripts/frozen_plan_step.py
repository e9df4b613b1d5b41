"""Training-step time of the default config (H = 256, 668 + 2 channels, T = 100) in bf16, dropout on, with parts of the model frozen
(requires_grad = False): all trainable, (b) the trunk frozen (tokenisers + heads train), (a) the encoder and its tokenisers frozen
(a decoder-only fine-tune), (c) only the heads trainable (a linear probe).  The four models alternate in rounds in one process, so that
clock / thermal drift hits all alike.  Per case: ms per step (median, rounds), the launches of the backward per segment against the
all-trainable plan's and the pruned gradient groups (Engine.backward_report).

    python scripts/frozen_plan_step.py [B=1024] [out.json] [steps|kernel|both]

A tree without Engine.backward_report (the parent commit: it honours requires_grad where gradients are handed out and launches the whole
backward) runs the same four cases and reports the plan's launch counts: run it there in the same session for the baseline.

`kernel`: the front half of the fused MLP backward (mmfm_mlp_bwd, dx == NULL) with t1 / g and without (du only, MMFM_MLP_DX_ONLY) at
R = B x 200 rows, seven alternating rounds of 200 launches.  The operands of either form (735 MB / 420 MB at R = 204,800) exceed the
256 MB Infinity Cache, and every launch reads and writes all of them, so no launch finds its operands cached (scripts/dw_slope.py)."""
import fnmatch
import statistics
import sys

from step_timer import O, emit, summarise, time_rounds, to_dev, torch, warm_runner
from multi_modal_foundation_model_amd.builders import build_model, model_config

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
WHICH = sys.argv[3] if len(sys.argv) > 3 else "both"
T, STEPS, ROUNDS = 100, 10, 5
K_ROUNDS, K_LAUNCHES = 7, 200

# case -> (fnmatch patterns, True: they name the trainable parameters / False: the frozen ones)
CASES = {
    "all_trainable": ([], False),
    "b_trunk_frozen": (["encoder_embeddings.*", "decoder_embeddings.*"], True),
    "a_decoder_only": (["encoder.*", "encoder_embeddings.*"], False),
    "c_heads_only": (["decoder_embeddings.*.out.*"], True),
}


def frozen_runner(pats, trainable):
    """step_timer.make_runner with the parameters the patterns select frozen before the optimiser is made."""
    model = build_model(model_config(), 668, 2, seed=42)
    model.compute_dtype = "bf16"
    model.cuda().train()
    for k, p in model.named_parameters():
        if pats and any(fnmatch.fnmatchcase(k, pat) for pat in pats) != trainable:
            p.requires_grad_(False)
    return warm_runner(model, to_dev(O.make_mod_dict(O.synth_batch(B, T, 668, 2, seed=0), "encoding"), targets=False))


def steps():
    runs = {name: frozen_runner(*spec) for name, spec in CASES.items()}
    time_rounds(runs, STEPS, ROUNDS)
    res = {}
    for name, r in runs.items():
        res[name] = summarise(r, spread=True, parameters=True)
        res[name]["ms_per_step_min_max"] = [min(r["ms"]), max(r["ms"])]
        res[name]["trainable_parameters"] = sum(p.numel() for p in r["model"].parameters() if p.requires_grad)
        eng = r["model"]._engine
        if hasattr(eng, "backward_report"):
            rep = eng.backward_report(B, T)
            res[name].update(backward_segments=[list(s) for s in rep["segments"]], pruned_groups=rep["pruned"])
        else:
            res[name]["backward_segments"] = [[seg, len(entries), len(entries)] for seg, entries in eng._last["bwd"]]
    return res


def kernel():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    R, BF = B * 2 * T, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=g, device="cuda") * scale
    e_up = dict(W=rnd(512, 256, scale=1 / 16), gamma=1 + 0.3 * rnd(256), beta=0.2 * rnd(256), bias=0.1 * rnd(512),
                Wp=torch.empty(512, 256, device="cuda", dtype=BF), bp=torch.empty(512, device="cuda"))
    e_dn = dict(W=rnd(256, 512, scale=1 / 22), WpT=torch.empty(512, 256, device="cuda", dtype=BF))
    table, n, tiles = K.prep_table([e_up, e_dn], "cuda")
    K.prep_weights(table, n, tiles)
    xh, dy = torch.nn.functional.layer_norm(rnd(R, 256), (256,)).to(BF), rnd(R, 256).to(BF)
    rng = torch.zeros(2, dtype=torch.int32, device="cuda")
    K.rng_seed(rng, 1)
    t1, gg, du = (torch.empty(R, w, device="cuda", dtype=BF) for w in (256, 512, 512))
    kw = dict(w_up=e_up["Wp"], b_up=e_up["bp"], xhat=xh, dy=dy, w_down_t=e_dn["WpT"], du=du, dx=None, act=L.MLP_GELU, drop=K.dropout(rng, 1, 0.4))
    plans = {}
    for name, (a, b) in (("full", (t1, gg)), ("du_only", (None, None))):
        plans[name] = []
        K.mlp_bwd(K.mlp_desc(R, t1=a, g=b, **kw), plan=plans[name])
        K.run_plan(plans[name])                                       # warm-up (LDS opt-in)
    torch.cuda.synchronize()
    us = {name: [] for name in plans}
    for _ in range(K_ROUNDS):
        for name, plan in plans.items():
            t0, t1e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(K_LAUNCHES):
                K.run_plan(plan)
            t1e.record()
            torch.cuda.synchronize()
            us[name].append(t0.elapsed_time(t1e) / K_LAUNCHES * 1e3)
    res = {name: dict(us_per_launch_median=statistics.median(v), us_per_launch_min_max=[min(v), max(v)], us_per_launch_rounds=v) for name, v in us.items()}
    res.update(R=R, rounds=K_ROUNDS, launches_per_round=K_LAUNCHES, bytes_moved=dict(full=R * 3584, du_only=R * 2048),
               du_only_below_full_range=res["du_only"]["us_per_launch_median"] < res["full"]["us_per_launch_min_max"][0])
    return res


res = dict(B=B, T=T, dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS, device=torch.cuda.get_device_name(0))
if WHICH in ("steps", "both"):
    res["cases"] = steps()
if WHICH in ("kernel", "both"):
    res["mlp_bwd_front_half"] = kernel()
emit(res, OUT)
