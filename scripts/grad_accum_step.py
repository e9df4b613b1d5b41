"""What does gradient accumulation cost, and does the ordinary step pay for it?  Default config (H = 256, 668 + 2 channels, T = 100),
bf16, dropout on.

    python scripts/grad_accum_step.py run B out.json [steps|kernel|both]
    python scripts/grad_accum_step.py merge profiles/grad_accum_step.json B=this_1.json,parent.json,this_2.json [B=...] [kernel.json]

`run` measures the tree it lies in (copy it into a checkout of the parent commit, built there, for the parent's numbers), in one
process, the cases alternating in five rounds of ten steps so that clock / thermal drift hits all alike:

  ordinary_step      (a) forward, backward, optimiser step, scheduler step, zero_grad(): k = 1, every path that existed before
  accumulating_step  (b) forward + backward WITHOUT zero_grad(): the engine adds into G.  The parent clones G (37.6 MB, allocated
                     fresh), runs the backward as one unit and adds the clone back; this commit stashes the accumulating runs into its
                     persistent buffer and adds them back behind the backward (mmfm_grad_accumulate)
  kernel             (c) mmfm_grad_accumulate alone, both modes over the model's whole gradient buffer, seven alternating rounds of 200
                     launches: stash moves 8 bytes per element, add 12 (skipped in a tree without the kernel)

`merge` applies the rule of DESIGN.md 3n / 3o / 3p to (a) per batch size - the parent's median must lie inside the interval of this
commit's two runs (before and after the parent's, same session), widened by the parent's own span - and puts (b) side by side.
"""
import json
import statistics
import sys

MODE = sys.argv[1]
T, STEPS, ROUNDS = 100, 10, 5
K_ROUNDS, K_LAUNCHES, PAIRS = 7, 200, 5
HBM_PEAK_TB_S, HBM_ACHIEVABLE_TB_S = 8.0, 6.3


def run(B, out, which):
    from step_timer import O, emit, summarise, time_rounds, to_dev, torch, warm_runner
    from multi_modal_foundation_model_amd import ops as K
    from multi_modal_foundation_model_amd.builders import build_model, model_config

    def runner(accumulate):
        model = build_model(model_config(), 668, 2, seed=42)
        model.compute_dtype = "bf16"
        model.cuda().train()
        md = to_dev(O.make_mod_dict(O.synth_batch(B, T, 668, 2, seed=0), "encoding"), targets=False)
        r = warm_runner(model, md)
        if accumulate:
            def step():
                out = model({m: dict(d) for m, d in md.items()})
                out.loss.backward()                       # no zero_grad(): every backward but the first accumulates
                return out.loss
            for _ in range(3):
                step()
            r["step"] = step
        return r

    res = dict(B=B, T=T, dtype="bf16", steps_per_round=STEPS, rounds=ROUNDS, device=torch.cuda.get_device_name(0),
               has_kernel=hasattr(K, "grad_accumulate"))
    if which in ("steps", "both"):
        runs = dict(ordinary_step=runner(False), accumulating_step=runner(True))
        time_rounds(runs, STEPS, ROUNDS)
        res["cases"] = {}
        for name, r in runs.items():
            res["cases"][name] = summarise(r, spread=True)
            res["cases"][name]["ms_per_step_min_max"] = [min(r["ms"]), max(r["ms"])]
        eng = runs["accumulating_step"]["model"]._engine
        res["gradient_elements"] = eng.G.numel()
        res["stash_allocated"] = getattr(eng, "_stash", None) is not None
    if which in ("kernel", "both") and res["has_kernel"]:
        from multi_modal_foundation_model_amd import _lib as L
        n = build_model(model_config(), 668, 2, seed=42).cuda().engine().G.numel()
        gen = torch.Generator(device="cuda").manual_seed(0)
        # one pair of buffers (75 MB) would stay in the 256 MB Infinity Cache from launch to launch: the launches walk PAIRS pairs
        # (376 MB), so that each finds its operands in HBM.  Values stay small: the add runs on 0.01-scale data a few hundred times
        pairs = [tuple(torch.randn(n, generator=gen, device="cuda") * 0.01 for _ in range(2)) for _ in range(PAIRS)]
        modes = dict(stash=(L.GRAD_STASH, 8), add=(L.GRAD_ADD, 12))
        us = {name: [] for name in modes}
        for mode, _ in modes.values():
            for g, stash in pairs:
                K.grad_accumulate(g, stash, 0, n, mode)
        torch.cuda.synchronize()
        for _ in range(K_ROUNDS):
            for name, (mode, _) in modes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(K_LAUNCHES):
                    g, stash = pairs[i % PAIRS]
                    K.grad_accumulate(g, stash, 0, n, mode)
                e1.record()
                torch.cuda.synchronize()
                us[name].append(e0.elapsed_time(e1) / K_LAUNCHES * 1e3)
        res["kernel"] = dict(elements=n, rounds=K_ROUNDS, launches_per_round=K_LAUNCHES, buffer_pairs=PAIRS, hbm_peak_tb_s=HBM_PEAK_TB_S,
                             hbm_achievable_tb_s=HBM_ACHIEVABLE_TB_S)
        for name, (_, nbytes) in modes.items():
            med = statistics.median(us[name])
            res["kernel"][name] = dict(us_per_launch_median=med, us_per_launch_min_max=[min(us[name]), max(us[name])], us_per_launch_rounds=us[name],
                                       bytes_per_launch=nbytes * n, tb_per_s=nbytes * n / med / 1e6)
    emit(res, out)


def merge(out, args):
    res = dict(rule="(a): the parent's median must lie inside [min, max] of this commit's two runs' medians, widened by the parent's own span")
    for a in args:
        if "=" not in a:
            with open(a) as f:
                res["kernel"] = json.load(f)["kernel"]
            continue
        key, files = a.split("=")
        this_1, parent, this_2 = (json.load(open(p)) for p in files.split(","))
        med = lambda r, case: r["cases"][case]["ms_per_step_median"]  # noqa: E731
        lo, hi = sorted((med(this_1, "ordinary_step"), med(this_2, "ordinary_step")))
        span = parent["cases"]["ordinary_step"]["ms_per_step_spread"]
        pm = med(parent, "ordinary_step")
        side = "inside" if lo - span <= pm <= hi + span else ("parent faster" if pm < lo - span else "parent slower")
        acc = dict(parent_clone_path=parent["cases"]["accumulating_step"], this_commit_first=this_1["cases"]["accumulating_step"],
                   this_commit_second=this_2["cases"]["accumulating_step"])
        acc["this_commit_faster"] = max(med(this_1, "accumulating_step"), med(this_2, "accumulating_step")) < med(parent, "accumulating_step")
        res[key] = dict(device=this_1["device"], steps_per_round=this_1["steps_per_round"], rounds=this_1["rounds"],
                        ordinary_step=dict(this_commit_first=this_1["cases"]["ordinary_step"], parent=parent["cases"]["ordinary_step"],
                                           this_commit_second=this_2["cases"]["ordinary_step"], interval_ms=[lo, hi], parent_span_ms=span,
                                           parent_median_ms=pm, verdict=side),
                        accumulating_step=acc)
    print(json.dumps(res, indent=1))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if MODE == "run":
    run(int(sys.argv[2]), sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "both")
elif MODE == "merge":
    merge(sys.argv[2], sys.argv[3:])
else:
    raise SystemExit(__doc__)
