"""Live rows, per objective: ms per training step of the YAML model in bf16 at B x T = 1024 x 100 with MMFM_LIVE_ROWS=0
and =1, the two runners alternating in rounds on one GPU (step_timer.time_rounds).  `encoding` has every `ap` bin dead, `decoding`
every `behavior` bin, `token_masking` about masker.ratio of both.

    python scripts/live_rows_step.py [--batch 1024] [--steps 10] [--rounds 5] [--out profiles/live_rows_step_B1024.json]"""
import argparse
import gc
import os

import step_timer as ST
import torch
from multi_modal_foundation_model_amd.builders import load_config

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

cfg = load_config()
res = dict(B=a.batch, T=100, dtype="bf16", steps_per_round=a.steps, rounds=a.rounds, objectives={})
for objective in ("encoding", "token_masking", "decoding"):
    runs = {}
    for live in ("0", "1"):
        os.environ["MMFM_LIVE_ROWS"] = live            # read when the plan is built, inside make_runner's warm-up steps
        runs[live] = ST.make_runner(cfg.model, 668, 2, a.batch, 100, objective=objective)
        names = [fn.__name__ for fn, _, _ in runs[live]["model"]._engine._last["fwd"]]
        assert ("mmfm_gemm_live" in names) == (live == "1")
    ST.time_rounds(runs, a.steps, a.rounds)
    r = {f"live_rows_{k}": ST.summarise(v, spread=True) for k, v in runs.items()}
    r["saved_ms"] = r["live_rows_0"]["ms_per_step_median"] - r["live_rows_1"]["ms_per_step_median"]
    res["objectives"][objective] = r
    del runs
    gc.collect()
    torch.cuda.empty_cache()
os.environ.pop("MMFM_LIVE_ROWS", None)
ST.emit(res, a.out)
