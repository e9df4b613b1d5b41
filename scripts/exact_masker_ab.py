"""Trainer-step time of the default config in bf16 under the three masker streams, in one process on one device:

    default    the trainer's token-mask-only stream (training.exact_masker_stream: false)
    exact      the reference-exact stream, the discarded [B, T, N] draws skipped by MT19937 jump-ahead
    exact_draw the same stream with MMFM_MASKER_JUMP=0: the draws are taken for real (the host-bound figure of earlier commits)

The legs are bench.py's own leg_trainer and alternate in rounds so that clock / thermal drift hits all alike; Python's `random` is
seeded alike before every leg, so every leg walks the same schedule of training objectives.  Also times one jump of the 'ap'
modality's size on the host.

    python scripts/exact_masker_ab.py [B=1024] [out.json]
"""
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multi_modal_foundation_model_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

from bench import leg_trainer  # noqa: E402
from multi_modal_foundation_model_amd.rngjump import advance_cpu_generator  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
OUT = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS, STEPS, WARM = 3, 12, 3
LEGS = {"default": dict(exact=False, jump="1"), "exact": dict(exact=True, jump="1"), "exact_draw": dict(exact=True, jump="0")}

dev = torch.device("cuda", 0)
ms = {name: [] for name in LEGS}
for rnd in range(ROUNDS):
    for name, leg in LEGS.items():
        os.environ["MMFM_MASKER_JUMP"] = leg["jump"]
        random.seed(1234)
        torch.manual_seed(1234)
        ms[name].append(leg_trainer(dev, "bf16", B, exact_masker=leg["exact"], steps=STEPS, warm=WARM) * 1e3)
os.environ.pop("MMFM_MASKER_JUMP", None)

n = 3 * B * 100 * 668
advance_cpu_generator(n)                                   # phi and this block count's polynomial are cached now
host = []
for _ in range(20):
    t0 = time.perf_counter()
    advance_cpu_generator(n)
    host.append((time.perf_counter() - t0) * 1e3)

random.seed(1234)
objectives = [random.sample(['encoding', 'decoding', 'token_masking'], 1)[0] for _ in range(WARM + STEPS)][WARM:]
res = dict(B=B, T=100, dtype="bf16", rounds=ROUNDS, steps_per_round=STEPS, device=torch.cuda.get_device_name(0),
           timed_objectives=objectives, masker_steps_per_round=objectives.count("token_masking"))
for name in LEGS:
    med = statistics.median(ms[name])
    res[name] = dict(ms_per_step_median=med, ms_per_step_rounds=ms[name], samples_per_s=B / med * 1e3)
res["exact_over_default"] = res["exact"]["ms_per_step_median"] / res["default"]["ms_per_step_median"]
res["exact_draw_over_default"] = res["exact_draw"]["ms_per_step_median"] / res["default"]["ms_per_step_median"]
res["host_ms_per_jump"] = dict(n=n, median=statistics.median(host), max=max(host))
print(json.dumps(res, indent=1))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
