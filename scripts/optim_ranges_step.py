"""What do the range-table optimiser launches cost beside the one-launch AdamW?  One process, the default model's flat buffers
(9.4 M parameters, bf16 weight copy on), rounds of launches that alternate between the cases so that clock drift hits all alike:

  parent_adamw_step        mmfm_adamw_step from the parent commit's library (a second libmmfm_hip.so given on the command line)
  adamw_step               mmfm_adamw_step from this library - the same kernel, the two spans should overlap
  ranges_one_group         mmfm_adamw_step_ranges, one range per parameter, one hyper row
  ranges_two_groups        the same with the no-decay split (everything below two dimensions in a second row)
  sumsq_alone              mmfm_grad_sumsq_ranges (both launches; it reads 4 of the 30 bytes per parameter)
  sumsq_plus_clipped_step  mmfm_grad_sumsq_ranges + the clipped range step
  torch_clip_plus_step     torch.nn.utils.clip_grad_norm_ over the parameters' gradient views + mmfm_adamw_step

    python scripts/optim_ranges_step.py PARENT_LIB [out.json]

Build PARENT_LIB from the parent commit (`make -C multi_modal_foundation_model_amd/csrc OUT=/some/where/libmmfm_hip_parent.so` in a
checkout of it).  Expectation, not a gate: ranges_one_group within 10 % of parent_adamw_step's median (both move the same 28 - 30 bytes
per parameter).
"""
import ctypes as C
import statistics
import sys

from step_timer import emit, torch
from multi_modal_foundation_model_amd import _lib as L, ops as K
from multi_modal_foundation_model_amd.builders import build_model, model_config
from multi_modal_foundation_model_amd.optim import adamw_hyper_row

PARENT = sys.argv[1]
OUT = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS, LAUNCHES = 7, 200

model = build_model(model_config(), 668, 2, seed=42).cuda().train()
model.compute_dtype = "bf16"
eng = model.engine()
n = eng.P.numel()
named = dict(eng.params)
spans = sorted((int(eng.layout.entries[k][0]), int(eng.layout.entries[k][0]) + p.numel(), int(p.ndim < 2)) for k, p in named.items())
gen = torch.Generator(device="cuda").manual_seed(0)
eng.G.copy_(torch.randn(n, generator=gen, device="cuda") * 0.01)
m, v = torch.zeros_like(eng.P), torch.zeros_like(eng.P)
rows = [adamw_hyper_row(1e-4, (0.9, 0.999), 1e-8, 0.01, 10), adamw_hyper_row(1e-4, (0.9, 0.999), 1e-8, 0.0, 10)]
hyper = torch.tensor(rows, dtype=torch.float64).to(torch.float32).cuda()
one = K.OptimRanges([(a, b, 0) for a, b, _ in spans], n, 1, device="cuda")
two = K.OptimRanges(spans, n, 2, device="cuda")
for p in named.values():
    p.grad = None
for k, p in named.items():
    p.grad = eng.Gv(k)
params = list(named.values())

old = C.CDLL(PARENT)
old.mmfm_adamw_step.restype, old.mmfm_adamw_step.argtypes = L._PROTOS["mmfm_adamw_step"]
new = L.lib()
st = torch.cuda.current_stream().cuda_stream
ptr = lambda t: t.data_ptr()  # noqa: E731
step_args = (ptr(eng.P), ptr(eng.G), ptr(m), ptr(v), ptr(eng.Pw), n, ptr(hyper), st)


def checked(rc):
    if rc:
        raise RuntimeError(f"launch failed ({rc}): {new.mmfm_last_error().decode()}")


def clipped():
    K.grad_sumsq_ranges(eng.G, one, coef_in=1.0, max_norm=1e9)
    K.adamw_step_ranges(eng.P, eng.G, m, v, eng.Pw, one, hyper, clipped=True)


def torch_clip():
    torch.nn.utils.clip_grad_norm_(params, 1e9)
    checked(new.mmfm_adamw_step(*step_args))


CALLS = {
    "parent_adamw_step": lambda: checked(old.mmfm_adamw_step(*step_args)),
    "adamw_step": lambda: checked(new.mmfm_adamw_step(*step_args)),
    "ranges_one_group": lambda: K.adamw_step_ranges(eng.P, eng.G, m, v, eng.Pw, one, hyper),
    "ranges_two_groups": lambda: K.adamw_step_ranges(eng.P, eng.G, m, v, eng.Pw, two, hyper),
    "sumsq_alone": lambda: K.grad_sumsq_ranges(eng.G, one, coef_in=1.0, max_norm=1e9),
    "sumsq_plus_clipped_step": clipped,
    "torch_clip_plus_step": torch_clip,
}


def timed(call, count):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(count):
        call()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / count * 1e3          # us per call


for call in CALLS.values():
    timed(call, 20)
us = {name: [] for name in CALLS}
for _ in range(ROUNDS):
    timed(CALLS["adamw_step"], 50)                      # unmeasured: the round starts with the clocks the host-bound case before it let drop
    for name, call in CALLS.items():
        us[name].append(timed(call, LAUNCHES if name != "torch_clip_plus_step" else 20))
res = dict(n=n, parameters=len(params), chunk=L.OPTIM_CHUNK, chunks_one_group=one.n_chunks, rounds=ROUNDS, launches_per_round=LAUNCHES,
           torch_clip_calls_per_round=20, device=torch.cuda.get_device_name(0), bytes_per_step=30 * n, us={})
for name, vals in us.items():
    med = statistics.median(vals)
    res["us"][name] = dict(median=med, min=min(vals), max=max(vals), rounds=vals, tb_per_s_at_30_bytes=30 * n / med / 1e6)
par = res["us"]["parent_adamw_step"]
res["adamw_step_median_within_parent_span"] = bool(par["min"] <= res["us"]["adamw_step"]["median"] <= par["max"])
res["ranges_one_group_over_parent_median"] = res["us"]["ranges_one_group"]["median"] / par["median"]
res["ranges_one_group_within_10_percent"] = bool(res["ranges_one_group_over_parent_median"] <= 1.10)
emit(res, OUT)
