"""Does the default step pay for the added loss kinds?  Two measurements in one process, after a warm-up:

 1. the spike head's loss launches of the default step - mmfm_masked_loss_fwd / _bwd, kind 0, bf16, R = 102,400 rows, N = 668, 30 %
    of the rows masked - on this library and on the parent commit's library (a second libmmfm_hip.so given on the command line),
    on the same buffers, alternating in rounds; and on this library through mmfm_masked_loss_kind_fwd / _bwd as well;
 2. the whole bf16 training step of the default model at B = 1024, dropout on.

    python scripts/loss_family_step.py PARENT_LIB [out.json] [B=1024]

Build PARENT_LIB from the parent commit (`make -C multi_modal_foundation_model_amd/csrc OUT=/some/where/libmmfm_hip_parent.so` in a
checkout of it).  Acceptance: this library's medians lie within the span of the parent's own rounds (or below it).
"""
import ctypes as C
import statistics
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd.builders import model_config

PARENT = sys.argv[1]
OUT = sys.argv[2] if len(sys.argv) > 2 else None
B = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
T, N, ROUNDS, LAUNCHES, STEPS = 100, 668, 7, 200, 10
R = B * T


def load(path):
    lib = C.CDLL(path)
    for name in ("mmfm_masked_loss_fwd", "mmfm_masked_loss_bwd", "mmfm_masked_loss_workspace"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L._PROTOS[name]
    return lib


new, old = L.lib(), load(PARENT)
g = torch.Generator(device="cuda").manual_seed(0)
pred = (torch.randn(R, N, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
tgt = torch.poisson(torch.full((R, N), 0.3, device="cuda"), generator=g)
tokmask = (torch.rand(B, 2 * T, generator=g, device="cuda") < 0.3).to(torch.uint8)
rowmask = tokmask[:, :T]
ws = torch.empty(new.mmfm_masked_loss_workspace(R, N) // 4, device="cuda")
out, gout = torch.empty(1, device="cuda"), torch.ones(1, device="cuda")
inv_n = torch.tensor([1.0 / (int(rowmask.sum()) * N)], device="cuda")
dpred = torch.empty_like(pred)
st = torch.cuda.current_stream().cuda_stream
P = lambda t: t.data_ptr()  # noqa: E731
fwd_args = (P(pred), P(tgt), P(rowmask), 2 * T, T, R, N, P(out), P(ws), ws.numel() * 4, st)
bwd_args = (P(pred), P(tgt), P(rowmask), 2 * T, T, R, N, P(gout), P(inv_n), P(dpred), st)
CALLS = {
    "parent": (lambda: old.mmfm_masked_loss_fwd(L.BF16, 0, *fwd_args), lambda: old.mmfm_masked_loss_bwd(L.BF16, 0, *bwd_args)),
    "this": (lambda: new.mmfm_masked_loss_fwd(L.BF16, 0, *fwd_args), lambda: new.mmfm_masked_loss_bwd(L.BF16, 0, *bwd_args)),
    "this_kind_entry": (lambda: new.mmfm_masked_loss_kind_fwd(L.BF16, 0, 0.0, 0, *fwd_args),
                        lambda: new.mmfm_masked_loss_kind_bwd(L.BF16, 0, 0.0, 0, *bwd_args)),
}


def timed(call, n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        rc = call()
        if rc:
            raise RuntimeError(f"loss launch failed ({rc})")
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n * 1e3          # us per launch


bits = {}
for name, (f, b) in CALLS.items():                  # warm-up, and the three must agree bit for bit
    timed(f, 20), timed(b, 20)
    bits[name] = (out.clone(), dpred.clone())
same_bits = all(torch.equal(bits[k][0], bits["parent"][0]) and torch.equal(bits[k][1].view(torch.int16), bits["parent"][1].view(torch.int16))
                for k in bits)
us = {name: dict(fwd=[], bwd=[]) for name in CALLS}
for _ in range(ROUNDS):
    for name, (f, b) in CALLS.items():
        us[name]["fwd"].append(timed(f, LAUNCHES))
        us[name]["bwd"].append(timed(b, LAUNCHES))
res = dict(B=B, T=T, N=N, R=R, masked_rows=int(rowmask.sum()), rounds=ROUNDS, launches_per_round=LAUNCHES, device=torch.cuda.get_device_name(0),
           kind0_bits_identical_to_parent=bool(same_bits), loss_us={})
for name, d in us.items():
    res["loss_us"][name] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v) for k, v in d.items()}
for k in ("fwd", "bwd"):
    par, cur = res["loss_us"]["parent"][k], res["loss_us"]["this"][k]
    res["loss_us"][f"{k}_this_median_within_parent_span"] = bool(par["min"] <= cur["median"] <= par["max"])
    res["loss_us"][f"{k}_this_median_at_most_parent_max"] = bool(cur["median"] <= par["max"])       # below the span = faster
del pred, tgt, dpred

# ---- the whole default step
runs = {"step": make_runner(model_config(), 668, 2, B, T)}
time_rounds(runs, STEPS, 5)
res["step"] = dict(summarise(runs["step"]), steps_per_round=STEPS)
emit(res, OUT)
