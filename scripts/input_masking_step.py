"""What input masking (mask_type: input with MultiModal.input_masking) costs.  One process, after a warm-up:

 1. the kernels alone at the default step's spike head - bf16, R = 102,400 rows x N = 668, operands beyond the Infinity Cache, seven
    rounds of 200 launches alternating: mmfm_masked_loss_elem_fwd / _bwd under a [B,1,N] mask and a full [B,T,N] mask of density 0.3
    against mmfm_masked_loss_kind_fwd / _bwd with 30 % of the rows masked (the row-mask kernels of this library: their source is the
    parent's, unchanged), and mmfm_stage_masked against the `copy_` it replaces;
 2. one MtM step (mode `neuron`, zero_ratio 1) against a token_masking step of the same model, alternating in rounds, and the host time
    of Masker.element_masks per call.

    python scripts/input_masking_step.py [out.json] [B=1024]
"""
import statistics
import sys
import time

from step_timer import O, build_model, emit, summarise, time_rounds, to_dev, torch, warm_runner
from multi_modal_foundation_model_amd import _lib as L, ops as K
from multi_modal_foundation_model_amd.builders import model_config

OUT = sys.argv[1] if len(sys.argv) > 1 else None
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
T, N, ROUNDS, LAUNCHES, STEPS = 100, 668, 7, 200, 10
R = B * T
HBM_ACHIEVABLE = 6.3e12          # bytes / s, the rate the streaming kernels of this project reach

g = torch.Generator(device="cuda").manual_seed(0)
pred = (torch.randn(R, N, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
tgt = torch.poisson(torch.full((R, N), 0.3, device="cuda"), generator=g)
rowmask = (torch.rand(B, T, generator=g, device="cuda") < 0.3).to(torch.uint8)
m_b1n = (torch.rand(B, 1, N, generator=g, device="cuda") < 0.3).to(torch.uint8)
m_btn = (torch.rand(B, T, N, generator=g, device="cuda") < 0.3).to(torch.uint8)
ws = torch.empty(K.masked_loss_elem_workspace(B, T, N) // 4 + 2, device="cuda")
out, cnt, gout = torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"), torch.ones(1, device="cuda")
inv_n = torch.tensor([1.0 / (0.3 * R * N)], device="cuda")
dpred = torch.empty_like(pred)
src = torch.poisson(torch.full((B, T, N), 0.3, device="cuda"), generator=g)
ld = (N + 7) // 8 * 8
dst = torch.zeros(R, ld, dtype=torch.bfloat16, device="cuda")

CALLS = {
    "row_fwd": lambda: K.masked_loss_kind_fwd(L.LOSS_POISSON_LOG, 0.0, 0, pred, tgt, rowmask, T, T, R, N, out, ws),
    "row_bwd": lambda: K.masked_loss_kind_bwd(L.LOSS_POISSON_LOG, 0.0, 0, pred, tgt, rowmask, T, T, R, N, gout, inv_n, dpred),
    "elem_B1N_fwd": lambda: K.masked_loss_elem_fwd(L.LOSS_POISSON_LOG, 0.0, 0, pred, tgt, m_b1n, B, T, N, out, cnt, ws),
    "elem_B1N_bwd": lambda: K.masked_loss_elem_bwd(L.LOSS_POISSON_LOG, 0.0, 0, pred, tgt, m_b1n, B, T, N, gout, inv_n, dpred),
    "elem_BTN_fwd": lambda: K.masked_loss_elem_fwd(L.LOSS_POISSON_LOG, 0.0, 0, pred, tgt, m_btn, B, T, N, out, cnt, ws),
    "elem_BTN_bwd": lambda: K.masked_loss_elem_bwd(L.LOSS_POISSON_LOG, 0.0, 0, pred, tgt, m_btn, B, T, N, gout, inv_n, dpred),
    "stage_B1N": lambda: K.stage_masked(src, m_b1n, B, T, N, dst, ld),
    "stage_BTN": lambda: K.stage_masked(src, m_btn, B, T, N, dst, ld),
    "copy_": lambda: dst.view(B, T, -1)[..., :N].copy_(src, non_blocking=True),
}
RN = R * N
# bytes a launch must move.  The row form skips 70 % of the rows outright; an element form at density 0.3 touches every 128-byte line
# of pred and target (a set element in nearly each), so its traffic is the full tensors plus the mask
BYTES = {"row_fwd": 0.3 * RN * 6, "row_bwd": 0.3 * RN * 6 + RN * 2,
         "elem_B1N_fwd": RN * 6 + B * N, "elem_B1N_bwd": RN * 8 + B * N, "elem_BTN_fwd": RN * 7, "elem_BTN_bwd": RN * 9,
         "stage_B1N": RN * 6 + B * N, "stage_BTN": RN * 7, "copy_": RN * 6}


def timed(call, n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        call()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n * 1e3          # us per launch


for call in CALLS.values():
    timed(call, 20)
us = {name: [] for name in CALLS}
for _ in range(ROUNDS):
    for name, call in CALLS.items():
        us[name].append(timed(call, LAUNCHES))
res = dict(B=B, T=T, N=N, R=R, rounds=ROUNDS, launches_per_round=LAUNCHES, device=torch.cuda.get_device_name(0), kernels_us={})
for name, v in us.items():
    med = statistics.median(v)
    res["kernels_us"][name] = dict(median=med, min=min(v), max=max(v), bytes=BYTES[name], fraction_of_achievable_hbm=BYTES[name] / (med * 1e-6) / HBM_ACHIEVABLE)
del pred, tgt, dpred, src, dst, m_btn

# ---- one MtM step against a token_masking step of the same model
model = build_model(model_config(), 668, 2, seed=42, input_masking=True)
model.compute_dtype = "bf16"
model.cuda().train()
batch = O.synth_batch(B, T, 668, 2, seed=0)
md_tok = to_dev(O.make_mod_dict(batch, "token_masking"), targets=False)
md_mtm = {m: dict(d, masking_mode="neuron") for m, d in md_tok.items()}
runs = {"token_masking": warm_runner(model, md_tok), "mtm_neuron": warm_runner(model, md_mtm)}
time_rounds(runs, STEPS, 5)
res["step"] = {k: dict(summarise(r), steps_per_round=STEPS) for k, r in runs.items()}
model.masker.mode = "neuron"
x = md_tok["ap"]["inputs"]
host = []
for _ in range(20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.masker.element_masks(x, md_tok["ap"]["inputs_regions"])
    host.append((time.perf_counter() - t0) * 1e3)
res["element_masks_host_ms"] = dict(median=statistics.median(host), min=min(host), max=max(host))
emit(res, OUT)
