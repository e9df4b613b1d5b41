"""What honouring space_attn_mask (MultiModal.neuron_padding) costs.  One process, after a warm-up:

 1. the kernels alone at the default step's spike head - bf16, R = 102,400 rows x N = 668, operands beyond the Infinity Cache, 30 % of
    the rows masked, seven rounds of 200 launches alternating: mmfm_masked_loss_chan_fwd / _bwd under a channel prefix of 668, 484 and
    300 of the 668 channels (one [B, N] mask, every sample the same prefix), mmfm_masked_loss_kind_fwd / _bwd on the same rows (the
    row form: the padding is read and counted), and mmfm_masked_loss_elem_fwd / _bwd on the expanded [B,T,N] product;
 2. one multi-session step of the default model (40 sessions of 300..668 neurons, batch i of session i % 40, spikes right-padded with
    -1, objective `encoding`) with the switch on against the switch off, alternating in rounds in one process.

The default step itself (the switch off: the plan is the parent's, call for call) is timed by `scripts/softmax_ce_step.py step` - five
rounds of ten steps - run on this commit, on the parent commit's tree and library, and on this commit again in one session; its three
records are kept in a file of their own, profiles/neuron_padding_default_step.json, which this script does not write.

    python scripts/neuron_padding_step.py [out.json] [B=1024] [kernels]        (kernels: part 1 alone)
"""
import statistics
import sys

from step_timer import O, build_model, emit, summarise, time_rounds, to_dev, torch, warm_runner
from multi_modal_foundation_model_amd import _lib as L, ops as K
from multi_modal_foundation_model_amd.builders import model_config
from multi_modal_foundation_model_amd.synthetic import session_sizes

OUT = sys.argv[1] if len(sys.argv) > 1 else None
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
KERNELS_ONLY = len(sys.argv) > 3 and sys.argv[3] == "kernels"
T, N, ROUNDS, LAUNCHES, STEPS, SESSIONS = 100, 668, 7, 200, 10, 40
PREFIXES = (668, 484, 300)
R = B * T
HBM_ACHIEVABLE = 6.3e12          # bytes / s, the rate the streaming kernels of this project reach
KIND = (L.LOSS_POISSON_LOG, 0.0, 0)

g = torch.Generator(device="cuda").manual_seed(0)
pred = (torch.randn(R, N, generator=g, device="cuda") * 0.5).to(torch.bfloat16)
tgt = torch.poisson(torch.full((R, N), 0.3, device="cuda"), generator=g)
rowmask = (torch.rand(B, T, generator=g, device="cuda") < 0.3).to(torch.uint8)
rows_on = float(rowmask.float().mean())
ws = torch.empty(K.masked_loss_chan_workspace(R, N) // 4 + 2, device="cuda")
out, cnt, gout = torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"), torch.ones(1, device="cuda")
inv_n = torch.tensor([1.0 / (0.3 * R * N)], device="cuda")
dpred = torch.empty_like(pred)
chan, full = {}, {}
for p in PREFIXES:
    chan[p] = torch.zeros(B, N, dtype=torch.uint8, device="cuda")
    chan[p][:, :p] = 1
    full[p] = (rowmask[:, :, None] * chan[p][:, None, :]).contiguous()

RN = R * N
CALLS = {"row_fwd": lambda: K.masked_loss_kind_fwd(*KIND, pred, tgt, rowmask, T, T, R, N, out, ws),
         "row_bwd": lambda: K.masked_loss_kind_bwd(*KIND, pred, tgt, rowmask, T, T, R, N, gout, inv_n, dpred)}
# bytes a launch moves: pred (2) and target (4) of the set elements; a backward also writes every element of dpred (2).  The chan
# form requests the sample's N channel-mask bytes once per MASKED row in both directions (the [B,N] mask is 684 KB in all and stays in
# cache: counting it as traffic is generous); the element form reads its [B,T,N] mask in full
BYTES = {"row_fwd": rows_on * RN * 6, "row_bwd": rows_on * RN * 6 + RN * 2}
for p in PREFIXES:
    CALLS[f"chan{p}_fwd"] = lambda p=p: K.masked_loss_chan_fwd(*KIND, pred, tgt, rowmask, T, T, R, N, chan[p], out, cnt, ws)
    CALLS[f"chan{p}_bwd"] = lambda p=p: K.masked_loss_chan_bwd(*KIND, pred, tgt, rowmask, T, T, R, N, chan[p], gout, inv_n, dpred)
    CALLS[f"elem{p}_fwd"] = lambda p=p: K.masked_loss_elem_fwd(*KIND, pred, tgt, full[p], B, T, N, out, cnt, ws)
    CALLS[f"elem{p}_bwd"] = lambda p=p: K.masked_loss_elem_bwd(*KIND, pred, tgt, full[p], B, T, N, gout, inv_n, dpred)
    BYTES[f"chan{p}_fwd"] = rows_on * R * p * 6 + rows_on * R * N
    BYTES[f"chan{p}_bwd"] = rows_on * R * p * 6 + RN * 2 + rows_on * R * N
    BYTES[f"elem{p}_fwd"] = rows_on * R * p * 6 + RN
    BYTES[f"elem{p}_bwd"] = rows_on * R * p * 6 + RN * 2 + RN


def timed(call, n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        call()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n * 1e3          # us per launch


# the forms agree before they are timed: the chan form's sum and count are the element form's bits on the expanded product
for p in PREFIXES:
    CALLS[f"chan{p}_fwd"]()
    a = (out.clone(), cnt.clone())
    CALLS[f"elem{p}_fwd"]()
    assert torch.equal(a[0].view(torch.int32), out.view(torch.int32)) and torch.equal(a[1], cnt), p
for call in CALLS.values():
    timed(call, 20)
us = {name: [] for name in CALLS}
for _ in range(ROUNDS):
    for name, call in CALLS.items():
        us[name].append(timed(call, LAUNCHES))
res = dict(B=B, T=T, N=N, R=R, rows_masked=rows_on, rounds=ROUNDS, launches_per_round=LAUNCHES, device=torch.cuda.get_device_name(0), kernels_us={})
for name, v in us.items():
    med = statistics.median(v)
    res["kernels_us"][name] = dict(median=med, min=min(v), max=max(v), bytes=BYTES[name], fraction_of_achievable_hbm=BYTES[name] / (med * 1e-6) / HBM_ACHIEVABLE)
del pred, tgt, dpred, chan, full
if KERNELS_ONLY:
    emit(res, OUT)
    sys.exit(0)

# ---- one multi-session step, the switch on against off
model = build_model(model_config(), N, 2, seed=42)
model.compute_dtype = "bf16"
model.cuda().train()
md = to_dev(O.make_mod_dict(O.synth_batch(B, T, N, 2, seed=0), "encoding"), targets=False)
spikes = md["ap"]["inputs"].clone()
sizes, state = session_sizes(SESSIONS, N), dict(i=0)
pool = []
for n in sizes:                        # session k: n_k real channels, the others padded with -1 and cleared in the mask
    x, v = spikes.clone(), torch.ones(B, N, dtype=torch.int64, device="cuda")
    x[:, :, n:] = -1.0
    v[:, n:] = 0
    pool.append((x, v))


def next_session(switch):
    x, v = pool[state["i"] % SESSIONS]
    state["i"] += 1
    md["ap"].update(inputs=x, targets=x, space_attn_mask=v)
    model.neuron_padding = switch


runs = {"off": warm_runner(model, md, pre_step=lambda: next_session(False)), "on": warm_runner(model, md, pre_step=lambda: next_session(True))}
time_rounds(runs, STEPS, 5)
res["multi_session_step"] = dict({k: dict(summarise(r, spread=True), steps_per_round=STEPS) for k, r in runs.items()}, sessions=SESSIONS,
                                 padded_fraction=1.0 - sum(sizes) / (SESSIONS * N), objective="encoding")
emit(res, OUT)
