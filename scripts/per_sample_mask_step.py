"""What per-sample token masking (MultiModal.per_sample_mask) costs.  One process, after a warm-up:

 1. the stitch launches alone at the default step's shape - bf16, B = 1024, two modalities x 100 bins, H = 256, max_F 100, with a
    position table, dropout 0.2 on d_tok - seven rounds of 100 launches alternating: this library's existing entry points
    (mmfm_stitch_fwd / mmfm_stitch_bwd, one shared keep row), the _rows pair at keep_ld = 0 (the same row) and at keep_ld = L (every
    sample's own row, 30 % masked), and - where the path of another build of libmmfm_hip.so is given, the parent commit's - that
    library's mmfm_stitch_fwd / mmfm_stitch_bwd on the same tensors;
 2. one training step of the default model per objective, switch off against switch on, alternating in rounds of ten steps, with the
    call counts of both plans.

    python scripts/per_sample_mask_step.py [out.json] [B=1024] [parent libmmfm_hip.so | -] [kernels]        (kernels: part 1 alone)
"""
import ctypes as C
import statistics
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch
from multi_modal_foundation_model_amd import _lib as L, ops as K
from multi_modal_foundation_model_amd.builders import model_config

OUT = sys.argv[1] if len(sys.argv) > 1 else None
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
PARENT = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else None
KERNELS_ONLY = len(sys.argv) > 4 and sys.argv[4] == "kernels"
T, M, H, MAX_F, ROUNDS, LAUNCHES, STEPS, P_DROP = 100, 2, 256, 100, 7, 100, 10, 0.2
Lq = M * T

g = torch.Generator(device="cuda").manual_seed(0)
tok = torch.randn(B * T, H, generator=g, device="cuda").to(torch.bfloat16)
dx = torch.randn(B, Lq, H, generator=g, device="cuda").to(torch.bfloat16)
x, emb, d_tok = torch.empty_like(dx), torch.empty_like(dx), torch.empty_like(tok)
mod_row, pos = torch.randn(H, generator=g, device="cuda"), torch.randn(MAX_F, H, generator=g, device="cuda")
d_mod, d_pos = torch.zeros(H, device="cuda"), torch.zeros(MAX_F, H, device="cuda")
ts = torch.arange(T, dtype=torch.int64, device="cuda")[None].repeat(B, 1).contiguous()
keep = (torch.rand(B, Lq, generator=g, device="cuda") > 0.3).to(torch.uint8)
keep0 = keep[0].contiguous()
ws = torch.empty(max(1, L.lib().mmfm_stitch_bwd_workspace(L.BF16, B, T, Lq, H, MAX_F) // 4), device="cuda")
state = torch.zeros(2, dtype=torch.int32, device="cuda")
K.rng_seed(state, 1)
drop = K.dropout(state, 7, P_DROP)

CALLS = {
    "existing_fwd": lambda: K.stitch_fwd(tok, mod_row, pos, ts, keep0, x, emb, B, T, Lq, 1, H, MAX_F),
    "existing_bwd": lambda: K.stitch_bwd(dx, None, ts, keep0, drop, d_tok, d_mod, d_pos, False, False, B, T, Lq, 1, H, MAX_F, ws),
    "rows_shared_fwd": lambda: K.stitch_fwd_rows(tok, mod_row, pos, ts, keep0, 0, None, x, emb, B, T, Lq, T, H, MAX_F),
    "rows_shared_bwd": lambda: K.stitch_bwd_rows(dx, None, ts, keep0, 0, None, drop, d_tok, d_mod, d_pos, False, False, B, T, Lq, T, H, MAX_F, ws),
    "rows_per_sample_fwd": lambda: K.stitch_fwd_rows(tok, mod_row, pos, ts, keep, Lq, None, x, emb, B, T, Lq, T, H, MAX_F),
    "rows_per_sample_bwd": lambda: K.stitch_bwd_rows(dx, None, ts, keep, Lq, None, drop, d_tok, d_mod, d_pos, False, False, B, T, Lq, T, H, MAX_F, ws),
}
if PARENT:
    par = C.CDLL(PARENT)
    for name in ("mmfm_stitch_fwd", "mmfm_stitch_bwd"):
        getattr(par, name).restype, getattr(par, name).argtypes = L._PROTOS[name]
    st = lambda: torch.cuda.current_stream().cuda_stream
    ptr = K.P
    CALLS["parent_fwd"] = lambda: L.check(par.mmfm_stitch_fwd(L.BF16, ptr(tok), ptr(mod_row), ptr(pos), ptr(ts), ptr(keep0), ptr(x), ptr(emb), B, T,
                                                              Lq, 1, H, MAX_F, st()), "parent mmfm_stitch_fwd")
    CALLS["parent_bwd"] = lambda: L.check(par.mmfm_stitch_bwd(L.BF16, ptr(dx), None, ptr(ts), ptr(keep0), drop, ptr(d_tok), ptr(d_mod), ptr(d_pos), 0,
                                                              0, B, T, Lq, 1, H, MAX_F, ptr(ws), ws.numel() * 4, st()), "parent mmfm_stitch_bwd")


def timed(call, n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        call()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n * 1e3          # us per call (the backward is several launches)


for call in CALLS.values():
    timed(call, 20)
us = {name: [] for name in CALLS}
for _ in range(ROUNDS):
    for name, call in CALLS.items():
        us[name].append(timed(call, LAUNCHES))
res = dict(B=B, T=T, M=M, H=H, max_F=MAX_F, drop_p=P_DROP, rounds=ROUNDS, launches_per_round=LAUNCHES, device=torch.cuda.get_device_name(0),
           parent_library=bool(PARENT), kernels_us={n: dict(median=statistics.median(v), min=min(v), max=max(v)) for n, v in us.items()})
del tok, dx, x, emb, d_tok, ws
if KERNELS_ONLY:
    emit(res, OUT)
    sys.exit(0)

# ---- one training step of the default model per objective, switch off against on
import step_timer  # noqa: E402
_build = step_timer.build_model
res["step"] = {}
for objective in ("encoding", "decoding", "token_masking"):
    runs = {"off": make_runner(model_config(), 668, 2, B, T, objective=objective)}
    step_timer.build_model = lambda mc, n_ap, n_beh, seed: _build(mc, n_ap, n_beh, seed=seed, per_sample_mask=True)
    try:
        runs["on"] = make_runner(model_config(), 668, 2, B, T, objective=objective)
    finally:
        step_timer.build_model = _build
    time_rounds(runs, STEPS, 5)
    res["step"][objective] = {k: dict(summarise(r, spread=True), steps_per_round=STEPS,
                                      live=[fn.__name__ for fn, _, _ in r["model"]._engine._last["fwd"]].count("mmfm_live_bins"))
                              for k, r in runs.items()}
    del runs
    torch.cuda.empty_cache()
emit(res, OUT)
