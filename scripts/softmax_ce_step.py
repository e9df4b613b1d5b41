"""What the softmax cross-entropy costs, and that the default step does not pay for it.  Two measurements, chosen on the command line:

    python scripts/softmax_ce_step.py kernels [out.json]          -> profiles/softmax_ce.json
    python scripts/softmax_ce_step.py step [out.json] [B=1024]    -> one run's entry of profiles/softmax_ce_step_B1024.json

kernels  mmfm_softmax_ce_fwd (rowstat saved) and mmfm_softmax_ce_bwd (rowstat read) alone at R = 102,400 rows (B = 1024, T = 100),
         N = 3, 16 and 668 classes, bf16 and fp32 logits, every row masked, index targets, class weights and smoothing 0.1.  Each
         launch takes the next of K operand sets, K chosen so that the sets together exceed 512 MB - twice the Infinity Cache - and a
         launch never finds its operands cached.  Seven rounds of 200 launches; us per launch, median [min, max]; the bytes a launch
         must move (forward: logits + targets + rowstat written; backward: logits + targets + rowstat read + dpred written) over the
         median, next to the achievable HBM rate DESIGN.md uses (6.3 TB/s).  F.cross_entropy on the same device (probability targets,
         reduction='none', times the mask, summed; forward + backward through autograd, fp32 logits) is a point of comparison, not a
         pass mark: it takes the [R, N] logits in one layout and keeps its own intermediates.
step     the whole bf16 training step of the default two-modality model (no categorical modality: the plan is the parent's, call
         for call), dropout on: five rounds of ten steps after warm-up.  Run it on this commit, on the parent commit's tree, and on this
         commit again, in one session; the parent's median must lie inside the interval of this commit's two runs widened by the parent's
         own span (the rule of DESIGN.md 3n / 3o / 3p).
"""
import statistics
import sys

from step_timer import emit, make_runner, summarise, time_rounds, torch

MODE = sys.argv[1] if len(sys.argv) > 1 else "kernels"
OUT = sys.argv[2] if len(sys.argv) > 2 else None
HBM_ACHIEVABLE = 6.3e12
ROUNDS, LAUNCHES = 7, 200


def timed(call, n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for i in range(n):
        call(i)
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n * 1e3          # us per call


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def kernels():
    import torch.nn.functional as F
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    B, T = 1024, 100
    R = B * T
    res = dict(R=R, rounds=ROUNDS, launches_per_round=LAUNCHES, device=torch.cuda.get_device_name(0), hbm_achievable_TBps=HBM_ACHIEVABLE / 1e12,
               cases={})
    g = torch.Generator(device="cuda").manual_seed(0)
    rowmask = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    gout, inv_n = torch.ones(1, device="cuda"), torch.tensor([1.0 / R], device="cuda")
    for N in (3, 16, 668):
        w = 0.25 + 1.5 * torch.rand(N, generator=g, device="cuda")
        ws = torch.empty(max(1, L.lib().mmfm_softmax_ce_workspace(R, N) // 4), device="cuda")
        for dtype in (torch.bfloat16, torch.float32):
            es = 2 if dtype == torch.bfloat16 else 4
            set_bytes = R * N * (es + 4 + es) + R * 8
            sets = max(2, -(-512 * 2 ** 20 // set_bytes))
            preds = [(torch.randn(R, N, generator=g, device="cuda") * 2).to(dtype) for _ in range(sets)]
            tgts = [F.one_hot(torch.randint(0, N, (R,), generator=g, device="cuda"), N).float() for _ in range(sets)]
            dpreds = [torch.empty(R, N, dtype=dtype, device="cuda") for _ in range(sets)]
            stats = [torch.empty(R, 2, device="cuda") for _ in range(sets)]
            out = torch.empty(1, device="cuda")

            def fwd(i):
                k = i % sets
                K.softmax_ce_fwd(preds[k], tgts[k], w, 0.1, rowmask, T, T, R, N, out, stats[k], ws)

            def bwd(i):
                k = i % sets
                K.softmax_ce_bwd(preds[k], tgts[k], w, 0.1, rowmask, T, T, R, N, stats[k], gout, inv_n, dpreds[k])
            timed(fwd, sets), timed(bwd, sets)              # warm-up, and every rowstat is written before a backward reads it
            us = dict(fwd=[], bwd=[])
            for _ in range(ROUNDS):
                us["fwd"].append(timed(fwd, LAUNCHES))
                us["bwd"].append(timed(bwd, LAUNCHES))
            bytes_ = dict(fwd=R * N * (es + 4) + R * 8, bwd=R * N * (es + 4 + es) + R * 8)
            case = dict(N=N, dtype=str(dtype).split(".")[-1], operand_sets=sets, operand_MB=sets * set_bytes / 2 ** 20)
            for k in ("fwd", "bwd"):
                s = spread(us[k])
                rate = bytes_[k] / (s["median"] * 1e-6)
                case[k] = dict(us=s, bytes=bytes_[k], TBps=rate / 1e12, of_achievable=rate / HBM_ACHIEVABLE)
            if dtype == torch.float32:                      # torch on the same device and operands, forward + backward
                leaves = [p.clone().requires_grad_(True) for p in preds]
                mask = rowmask.view(R).float()

                def ref(i):
                    k = i % sets
                    leaves[k].grad = None
                    (F.cross_entropy(leaves[k], tgts[k], weight=w, label_smoothing=0.1, reduction="none") * mask).sum().mul(1.0 / R).backward()
                timed(ref, sets)
                case["torch_cross_entropy_fwd_bwd_us"] = spread([timed(ref, LAUNCHES) for _ in range(ROUNDS)])
                case["this_fwd_plus_bwd_us_median"] = case["fwd"]["us"]["median"] + case["bwd"]["us"]["median"]
                del leaves
            res["cases"][f"N{N}_{case['dtype']}"] = case
            del preds, tgts, dpreds, stats
            torch.cuda.empty_cache()
    return res


def step():
    from multi_modal_foundation_model_amd.builders import model_config
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    runs = {"step": make_runner(model_config(), 668, 2, B, 100)}
    time_rounds(runs, 10, 5)
    return dict(B=B, T=100, device=torch.cuda.get_device_name(0), steps_per_round=10, **summarise(runs["step"], spread=True))


if __name__ == "__main__":
    if MODE not in ("kernels", "step"):
        raise SystemExit(__doc__)
    emit(kernels() if MODE == "kernels" else step(), OUT)
