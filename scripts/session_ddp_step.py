"""What do the span kernels of the sparse session all-reduce cost?  One MI355X, no second rank: the collective itself is not measured.

    python scripts/session_ddp_step.py profiles/session_ddp.json

The read-out block of 8 of 40 sessions, sizes and P as `train_multi_modal.py --use_session --n_sessions 40` builds them (n_k from
synthetic.session_sizes(40, 668), P = 668): per session a [n_k, P] weight and an [n_k] bias in 32-byte aligned slots of a flat fp32
buffer, packed spans on multiples of four elements - the table EngineDDP builds at `head`.  mmfm_span_gather and mmfm_span_scatter
each move 8 bytes per element; for scale, mmfm_grad_accumulate's stash over the same number of elements in the same process.
Seven alternating rounds of 100 launches; the launches walk six buffer sets and five groups of sessions, so that no launch finds its
operands in the 256 MB Infinity Cache.  Figures are us per launch as median [min, max] of the rounds."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_modal_foundation_model_amd import _lib as L  # noqa: E402
from multi_modal_foundation_model_amd import ops as K  # noqa: E402
from multi_modal_foundation_model_amd.synthetic import session_sizes  # noqa: E402

N_SESSIONS, PER_STEP, N_AP, WIDTH = 40, 8, 668, 668
ROUNDS, LAUNCHES, SETS = 7, 100, 6
align = lambda n, a: (n + a - 1) // a * a  # noqa: E731


def main(out):
    sizes = session_sizes(N_SESSIONS, N_AP)
    entries, n = [], 0                                   # (session, offset, length) in layout order: weight, bias per session
    for k, nk in enumerate(sizes):
        for length in (nk * WIDTH, nk):
            n = align(n, 8)
            entries.append((k, n, length))
            n += length
    n = align(n, 64)
    groups = []
    for g0 in range(0, N_SESSIONS, PER_STEP):
        rows, s = [], 0
        for k, off, length in entries:
            if g0 <= k < g0 + PER_STEP:
                rows.append((off, s, length, 1))
                s = align(s + length, 4)
        groups.append((rows, s))
    cap = max(s for _, s in groups)
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = [(torch.randn(n, generator=gen, device="cuda") * 0.01, torch.zeros(cap, device="cuda"), torch.empty(n, device="cuda")) for _ in range(SETS)]
    tables = [K.span_table(rows, n, cap).cuda() for rows, _ in groups]
    elems = statistics.mean(sum(r[2] for r in rows) for rows, _ in groups)

    def gather(i):
        G, stage, _ = sets[i % SETS]
        K.span_gather(G, stage, tables[i % len(groups)], len(groups[i % len(groups)][0]))

    def scatter(i):
        G, stage, _ = sets[i % SETS]
        K.span_scatter(stage, G, tables[i % len(groups)], len(groups[i % len(groups)][0]))

    def stash(i):                                        # the same number of elements, one contiguous range
        G, _, st = sets[i % SETS]
        lo = min(groups[i % len(groups)][0][0][0], n - int(elems))
        K.grad_accumulate(G, st, lo, lo + int(elems), L.GRAD_STASH)

    cases = dict(span_gather=gather, span_scatter=scatter, grad_accumulate_stash=stash)
    us = {name: [] for name in cases}
    for fn in cases.values():
        for i in range(SETS * len(groups)):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(LAUNCHES):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    res = dict(device=torch.cuda.get_device_name(0), n_sessions=N_SESSIONS, sessions_per_step=PER_STEP, width=WIDTH, sizes=sizes,
               spans_per_launch=2 * PER_STEP, elements_per_launch_mean=elems, block_elements=n, rounds=ROUNDS, launches_per_round=LAUNCHES,
               buffer_sets=SETS, session_groups=len(groups))
    for name in cases:
        med = statistics.median(us[name])
        res[name] = dict(us_per_launch_median=med, us_per_launch_min_max=[min(us[name]), max(us[name])], us_per_launch_rounds=us[name],
                         bytes_per_launch=8 * elems, tb_per_s=8 * elems / med / 1e6)
    print(json.dumps(res, indent=1))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
