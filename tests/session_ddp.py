"""Shared by the tests of data parallelism over per-session layers (tests/test_session_ddp_cpu.py, tests/test_session_ddp_gpu.py): the
session mixes of the two ranks, a spawner that gives every worker its own time limit and checks its exit status, and the rule's
arithmetic done through the span table on flat numpy buffers."""
import socket
import time

import numpy as np
import torch.multiprocessing as mp

WORLD, B, T, P, N_MAX = 2, 4, 8, 8, 12
SIZES = (12, 7, 9)                       # sessions of "ap"
# (sessions of rank 0's samples, of rank 1's, synchronising?, zero_grad() in front?)
SCHEDULE = [
    ([0, 0, 0, 0], [1, 1, 1, 1], True, True),            # step 0: session 2 is nowhere
    ([1, 1, 1, 1], [1, 1, 1, 1], True, True),            # step 1
    ([0, 2, 2, 1], [1, 1, 1, 1], True, True),            # step 2
    ([0, 0, 0, 0], [1, 1, 1, 1], False, False),          # one group of two micro-batches, the first under no_sync(), and zero_grad()
    ([2, 2, 2, 2], [1, 1, 1, 1], True, False),           # omitted in front of it: step 2's gradients are still there
]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(worker, args, world=WORLD, limit=120.0):
    """Start `worker(rank, *args)` once per rank, each process under its own time limit; a worker that exits with a status other
    than 0 or outlives its limit fails the test (the others are ended first)."""
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=worker, args=(rank,) + tuple(args)) for rank in range(world)]
    t0 = time.monotonic()
    for p in procs:
        p.start()
    status = []
    for p in procs:
        p.join(max(0.0, limit - (time.monotonic() - t0)))
        if p.is_alive():
            for q in procs:
                q.kill()
            raise AssertionError(f"a worker outlived its limit of {limit} s")
        status.append(p.exitcode)
    assert status == [0] * world, f"worker exit status {status}"


def groups(schedule=SCHEDULE):
    """The schedule cut into groups: lists of step indices, each closed by its synchronising step."""
    out, cur = [], []
    for i, step in enumerate(schedule):
        cur.append(i)
        if step[2]:
            out.append(cur)
            cur = []
    assert not cur
    return out


def through_the_table(layout, rule, grads):
    """The rule's arithmetic as EngineDDP does it, on numpy: per rank a flat buffer G (NaN wherever nothing is held), the gather of the
    rule's rows (dead spans: zeros, never read), the mean of the packed buffers, the scatter back.  grads[r]: name -> array or None.
    Returns per rank name -> array for the names the rule updates."""
    world = len(grads)
    out = [dict() for _ in range(world)]
    for which in ("out", "in"):
        total = max((s + n for rows in (rule["tables"][r][which] for r in range(world)) for _, s, n, _ in rows), default=0)
        stages = []
        for r in range(world):
            G = np.full(layout.n, np.nan, dtype=np.float32)
            for name, g in grads[r].items():
                if g is not None and name in layout.entries:
                    off = layout.entries[name][0]
                    G[off:off + g.size] = np.asarray(g, dtype=np.float32).ravel()
            stage = np.full(total, np.nan, dtype=np.float32)
            for g_off, s_off, n, live in rule["tables"][r][which]:
                stage[s_off:s_off + n] = G[g_off:g_off + n] if live else 0.0
            stages.append(stage)
        mean = (np.sum(stages, axis=0, dtype=np.float32) * np.float32(1.0 / world)) if total else None
        rows0 = rule["tables"][0][which]
        assert all([row[:3] for row in rule["tables"][r][which]] == [row[:3] for row in rows0] for r in range(world))      # same spans everywhere
        by_off = {off: (name, shape) for name, (off, shape) in layout.entries.items()}
        for g_off, s_off, n, _ in rows0:
            name, shape = by_off[g_off]
            for r in range(world):
                out[r][name] = mean[s_off:s_off + n].reshape(shape)
    return out
