"""Data parallelism over per-session layers with the REAL engine: two ranks (processes) on the one GPU, gloo, the fp32 tiny model -
the harness of tests/test_ddp_gpu.py, every worker under its own time limit and its exit status checked.  Sessions ap: (12, 7, 9),
P = 8, B = 4, T = 8, through the mixes of tests/session_ddp.py: ranks with disjoint sessions, the same session, a mixed batch, and one
accumulation group of two micro-batches (the first under no_sync()) entered without zero_grad().

After every backward both ranks' gradients must equal (c_0 + c_1) * 0.5, c_r = what rank r's .grad would be on one process (zeros
where None), from an emulation that runs the two shards through the same engine in this process.  The comparison is torch.equal for
the session spans AND for the dense spans: every kernel gives the same bits for the same inputs, a two-term fp32 sum is commutative
(the engine's accumulate is g + stash, gloo's sum is a + b) and the scaling by 0.5 is exact, so nothing on the way rounds differently.
The parameters after each optimiser step are compared the same way."""
import os
import random

import pytest
import torch

import session_ddp as S
from conftest import ROOT  # noqa: F401  (the workers import the package from the tree)

pytestmark = pytest.mark.gpu
N_BEH = 2
SESSIONS = {"s.12": 12, "s.7": 7, "s.9": 9}
EIDS = list(SESSIONS)
OBJECTIVES = ("encoding", "decoding", "token_masking", "encoding", "decoding")
SEED = 11


def make_model(seed):
    from helpers import build_model, tiny_config
    mc = tiny_config(max_F=8, n_enc=2, n_dec=2)
    mc["use_session"] = True
    mc["stitcher"] = {"width": S.P, "bias": True}
    return build_model(mc, S.N_MAX, N_BEH, seed=seed, sessions=SESSIONS).cuda().train()


def mod_dict(rank, i):
    from model_checks import to_dev
    from oracle import mm_oracle as O
    sid = S.SCHEDULE[i][rank]
    batch = O.synth_batch(S.B, S.T, S.N_MAX, N_BEH, seed=100 * rank + i)
    for b, k in enumerate(sid):
        batch["spikes_data"][b, :, S.SIZES[k]:] = -1.0
    md = O.make_mod_dict(batch, OBJECTIVES[i])
    md["ap"]["eid"] = [EIDS[k] for k in sid]
    return to_dev(md)


def run(model, rank, i):
    torch.manual_seed(SEED + i)
    random.seed(SEED + i)
    out = model(mod_dict(rank, i))
    out.loss.backward()
    return out


def grads_of(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def session_state(model, opt, k):
    """The bits session k's parameters, moments and step counts hold."""
    eng = model._engine
    names = [n for n in eng.layout.entries if n.startswith("session_") and n.split(".")[2] == str(k)]
    spans = [(eng.layout.entries[n][0], eng.layout.entries[n][0] + eng.layout.view(eng.P, n).numel()) for n in names]
    bufs = [t for t in (eng.P, opt._m, opt._v) if t is not None]
    steps = None if opt._steps is None else [opt._steps[n] for n in names]
    return [[t[a:b].clone().cpu() for a, b in spans] for t in bufs], steps, opt._t


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(S.WORLD), LOCAL_RANK="0")
    import torch.distributed as dist
    from helpers import make_optimizer
    from multi_modal_foundation_model_amd.ddp import DataParallelModel
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=S.WORLD)
    model = make_model(7 + rank)                                     # replicas differ until the broadcast
    ddp = DataParallelModel(model, bucket_bytes=16 << 10)
    opt, sch = make_optimizer(ddp, 10)
    rec = []
    for i, step in enumerate(S.SCHEDULE):
        sync, zero = step[2], step[3]
        if zero:
            opt.zero_grad()
        d = ddp._ddp
        before = (0, 0, 0) if d is None else (d.collectives, d.session_collectives, d.presence_collectives)
        if sync:
            run(ddp, rank, i)
        else:
            with ddp.no_sync():
                run(ddp, rank, i)
        d = ddp._ddp
        r = dict(grads={k: None if g is None else g.cpu() for k, g in grads_of(model).items()},
                 counts=tuple(a - b for a, b in zip((d.collectives, d.session_collectives, d.presence_collectives), before)),
                 union=d.last_union, dense=len([x for x in d._spans[None].values() if x is not None]))
        if sync:
            if i == 0:
                opt._bind()                                          # (the moment buffers exist from the first step on; made now to be compared)
                r["ses1_before"] = session_state(model, opt, 1)[0][0]
                r["ses2_before"] = session_state(model, opt, 2)
            opt.step()
            sch.step()
            if i == 0:
                r["ses1_after"] = session_state(model, opt, 1)[0][0]
                r["ses2_after"] = session_state(model, opt, 2)
                r["steps"] = None if opt._steps is None else dict(opt._steps)
            r["P"] = model._engine.P.detach().cpu().clone()
        rec.append(r)
    torch.save(rec, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) or torch.equal(a, b)       # (+0 == -0 is no difference)


def test_two_ranks_hold_the_mean_over_the_union_of_their_sessions(tmp_path):
    S.run_ranks(_worker, (S.free_port(), str(tmp_path)), limit=240.0)
    rec = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(S.WORLD)]
    from helpers import make_optimizer
    model = make_model(7)                                            # rank 0's initial parameters
    opt, sch = make_optimizer(model, 10)
    names = [k for k, _ in model.named_parameters()]
    ses = lambda k: int(k.split(".")[2]) if k.startswith("session_") else None
    state = [dict.fromkeys(names) for _ in range(S.WORLD)]           # per rank: what its .grad would be on one process
    for group in S.groups():
        local = [set() for _ in range(S.WORLD)]
        for i in group:
            step = S.SCHEDULE[i]
            for r in range(S.WORLD):
                if step[3]:
                    state[r] = dict.fromkeys(names)
                model.zero_grad(set_to_none=True)
                run(model, r, i)
                for k, g in grads_of(model).items():
                    if g is not None:
                        state[r][k] = g if state[r][k] is None else state[r][k] + g
                local[r] |= set(step[r])
            if i != group[-1]:                                       # inside no_sync(): local gradients, no collective of any kind
                for r in range(S.WORLD):
                    assert rec[r][i]["counts"] == (0, 0, 0)
                    for k in names:
                        got, want = rec[r][i]["grads"][k], state[r][k]
                        assert (got is None) == (want is None), (i, r, k)
                        assert got is None or same(got, want.cpu()), (i, r, k)
        i, union = group[-1], local[0] | local[1]
        zeros = lambda k: torch.zeros_like(dict(model.named_parameters())[k])
        mean = {}
        for k in names:
            if ses(k) is None or ses(k) in union:
                c = [state[r][k] if state[r][k] is not None else zeros(k) for r in range(S.WORLD)]
                mean[k] = (c[0] + c[1]) * 0.5
        worst = 0.0
        for r in range(S.WORLD):
            assert rec[r][i]["union"] == [("ap", k) for k in sorted(union)]
            # 2 packed session all-reduces beside the dense buckets', one presence collective for the whole group
            assert rec[r][i]["counts"] == (rec[r][i]["dense"] + 2, 2, 1) and rec[r][i]["dense"] >= 3, rec[r][i]["counts"]
            for k in names:
                got = rec[r][i]["grads"][k]
                if k in mean:
                    assert got is not None, (i, r, k)
                    worst = max(worst, float((got - mean[k].cpu()).abs().max()))
                    assert same(got, mean[k].cpu()), (i, r, k, float((got - mean[k].cpu()).abs().max()))
                else:                                                # nobody's session: .grad is what it was
                    assert (got is None) == (state[r][k] is None), (i, r, k)
                    assert got is None or same(got, state[r][k].cpu()), (i, r, k)
        print("step", i, "union", sorted(union), "largest gradient difference", worst)
        for r in range(S.WORLD):
            state[r].update(mean)
        eng = model._engine
        for k, p in model.named_parameters():                        # the emulation's optimiser step on the mean
            if state[0][k] is None:
                p.grad = None
            else:
                eng.Gv(k).copy_(state[0][k])
                p.grad = eng.Gv(k)
        opt.step()
        sch.step()
        assert same(rec[0][i]["P"], rec[1][i]["P"]), f"replicas diverged at step {i}"
        assert same(rec[0][i]["P"], eng.P.detach().cpu()), f"step {i}: the parameters differ from the emulation's"
    # step 0: session 2 was on no rank - .grad None, and the optimiser left its parameters, moments and step counts alone
    for r in range(S.WORLD):
        g0 = rec[r][0]["grads"]
        assert all(g0[k] is None for k in names if ses(k) == 2) and all(g0[k] is not None for k in names if ses(k) in (0, 1))
        (b_bufs, b_steps, b_t), (a_bufs, a_steps, a_t) = rec[r][0]["ses2_before"], rec[r][0]["ses2_after"]
        assert all(same(x, y) for xs, ys in zip(b_bufs, a_bufs) for x, y in zip(xs, ys))
        assert len(b_bufs) == len(a_bufs) == 3 and a_t == b_t + 1 and a_steps is not None and all(n == b_t for n in a_steps)
        steps = rec[r][0]["steps"]
        assert {k for k in steps if ses(k) == 2} == {k for k in names if ses(k) == 2}
        assert all(n == (b_t if ses(k) == 2 else a_t) for k, n in steps.items())
    # ... and session 1's parameters moved on rank 0, which never saw it
    assert not any(same(x, y) for x, y in zip(rec[0][0]["ses1_before"], rec[0][0]["ses1_after"]))
    assert same(rec[0][-1]["P"], rec[1][-1]["P"])


def _rccl_worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as dist
    from helpers import make_optimizer
    from multi_modal_foundation_model_amd.ddp import DataParallelModel
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    finals, counts = [], None
    for wrap in (True, False):
        model = make_model(7)
        m = DataParallelModel(model, bucket_bytes=16 << 10) if wrap else model
        opt, sch = make_optimizer(m, 10)
        for i, step in enumerate(S.SCHEDULE):
            if step[3]:
                opt.zero_grad()
            if wrap and not step[2]:
                with m.no_sync():
                    run(m, 0, i)
            else:
                run(m, 0, i)
            if step[2]:
                opt.step()
                sch.step()
        if wrap:
            d = m._ddp
            assert d.avg_op is not None and d._presence_dev is not None
            counts = (d.session_collectives, d.presence_collectives, d.last_union)
        finals.append(model._engine.P.detach().cpu().clone())
    torch.save(dict(finals=finals, counts=counts), os.path.join(out_dir, "rccl.pt"))
    dist.destroy_process_group()


def test_rccl_path_single_rank_equals_the_unwrapped_run(tmp_path):
    """RCCL needs one GPU per rank, so only a world of 1 can run it here: the collectives are identities then, but the calls are the
    8-GPU run's - the digest all-gather, the presence MAX on a device int32 tensor, the AVG all-reduce of the packed buffers between
    the backward segments, the scatter behind the wait.  With one rank U = L, so the result must be the unwrapped run's bits."""
    S.run_ranks(_rccl_worker, (S.free_port(), str(tmp_path)), world=1, limit=180.0)
    r = torch.load(os.path.join(tmp_path, "rccl.pt"), weights_only=False)
    assert same(r["finals"][0], r["finals"][1])
    groups = S.groups()
    assert r["counts"] == (2 * len(groups), len(groups), [("ap", 0), ("ap", 2)])


def _plain_worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as dist
    from helpers import build_model, tiny_config
    from model_checks import to_dev
    from multi_modal_foundation_model_amd import ddp as D
    from oracle import mm_oracle as O
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    model = build_model(tiny_config(n_enc=2, n_dec=2), S.N_MAX, N_BEH, seed=7).cuda().train()
    wrapped = D.DataParallelModel(model, bucket_bytes=16 << 10)
    calls, real, gathers = [], dist.all_reduce, []
    real_gather = dist.all_gather

    def spy(t, *a, **kw):
        G = model._engine.G
        calls.append(((t.data_ptr() - G.data_ptr()) // 4, (t.data_ptr() - G.data_ptr()) // 4 + t.numel()) if t.is_cuda else ("host", t.numel()))
        return real(t, *a, **kw)

    dist.all_reduce = spy
    dist.all_gather = lambda *a, **kw: (gathers.append(1), real_gather(*a, **kw))[1]
    for i in range(2):
        wrapped(to_dev(O.make_mod_dict(O.synth_batch(S.B, S.T, S.N_MAX, N_BEH, seed=i), "encoding"))).loss.backward()
        model.zero_grad(set_to_none=True)
    d, eng = wrapped._ddp, model._engine
    was = D.GradBuckets(eng.layout, eng.cfg, 16 << 10)               # the buckets as they were built before the session cut existed
    want = [was.trigger[n] for n in D.backward_order(eng.layout, eng.cfg) if n in was.trigger]
    torch.save(dict(calls=calls, want=want * 2, gathers=len(gathers), counts=(d.collectives, d.session_collectives, d.presence_collectives),
                    sessions=d.sessions), os.path.join(out_dir, "plain.pt"))
    dist.destroy_process_group()


def test_a_model_without_sessions_issues_the_collectives_it_always_issued(tmp_path):
    S.run_ranks(_plain_worker, (S.free_port(), str(tmp_path)), world=1, limit=120.0)
    r = torch.load(os.path.join(tmp_path, "plain.pt"), weights_only=False)
    assert r["sessions"] is None and r["gathers"] == 0
    assert [tuple(c) for c in r["calls"]] == [tuple(w) for w in r["want"]] and len(r["want"]) >= 6
    assert r["counts"] == (len(r["want"]), 0, 0)
