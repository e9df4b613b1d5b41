"""Data parallelism over per-session layers without a GPU.  The rule EngineDDP implements is torch DDP's with
find_unused_parameters=True, so the rule is checked against torch itself: two gloo ranks run DistributedDataParallel over the
plain-torch session layers of tests/session_stitch.py through the mixes of tests/session_ddp.py, and the pure functions of ddp.py
(`session_sync_rule`: the union, the span tables and `live`) must predict which .grad are None and, with the per-rank gradients of an
emulation that never talks to another rank, torch's gradients.  Beside it: the bucket cut, the refusal of mismatched session tables
on every rank, and the loader's rank -> session map."""
import os

import numpy as np
import pytest
import torch

import session_ddp as S
import session_stitch as R
from helpers import tiny_config
from multi_modal_foundation_model_amd.ddp import (GradBuckets, session_slots, session_span_rows, session_sync_rule, trainable_spans)
from multi_modal_foundation_model_amd.engine import EngineConfig, ParamLayout
from multi_modal_foundation_model_amd.synthetic import MultiSessionLoader

MODS = [("ap", S.P), ("behavior", 2)]


def session_cfg(sizes=S.SIZES, bias=True):
    mc = tiny_config(max_F=8)
    mc["use_session"] = True
    mc["stitcher"] = {"width": S.P, "bias": bias}
    return EngineConfig.from_model_config(mc, MODS, per_side=True, embedder_opts=True, sessions={"ap": tuple(sizes)}, stitch_bias=bias)


class Net(torch.nn.Module):
    """Read-in, a shared trunk, read-out: the session layers of tests/session_stitch.py around one dense layer."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.layers = R.RefLayers(S.SIZES, S.P)
        self.trunk = torch.nn.Linear(S.P, S.P)

    def forward(self, x, sid):
        Win, bin_ = self.layers.tensors("in")
        Wout, bout = self.layers.tensors("out")
        f = torch.tanh(self.trunk(R.read_in(x, sid, S.SIZES, Win, bin_)))
        return R.read_out(f, sid, S.SIZES, Wout, bout, S.N_MAX).pow(2).mean()


def shard(rank, step):
    g = torch.Generator().manual_seed(100 * rank + step)
    return torch.randn(S.B, S.T, S.N_MAX, generator=g)


def grads_of(net):
    return {k.replace("layers.", ""): (None if p.grad is None else p.grad.detach().clone().numpy()) for k, p in net.named_parameters()}


def _torch_worker(rank, port, out_dir):
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=S.WORLD)
    net = Net()
    ddp = DistributedDataParallel(net, find_unused_parameters=True)
    seen = []
    for i, step in enumerate(S.SCHEDULE):
        sid, sync, zero = step[rank], step[2], step[3]
        if zero:
            net.zero_grad(set_to_none=True)
        if sync:
            ddp(shard(rank, i), sid).backward()
        else:
            with ddp.no_sync():
                ddp(shard(rank, i), sid).backward()
        seen.append(grads_of(net))
    torch.save(seen, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_the_rule_predicts_torch_ddp_with_find_unused_parameters(tmp_path):
    S.run_ranks(_torch_worker, (S.free_port(), str(tmp_path)))
    seen = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(S.WORLD)]
    cfg = session_cfg()
    layout = ParamLayout(cfg)
    # the emulation: one replica per rank that never talks to the other; .grad follows torch's own rules on one process
    nets = [Net() for _ in range(S.WORLD)]
    checked = 0
    for group in S.groups():
        local = [set() for _ in range(S.WORLD)]
        for i in group:
            step = S.SCHEDULE[i]
            for r, net in enumerate(nets):
                if step[3]:
                    net.zero_grad(set_to_none=True)
                local[r] |= {("ap", k) for k in step[r]}
            if i == group[-1]:                           # which .grad are None when the closing backward starts
                grad_none = [{k for k, g in grads_of(net).items() if g is None and k.startswith("session_")} for net in nets]
            for r, net in enumerate(nets):
                net(shard(r, i), step[r]).backward()
            if i != group[-1]:                           # inside no_sync(): torch's gradients are the local ones
                for r in range(S.WORLD):
                    mine = grads_of(nets[r])
                    for k, g in seen[r][i].items():
                        assert (g is None) == (mine[k] is None), (i, r, k)
                        if g is not None:
                            np.testing.assert_allclose(g, mine[k], rtol=1e-6, atol=0)
        i = group[-1]
        rule = session_sync_rule(layout, cfg.sessions, local, grad_none)
        assert rule["union"] == set().union(*local)
        c = [grads_of(net) for net in nets]              # c_r: what rank r's .grad is at that moment on one process
        want = S.through_the_table(layout, rule, c)
        for r in range(S.WORLD):
            got = seen[r][i]
            assert set(rule["updated"]) | set(rule["kept"]) == {k for k in got if k.startswith("session_")}
            for k in rule["updated"]:                    # on every rank, whether or not it saw the session
                assert got[k] is not None, (i, r, k)
                np.testing.assert_allclose(got[k], want[r][k], rtol=1e-6, atol=1e-12, err_msg=f"{i} {r} {k}")
                checked += 1
            for k in rule["kept"]:                       # nobody's session: None stays None, a tensor keeps its bits
                assert (got[k] is None) == (c[r][k] is None), (i, r, k)
                if got[k] is not None:
                    assert np.array_equal(got[k], c[r][k]), (i, r, k)
            for k in ("trunk.weight", "trunk.bias"):
                np.testing.assert_allclose(got[k], 0.5 * (c[0][k] + c[1][k]), rtol=1e-6, atol=1e-12)
        for r, net in enumerate(nets):                   # the replicas go on from what the collective left
            for k, p in net.named_parameters():
                k = k.replace("layers.", "")
                if k in want[r]:
                    p.grad = torch.from_numpy(np.array(want[r][k]))
                elif not k.startswith("session_"):
                    p.grad = torch.from_numpy(0.5 * (c[0][k] + c[1][k]))
    assert checked > 40
    # the facts the mixes were chosen for
    assert all(seen[r][0][f"session_{w}.ap.2.weight"] is None for r in range(2) for w in ("in", "out"))       # step 0: session 2 is nowhere
    assert seen[0][0]["session_in.ap.1.weight"] is not None                                                      # rank 0 never saw session 1


def test_span_rows_order_padding_and_live():
    cfg = session_cfg()
    layout = ParamLayout(cfg)
    union = {("ap", 0), ("ap", 2)}
    rows, names, total = session_span_rows(layout, "out", union, lambda name: ".2." not in name)
    assert names == ["session_out.ap.0.weight", "session_out.ap.0.bias", "session_out.ap.2.weight", "session_out.ap.2.bias"]
    assert [r[2] for r in rows] == [12 * 8, 12, 9 * 8, 9] and [r[3] for r in rows] == [1, 1, 0, 0]
    assert [r[1] for r in rows] == [0, 96, 108, 180] and total == 192 and all(r[1] % 4 == 0 for r in rows)
    assert [r[0] for r in rows] == [layout.entries[k][0] for k in names] and all(r[0] % 8 == 0 for r in rows)
    # a frozen parameter has no row; the read-in block is the other tail
    rows, names, _ = session_span_rows(layout, "in", union, lambda name: True, trainable={k for k in layout.entries if not k.endswith(".bias")})
    assert names == ["session_in.ap.0.weight", "session_in.ap.2.weight"] and [r[1] for r in rows] == [0, 96]
    assert session_slots({"ap": (3, 2), "lfp": (5,)}) == {("ap", 0): 0, ("ap", 1): 1, ("lfp", 0): 2}
    assert session_span_rows(layout, "out", set(), lambda name: True) == ([], [], 0)


@pytest.mark.parametrize("bucket_bytes", [1 << 10, 16 << 10, 8 << 20])
def test_bucket_cut(bucket_bytes):
    # a layout without sessions: the same buckets and the same spans with the cut as without
    mc = tiny_config(max_F=8)
    plain = EngineConfig.from_model_config(mc, [("ap", 12), ("behavior", 2)], per_side=True, embedder_opts=True)
    lay = ParamLayout(plain)
    a, b = GradBuckets(lay, plain, bucket_bytes), GradBuckets(lay, plain, bucket_bytes, cut_sessions=True)
    assert a.buckets == b.buckets and a.trigger == b.trigger
    some = [k for k in lay.entries if "decoder" in k]
    assert trainable_spans(lay, a.buckets, some) == trainable_spans(lay, b.buckets, some)
    assert trainable_spans(lay, b.buckets, list(lay.entries)) == dict(a.trigger)
    # with sessions: no dense range holds a session entry, every other entry is in exactly one, embed is a bucket of its own
    cfg = session_cfg()
    lay = ParamLayout(cfg)
    cut = GradBuckets(lay, cfg, bucket_bytes, cut_sessions=True)
    for name, (off, shape) in lay.entries.items():
        n = sum(lo <= off and off + int(np.prod(shape)) <= hi for _, lo, hi in cut.buckets)
        assert n == (0 if name.startswith("session_") else 1), name
    seg = {n: (s, e) for n, s, e in lay.segments}
    assert cut.buckets[-1] == ("embed", seg["embed"][0], lay.entries["session_in.ap.0.weight"][0])
    assert cut.buckets[0][2] == lay.entries["session_out.ap.0.weight"][0]
    spans = trainable_spans(lay, cut.buckets, list(lay.entries))
    assert spans == dict(cut.trigger)
    # uncut, the dense ranges are today's (the refusal keeps anybody from using them over sessions)
    assert GradBuckets(lay, cfg, bucket_bytes).buckets[0][2] == seg["head"][1]


class _Fake:
    """What EngineDDP's constructor reads before it refuses."""
    def __init__(self, cfg):
        self.cfg, self.layout = cfg, ParamLayout(cfg)
        self.grad_ready_hooks, self.backward_done_hooks, self.forward_done_hooks = [], [], []


def _mismatch_worker(rank, port, out_dir, same):
    import torch.distributed as dist
    from multi_modal_foundation_model_amd.ddp import EngineDDP
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=S.WORLD)
    cfg = session_cfg(S.SIZES if rank == 0 or same else (12, 9, 7))
    try:
        EngineDDP(_Fake(cfg), broadcast=False, session_sync=True)
        msg = "built"
    except ValueError as e:
        msg = "ValueError: " + str(e)
    except Exception as e:                 # (beyond the check a CPU stand-in has no device for the staging buffers)
        msg = "other: " + type(e).__name__
    with open(os.path.join(out_dir, f"rank{rank}.txt"), "w") as f:
        f.write(msg)
    dist.barrier()
    dist.destroy_process_group()


def test_session_table_mismatch_raises_on_every_rank(tmp_path):
    S.run_ranks(_mismatch_worker, (S.free_port(), str(tmp_path), False))
    for r in range(S.WORLD):
        msg = open(os.path.join(tmp_path, f"rank{r}.txt")).read()
        assert msg.startswith("ValueError") and "session tables" in msg and "[1]" in msg, msg


def test_session_tables_that_agree_pass_the_check(tmp_path):
    S.run_ranks(_mismatch_worker, (S.free_port(), str(tmp_path), True))
    for r in range(S.WORLD):
        assert not open(os.path.join(tmp_path, f"rank{r}.txt")).read().startswith("ValueError")


def test_refusal_names_the_keyword():
    from multi_modal_foundation_model_amd.ddp import EngineDDP
    with pytest.raises(NotImplementedError, match="session_sync"):
        EngineDDP(_Fake(session_cfg()))


# ------------------------------------------------------------------------------------------------- the loader
def test_loader_world_1_is_todays_sequence():
    kw = dict(T=5, n_ap=320, n_beh=2, n_sessions=3, seed0=4)
    for rank in (0, 2):
        a, b = MultiSessionLoader(4, 2, rank=rank, **kw), MultiSessionLoader(4, 2, rank=rank, world=1, **kw)
        for i, (x, y) in enumerate(zip(a, b)):
            assert x["eid"] == y["eid"] == [f"session{i % 3}"] * 2
            assert all(torch.equal(x[k], y[k]) for k in x if isinstance(x[k], torch.Tensor))
            n = a.sizes[i % 3]
            assert bool((x["spikes_data"][:, :, n:] == -1).all()) and int(x["space_attn_mask"].sum()) == 2 * n


def test_loader_world_4_maps_rank_and_step_to_sessions():
    for r in range(4):
        ld = MultiSessionLoader(5, 2, T=5, n_ap=320, n_beh=2, n_sessions=3, rank=r, world=4)
        for i, b in enumerate(ld):
            k = (i * 4 + r) % 3
            assert b["eid"] == [f"session{k}"] * 2 and int(b["space_attn_mask"][0].sum()) == ld.sizes[k]
    with pytest.raises(ValueError):
        MultiSessionLoader(1, 2, n_sessions=3, rank=4, world=4)
