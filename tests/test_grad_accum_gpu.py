"""Gradient accumulation on the GPU: mmfm_grad_accumulate bit for bit, the engine's stash / add around its backward (torch's rule per
parameter, no clone), the reference's accumulation curve (tests/golden/grad_accum_curve.json, scripts/make_grad_accum_goldens.py),
the trainer's groups against a hand loop, resume at k = 3, two ranks under no_sync and the entry script."""
import functools
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT, load_json
from helpers import build_model, load_config, make_optimizer, model_config, tiny_config
from model_checks import to_dev
from oracle import mm_oracle as O
from test_ddp_gpu import _free_port, _paths

pytestmark = pytest.mark.gpu
B, T, N_AP, N_BEH = 2, 8, 12, 2
OBJ = ("encoding", "decoding", "token_masking")


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------- the kernel
N = 2 * 4096 + 37
SPECIAL = [float("inf"), float("-inf"), 1e-40, -3e-42, 1.4e-45, 0.0, -0.0, 3.4e38, -3.4e38]


def kernel_inputs(goff, soff):
    """(g, stash) as views at element offsets goff / soff of two larger buffers (offset 0: 16-byte aligned), random fp32 with inf, NaN
    and denormal entries; no element is NaN in both (a NaN + NaN's payload is the one thing that may depend on operand order)."""
    gen = torch.Generator().manual_seed(5)
    vals = [torch.randn(N, generator=gen) for _ in range(2)]          # the views' contents do not depend on the offsets
    where = torch.randperm(N, generator=gen)
    full = [torch.randn(N + 8, generator=gen) for _ in range(2)]
    for j, (buf, off) in enumerate(zip(full, (goff, soff))):
        buf[off: off + N] = vals[j]
        spots = where[40 * j: 40 * (j + 1)]
        buf[off + spots[:len(SPECIAL)]] = torch.tensor(SPECIAL)
        buf[off + spots[len(SPECIAL): len(SPECIAL) + 4]] = float("nan")
    # inf + -inf and two denormals meeting, inside the range
    full[0][goff + 100], full[1][soff + 100] = float("inf"), float("-inf")
    full[0][goff + 101], full[1][soff + 101] = 1e-40, 2e-40
    full = [f.cuda() for f in full]
    return full, full[0][goff: goff + N], full[1][soff: soff + N]


# (g offset, stash offset, start, end): aligned buffers with a range off alignment at both ends; the same with the 16-byte grid of the
# buffers shifted; buffers that disagree modulo 16 bytes (element path throughout); aligned ends; ranges shorter than one quad
KERNEL_CASES = [(0, 0, 3, N - 2), (1, 1, 3, N - 2), (3, 3, 2, N - 1), (1, 2, 3, N - 2), (0, 0, 0, N), (0, 0, 4096, 8192), (0, 0, 5, 7),
                (0, 0, 3, 4), (2, 2, 1, 6)]


@pytest.mark.parametrize("goff, soff, start, end", KERNEL_CASES)
def test_grad_accumulate_kernel_bit_for_bit(goff, soff, start, end):
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    full, g, s = kernel_inputs(goff, soff)
    full0 = [f.clone() for f in full]
    g0, s0 = g.clone(), s.clone()
    inside = torch.zeros(N, dtype=torch.bool, device="cuda")
    inside[start:end] = True
    # stash: stash = g inside, every byte of both buffers kept outside
    K.grad_accumulate(g, s, start, end, L.GRAD_STASH)
    assert torch.equal(bits(s)[inside], bits(g0)[inside])
    assert torch.equal(bits(s)[~inside], bits(s0)[~inside]) and torch.equal(bits(full[0]), bits(full0[0]))
    assert torch.equal(bits(full[1])[:soff], bits(full0[1])[:soff]) and torch.equal(bits(full[1])[soff + N:], bits(full0[1])[soff + N:])
    # add: g = g + stash inside (torch.add of the two inputs), g untouched outside, stash kept
    s.copy_(s0)
    K.grad_accumulate(g, s, start, end, L.GRAD_ADD)
    want = torch.add(g0, s0)
    assert torch.equal(bits(g)[inside], bits(want)[inside])
    assert torch.equal(bits(g)[~inside], bits(g0)[~inside]) and torch.equal(bits(full[1]), bits(full0[1]))
    assert torch.equal(bits(full[0])[:goff], bits(full0[0])[:goff]) and torch.equal(bits(full[0])[goff + N:], bits(full0[0])[goff + N:])
    if start <= 100 and 102 <= end:
        assert torch.isnan(g[100]) and float(g[101]) == pytest.approx(3e-40, rel=1e-3)      # inf - inf; denormals are not flushed


def test_grad_accumulate_kernel_result_does_not_depend_on_alignment():
    """The range of the issue (start 3, end n - 2) through the 16-byte path and through the element path: the same bits."""
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    out = []
    for goff, soff in ((0, 0), (1, 1), (1, 2)):
        _, g, s = kernel_inputs(goff, soff)
        K.grad_accumulate(g, s, 3, N - 2, L.GRAD_ADD)
        out.append(bits(g).clone())
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])


@pytest.mark.parametrize("mode", [0, 1])
def test_grad_accumulate_kernel_empty_range(mode):
    """start == end is answered before any HIP call (tests/test_grad_accum_cpu.py: without a GPU it returns 0); here: nothing changes."""
    from multi_modal_foundation_model_amd import ops as K
    full, g, s = kernel_inputs(0, 0)
    full0 = [f.clone() for f in full]
    for at in (0, 5, N):
        K.grad_accumulate(g, s, at, at, mode)
    torch.cuda.synchronize()
    assert torch.equal(bits(full[0]), bits(full0[0])) and torch.equal(bits(full[1]), bits(full0[1]))


# ------------------------------------------------------------------------------------------------- the engine
FREEZE = ["encoder.0.attn.*", "decoder.1.mlp.up_proj.bias", "encoder_embeddings.ap.embedder.projection.*", "decoder_norm.*"]


def micro(model, i):
    """Micro-batch i: its own data, objective and mask stream."""
    torch.manual_seed(100 + i)
    return model(to_dev(O.make_mod_dict(O.synth_batch(B, T, N_AP, N_BEH, seed=i), OBJ[i % 3])))


def tiny_model(dtype="fp32", freeze=False):
    from multi_modal_foundation_model_amd.optim import freeze_parameters
    model = build_model(tiny_config(n_enc=2, n_dec=2), N_AP, N_BEH, seed=7)
    model.compute_dtype = dtype
    model.cuda().train()
    if freeze:
        assert freeze_parameters(model, FREEZE)
    return model


def singles(model, n=3):
    """Each micro-batch's gradient on its own, zero_grad() in between."""
    out = []
    for i in range(n):
        model.zero_grad(set_to_none=True)
        micro(model, i).loss.backward()
        out.append(model._engine.G.clone())
    model.zero_grad(set_to_none=True)
    return out


@pytest.mark.parametrize("freeze", [False, True], ids=["all", "frozen"])
@pytest.mark.parametrize("graph", ["0", "1"], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_three_micro_batches_sum_bit_for_bit(monkeypatch, dtype, graph, freeze):
    monkeypatch.setenv("MMFM_GRAPH", graph)
    model = tiny_model(dtype, freeze)
    g1, g2, g3 = singles(model)
    eng = model._engine
    assert eng._stash is None                                   # a run that never accumulates pays nothing
    for i in range(3):
        micro(model, i).loss.backward()
    assert (set(eng._last["graphs"]) == {"fwd", "bwd"}) == (graph == "1")
    want = (g1 + g2) + g3
    assert float(want.abs().max()) > 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            assert freeze and p.grad is None, name
            continue
        assert p.grad.data_ptr() == eng.Gv(name).data_ptr()
        assert torch.equal(bits(p.grad), bits(eng.layout.view(want, name))), name
    if not freeze:
        assert torch.equal(bits(eng.G), bits(want))           # padding included
    assert any(not p.requires_grad for p in model.parameters()) == freeze


def test_per_segment_adds_complete_before_each_hook(monkeypatch):
    """With grad_ready_hooks (data parallelism) an accumulating backward keeps the per-segment graphs and their tags; each segment's add
    has been issued when its hook fires: what the hook reads of the segment on the stream is the final sum.  The plan's lists are what
    they were before the first accumulating backward."""
    monkeypatch.setenv("MMFM_GRAPH", "1")
    model = tiny_model()
    eng = model.engine()
    seen = {}
    hook = lambda name: seen.__setitem__(name, eng.G[slice(*eng.segment_range(name))].clone())
    eng.grad_ready_hooks.append(hook)
    g1, g2, g3 = singles(model)
    plan = eng._last
    shape = (len(plan["fwd"]), [(n, len(seg)) for n, seg in plan["bwd"]])
    for i in range(3):
        seen.clear()
        micro(model, i).loss.backward()
    assert eng._last is plan and shape == (len(plan["fwd"]), [(n, len(seg)) for n, seg in plan["bwd"]])
    assert set(plan["graphs"]) == {"fwd"} | {"bwd/" + n for n, seg in plan["bwd"] if seg}
    want = (g1 + g2) + g3
    assert list(seen) == [n for n, _ in plan["bwd"]]
    for name, got in seen.items():
        lo, hi = eng.segment_range(name)
        assert torch.equal(bits(got), bits(want[lo:hi])), name
    assert torch.equal(bits(eng.G), bits(want))


def test_grad_none_parameter_takes_the_last_gradient_alone():
    model = tiny_model()
    g1, g2 = singles(model, 2)
    eng = model._engine
    named = dict(model.named_parameters())
    names = list(eng.layout.entries)
    alone = names[len(names) // 2]
    micro(model, 0).loss.backward()
    named[alone].grad = None
    micro(model, 1).loss.backward()
    both = g1 + g2
    for name, p in named.items():
        want = g2 if name == alone else both
        assert torch.equal(bits(p.grad), bits(eng.layout.view(want, name))), name
    named[alone].grad = None                             # the runs the next backward would accumulate: split around it
    runs = eng.accumulating_runs()
    off, shape = eng.layout.entries[alone]
    assert len(runs) == 2 and runs[0][1] <= off and runs[1][0] >= off + int(np.prod(shape, dtype=np.int64))


def test_in_place_zero_between_micro_batches():
    """The add reads the CURRENT G: after p.grad.zero_() on every parameter the next backward leaves exactly its own gradient."""
    model = tiny_model()
    g1, g2 = singles(model, 2)
    micro(model, 0).loss.backward()
    for p in model.parameters():
        p.grad.zero_()
    micro(model, 1).loss.backward()
    for name, p in model.named_parameters():
        assert torch.equal(p.grad, model._engine.layout.view(g2, name)), name


def test_accumulating_backward_allocates_no_copy_of_the_gradient_buffer():
    """Default widths (hidden 256, 5 + 5 layers, 668 + 2 channels: 9.41 M gradient elements), B = 2, T = 8.  From the second accumulating
    backward on the stash exists: the peak of a further one stays below one more G."""
    model = build_model(model_config(), 668, 2, seed=7).cuda().train()
    micro_big = lambda i: model(to_dev(O.make_mod_dict(O.synth_batch(B, T, 668, 2, seed=i), "encoding")))
    for i in range(3):                                   # one ordinary backward, then two accumulating ones
        micro_big(i).loss.backward()
    eng = model._engine
    assert eng._stash is not None and eng._stash.numel() == eng.G.numel() > 9_000_000
    out = micro_big(3)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out.loss.backward()                                  # the third accumulating backward
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("peak - before", peak - before, "G bytes", eng.G.numel() * 4)
    assert peak < before + eng.G.numel() * 4


# ------------------------------------------------------------------------------------------------- the reference's curve
def loop(model, opt, sch, sizes, epochs, seed_base, objectives, on_first_group=None):
    """The standard accumulation loop of the fixture: per batch of a group of r `(loss / r).backward()`, per group step / step /
    zero_grad.  Returns the batch losses and (lr, beta1) at every optimiser step."""
    losses, lr, beta1, index = [], [], [], 0
    for _ in range(epochs):
        for r in sizes:
            for _ in range(r):
                out = model(to_dev(O.make_mod_dict(O.synth_batch(B, T, N_AP, N_BEH, seed=seed_base + index), objectives[index])))
                (out.loss / r).backward() if r > 1 else out.loss.backward()
                losses.append(out.loss.detach())
                index += 1
            if on_first_group is not None and not lr:
                on_first_group()
            lr.append(opt.param_groups[0]["lr"])
            beta1.append(opt.param_groups[0]["betas"][0])
            opt.step()
            sch.step()
            opt.zero_grad()
    return [x.item() for x in losses], lr, beta1


@pytest.mark.parametrize("k", [3, 4])
def test_accumulation_curve_vs_reference_fixture(k):
    g = load_json("grad_accum_curve.json")[f"k{k}"]
    assert (g["B"], g["T"], g["n_ap"], g["n_beh"]) == (B, T, N_AP, N_BEH) and g["k"] == k
    from trainer.base import accumulation_groups
    sizes = accumulation_groups(g["batches_per_epoch"], k)
    assert sizes == g["group_sizes"] and g["total_steps"] == g["epochs"] * len(sizes)
    model = build_model(tiny_config(), N_AP, N_BEH, seed=g["model_seed"]).cuda().train()
    named = dict(model.named_parameters())
    assert list(named) == g["params"]
    opt, sch = make_optimizer(model, g["total_steps"])
    torch.manual_seed(1234)
    first = {}
    losses, lr, beta1 = loop(model, opt, sch, sizes, g["epochs"], g["seed_base"], g["objective"],
                             on_first_group=lambda: first.update({n: float(p.grad.double().norm()) for n, p in named.items()}))
    print("loss", losses[:3], "...", losses[-1], "reference", g["loss"][:3], "...", g["loss"][-1])
    assert len(lr) == g["total_steps"] == sch.last_epoch
    assert lr == g["lr"] and beta1 == g["beta1"]
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)
    for n, ref in zip(g["params"], g["first_group_grad_norm"]):
        assert first[n] == pytest.approx(ref, rel=5e-3, abs=1e-8), n
    final = [float(p.detach().double().norm()) for p in named.values()]
    np.testing.assert_allclose(final, g["final_param_norm"], rtol=1e-4)


# ------------------------------------------------------------------------------------------------- the trainer
N_BATCHES = 8


def loader_batches():
    out = []
    for i in range(N_BATCHES):
        b = O.synth_batch(B, T, N_AP, N_BEH, seed=i)
        b["eid"] = ["synthetic"] * B
        b["neuron_regions"] = [["XX"] * B for _ in range(N_AP)]
        out.append(b)
    return out


def make_trainer(k, total_steps, log_dir, model=None):
    from multi_modal_foundation_model_amd.ddp import Accelerator
    from trainer.make import make_multimodal_trainer
    if model is None:
        model = build_model(tiny_config(), N_AP, N_BEH, seed=7)
        model.engine_seed = 5
    acc = Accelerator()
    model = acc.prepare(model)
    opt, sch = make_optimizer(model, total_steps, lr=1e-3)
    cfg = load_config()
    cfg["training"]["exact_masker_stream"] = True
    cfg["optimizer"]["gradient_accumulation_steps"] = k
    tr = make_multimodal_trainer(model=model, train_dataloader=loader_batches(), eval_dataloader=[], optimizer=opt, log_dir=str(log_dir),
                                 accelerator=acc, lr_scheduler=sch, avail_mod=["ap", "behavior"], config=cfg,
                                 modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=True,
                                 num_neurons=[N_AP])
    return model, opt, sch, tr


@pytest.mark.parametrize("k", [3, 1])
def test_trainer_equals_the_hand_loop(tmp_path, k):
    """Two epochs of 8 batches.  k = 3: groups 3, 3, 2 - six optimiser steps, the scheduler ends on its last one (before: 16 steps, and
    OneCycleLR raised on the seventh).  k = 1: the bits of an explicit forward / backward / step / step / zero_grad loop."""
    from trainer.base import accumulation_groups
    epochs, sizes = 2, accumulation_groups(N_BATCHES, k)
    total = epochs * len(sizes)
    assert total == (6 if k == 3 else 16)
    model, opt, sch, tr = make_trainer(k, total, tmp_path)
    steps, real_step = [], opt.step
    opt.step = functools.wraps(real_step)(lambda *a, **kw: (steps.append(1), real_step(*a, **kw))[1])
    random.seed(42); torch.manual_seed(99)
    got = [tr.train_epoch(e)["train_loss"] for e in range(epochs)]
    assert len(steps) == total and sch.last_epoch == total
    # the hand loop: a second, identical model; the batch -> mod_dict translation and the objective sampling are the trainer's
    ref, opt2, sch2, tr2 = make_trainer(1, total, tmp_path)
    ref.train()
    random.seed(42); torch.manual_seed(99)
    want = []
    for _ in range(epochs):
        losses, it = [], iter(tr2.train_dataloader)
        for r in sizes:
            for _ in range(r):
                tr2._sample_modes()
                loss = tr2._forward_model_outputs(next(it), masking_mode=tr2.masking_mode, training_mode=tr2.training_mode).loss
                (loss / r).backward() if r > 1 else loss.backward()
                losses.append(loss.detach())
            opt2.step(); sch2.step(); opt2.zero_grad()
        want.append(float(sum(x.item() for x in torch.stack(losses).double().cpu())))
    assert got == want and all(np.isfinite(got))            # train_loss: the sum of the unscaled batch losses, bit for bit
    for (name, a), b in zip(model.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), name
    assert sch.state_dict()["last_epoch"] == sch2.state_dict()["last_epoch"] and opt.param_groups[0]["lr"] == opt2.param_groups[0]["lr"]


def test_resume_between_epochs_at_k3(tmp_path):
    """One epoch + save_model + a fresh trainer with load_train_state + one epoch == two epochs uninterrupted, bit for bit: an epoch
    boundary never holds a half-applied gradient, so the training state needs no field for one."""
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    m0, _, sch0, tr0 = make_trainer(3, 6, tmp_path / "a")
    random.seed(42); torch.manual_seed(99)
    tr0.train_epoch(0); tr0.train_epoch(1)
    want = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    m1, _, _, tr1 = make_trainer(3, 6, tmp_path / "b")
    random.seed(42); torch.manual_seed(99)
    tr1.train_epoch(0)
    tr1.save_model(name="last", epoch=0)
    del m1, tr1
    random.seed(0); torch.manual_seed(0)                                          # scramble every host stream
    ck = torch.load(tmp_path / "b" / "model_last.pt", weights_only=False)          # our own file (whole-module pickle)
    m2, _, sch2, tr2 = make_trainer(3, 6, tmp_path / "b", model=ck["model"])
    assert tr2.load_train_state(name="last") == 0 and sch2.last_epoch == 3
    tr2.train_epoch(1)
    assert sch2.last_epoch == sch0.last_epoch == 6
    for k, v in m2.state_dict().items():
        assert torch.equal(v, want[k]), k


# ------------------------------------------------------------------------------------------------- two ranks
WORLD, GROUPS, MICRO = 2, 3, 2


def _rank_batch(rank, index):
    md = O.make_mod_dict(O.synth_batch(4, T, N_AP, N_BEH, seed=100 * rank + index), OBJ[:2][index % 2])
    return to_dev(md)


def _ddp_model(seed):
    return build_model(tiny_config(n_enc=2, n_dec=2), N_AP, N_BEH, seed=seed).cuda().train()


def _worker(rank, port, out_dir):
    _paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD), LOCAL_RANK="0")
    import torch.distributed as dist
    from multi_modal_foundation_model_amd.ddp import DataParallelModel
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    model = _ddp_model(7 + rank)                                       # replicas differ until the broadcast
    ddp = DataParallelModel(model, bucket_bytes=16 << 10)
    opt, sch = make_optimizer(ddp, 10)
    per_group = []
    for grp in range(GROUPS):
        before = ddp._ddp.collectives if ddp._ddp is not None else 0
        with ddp.no_sync():
            (ddp(_rank_batch(rank, grp * MICRO)).loss / MICRO).backward()
        assert ddp._ddp.collectives == before and ddp._ddp.works == []
        (ddp(_rank_batch(rank, grp * MICRO + 1)).loss / MICRO).backward()
        per_group.append(ddp._ddp.collectives - before)
        opt.step(); sch.step(); opt.zero_grad()
    torch.save(dict(state={k: v.detach().cpu() for k, v in model.state_dict().items()}, per_group=per_group,
                    buckets=len(ddp._ddp.buckets.buckets)), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_no_sync_match_the_emulation(tmp_path):
    """Two ranks on the one GPU over gloo, groups of two micro-batches with the first under no_sync: replicas identical after three
    optimiser steps, equal to the single-process emulation (mean over ranks of the per-rank group means), one set of bucket collectives
    per group."""
    _paths()
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    r = [torch.load(os.path.join(tmp_path, f"rank{i}.pt"), weights_only=True) for i in range(WORLD)]
    for k in r[0]["state"]:
        assert torch.equal(r[0]["state"][k], r[1]["state"][k]), f"replicas diverged: {k}"
    assert r[0]["buckets"] >= 3
    assert r[0]["per_group"] == r[1]["per_group"] == [r[0]["buckets"]] * GROUPS
    model = _ddp_model(7)
    opt, sch = make_optimizer(model, 10)
    for grp in range(GROUPS):
        mean = None
        for rank in range(WORLD):
            opt.zero_grad()
            for i in range(MICRO):
                (model(_rank_batch(rank, grp * MICRO + i)).loss / MICRO).backward()
            g = model._engine.G.clone()
            mean = g if mean is None else mean + g
        model._engine.G.copy_(mean / WORLD)
        opt.step(); sch.step()
    opt.zero_grad()
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(v.detach().cpu().numpy(), r[0]["state"][k].numpy(), rtol=2e-5, atol=2e-7, err_msg=k)


# ------------------------------------------------------------------------------------------------- the entry script
def test_entry_script_with_grad_accum_steps(tmp_path):
    """`train_multi_modal.py --grad_accum_steps 3 --epochs 2` (8 batches per epoch: groups 3, 3, 2) runs to the end and writes its
    checkpoints; it used to die in OneCycleLR halfway through."""
    script = os.path.join(ROOT, "multi_modal_foundation_model_amd", "src", "train_multi_modal.py")
    cmd = [sys.executable, script, "--mixed_training", "--grad_accum_steps", "3", "--epochs", "2", "--n_neurons", "64", "--dtype", "bf16",
           "--base_path", str(tmp_path), "--overwrite"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    ckpts = glob.glob(os.path.join(str(tmp_path), "results", "**", "model_last.pt"), recursive=True)
    states = glob.glob(os.path.join(str(tmp_path), "results", "**", "train_state_last.pt"), recursive=True)
    assert len(ckpts) == 1 and len(states) == 1, (ckpts, states)
    state = torch.load(states[0], weights_only=False)                  # our own file
    assert state["lr_scheduler"]["last_epoch"] == state["lr_scheduler"]["total_steps"] == 6
