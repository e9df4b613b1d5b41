"""Gradient accumulation without a GPU: the argument checks of mmfm_grad_accumulate (they return before anything is launched), the
group-size function the trainer and the entry script share, the trainer's validation of optimizer.gradient_accumulation_steps, and
EngineDDP.no_sync on a stand-in engine over gloo (two ranks): one set of bucket collectives per GROUP of backwards, and the mean over
ranks of the per-rank sums in G."""
import contextlib
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from helpers import build_model, load_config, tiny_config
from test_ddp_cpu import FakeEngine, _free_port

FAKE = 0x1000            # a non-NULL "device pointer": the checks return before anything dereferences or launches


@pytest.fixture(scope="module")
def lib():
    from multi_modal_foundation_model_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------- the kernel's argument checks
BAD_CALLS = {
    "NULL g": (dict(g=None), "NULL pointer"),
    "NULL stash": (dict(stash=None), "NULL pointer"),
    "start < 0": (dict(start=-1), "range"),
    "end > n": (dict(end=101), "range"),
    "start > end": (dict(start=11, end=10), "range"),
    "unknown mode": (dict(mode=2), "unknown mode"),
    "negative mode": (dict(mode=-1), "unknown mode"),
}


@pytest.mark.parametrize("case", list(BAD_CALLS))
def test_grad_accumulate_refuses_bad_arguments_before_launching(lib, case):
    kw, msg = BAD_CALLS[case]
    a = dict(dict(g=FAKE, stash=FAKE + 0x1000, n=100, start=3, end=50, mode=lib.GRAD_STASH), **kw)
    assert lib.lib().mmfm_grad_accumulate(a["g"], a["stash"], a["n"], a["start"], a["end"], a["mode"], None) == -1
    assert msg in lib.lib().mmfm_last_error().decode()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("at", [0, 7, 100])
def test_grad_accumulate_empty_range_is_no_launch(lib, mode, at):
    """start == end returns 0 before any HIP call: a machine without a GPU answers it, and nothing touches the (fake) pointers."""
    assert lib.lib().mmfm_grad_accumulate(FAKE, FAKE + 0x1000, 100, at, at, mode, None) == 0


def test_header_declares_the_feature_macro(lib):
    with open(lib.HEADER_PATH) as f:
        src = f.read()
    assert "#define MMFM_GRAD_ACCUM 1" in src and "#define MMFM_VERSION 401" in src
    assert f"#define MMFM_GRAD_STASH {lib.GRAD_STASH}" in src and f"#define MMFM_GRAD_ADD {lib.GRAD_ADD}" in src
    assert "mmfm_grad_accumulate" in lib.header_symbols()


# ------------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("n_batches, k, want", [(8, 3, [3, 3, 2]), (8, 4, [4, 4]), (8, 1, [1] * 8), (2, 5, [2]), (0, 3, [])])
def test_accumulation_groups(n_batches, k, want):
    from trainer.base import accumulation_groups
    sizes = accumulation_groups(n_batches, k)
    assert sizes == want
    assert sum(sizes) == n_batches and all(1 <= r <= k for r in sizes)
    assert accumulation_groups(n_batches, 1) == [1] * n_batches
    # every group but the epoch's last is full
    assert all(r == k for r in sizes[:-1])


@pytest.mark.parametrize("k", [0, -2, 1.5, 2.0, True, "3", None])
def test_accumulation_groups_refuses_what_is_no_positive_int(k):
    from trainer.base import accumulation_groups
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        accumulation_groups(8, k)


def _trainer(k):
    from trainer.make import make_multimodal_trainer

    class Acc:
        device = torch.device("cpu")
    cfg = load_config()
    cfg["optimizer"]["gradient_accumulation_steps"] = k
    return make_multimodal_trainer(model=build_model(tiny_config(), 12, 2, seed=1), train_dataloader=[], eval_dataloader=[], optimizer=None,
                                   log_dir="/tmp", accelerator=Acc(), lr_scheduler=None, avail_mod=["ap", "behavior"], config=cfg,
                                   modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=True,
                                   num_neurons=[12])


@pytest.mark.parametrize("k", [0, 1.5])
def test_trainer_refuses_bad_accumulation_steps(k):
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        _trainer(k)


def test_trainer_reads_accumulation_steps():
    assert load_config().optimizer.gradient_accumulation_steps == 1           # the shipped YAML: a step per batch
    assert _trainer(1).accum_steps == 1 and _trainer(3).accum_steps == 3


class StubModel(torch.nn.Module):
    """A model the epoch loop can drive without a GPU: one weight vector, `no_sync` recorded like a data-parallel wrapper's."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.arange(1.0, 5.0))
        self.held = []                     # per backward: was it inside no_sync()?
        self._inside = False

    @contextlib.contextmanager
    def no_sync(self):
        self._inside = True
        try:
            yield
        finally:
            self._inside = False

    def loss_of(self, x):
        loss = (self.w * x).pow(2).sum()
        loss.register_hook(lambda g: self.held.append(self._inside))
        return types.SimpleNamespace(loss=loss)


def _stub_run(k, epochs=2, n_batches=8):
    from torch.optim.lr_scheduler import OneCycleLR
    from trainer.base import accumulation_groups
    tr = _trainer(k)
    model = tr.model = StubModel()
    tr.train_dataloader = [torch.randn(4, generator=torch.Generator().manual_seed(i)) for i in range(n_batches)]
    tr.optimizer = torch.optim.AdamW(model.parameters(), lr=1e-2)
    total = epochs * len(accumulation_groups(n_batches, k))
    tr.lr_scheduler = OneCycleLR(tr.optimizer, total_steps=total, max_lr=1e-2)
    tr._forward_model_outputs = lambda batch, masking_mode, training_mode: model.loss_of(batch)
    tr._report_backward = lambda: setattr(tr, "_backward_reported", True)
    losses = [tr.train_epoch(e)["train_loss"] for e in range(epochs)]
    return tr, model, losses, total


@pytest.mark.parametrize("k", [1, 3, 4, 5])
def test_train_epoch_groups_on_a_stub_model(k):
    """k consecutive batches per optimiser step, the epoch's last group closing short; the mean gradient of the group is applied; all but
    a group's last backward run under no_sync; the scheduler ends exactly on the last optimiser step; train_loss is the unscaled sum."""
    from torch.optim.lr_scheduler import OneCycleLR
    from trainer.base import accumulation_groups
    tr, model, losses, total = _stub_run(k)
    sizes = accumulation_groups(8, k)
    assert tr.lr_scheduler.last_epoch == total == 2 * len(sizes)
    assert model.held == [i < r - 1 for r in sizes for i in range(r)] * 2
    ref = StubModel()
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-2)
    sch = OneCycleLR(opt, total_steps=total, max_lr=1e-2)
    want = []
    for _ in range(2):
        it, ep = iter(tr.train_dataloader), []
        for r in sizes:
            for _ in range(r):
                loss = ref.loss_of(next(it)).loss
                (loss / r).backward() if r > 1 else loss.backward()
                ep.append(loss.detach())
            opt.step(); sch.step(); opt.zero_grad()
        want.append(float(sum(x.item() for x in torch.stack(ep).double())))
    assert losses == want and torch.equal(model.w, ref.w)


# ------------------------------------------------------------------------------------------------- no_sync over gloo
GROUPS, MICRO = 2, 2


class AccumulatingFakeEngine(FakeEngine):
    """FakeEngine whose backward keeps the engine's accumulation rule: with `accumulate` the new gradient is added to what G holds,
    segment by segment, before that segment's hooks fire."""

    def run_backward(self, grads_by_name, accumulate=False):
        if accumulate:
            grads_by_name = {k: self.layout.view(self.G, k) + g for k, g in grads_by_name.items()}
        super().run_backward(grads_by_name)


def _micro_grads(lay, rank, index):
    g = torch.Generator().manual_seed(1000 * rank + index)
    return {k: torch.randn(shape, generator=g) for k, (_, shape) in lay.entries.items()}


def _layout():
    from multi_modal_foundation_model_amd.engine import EngineConfig, ParamLayout
    ec = EngineConfig.from_model_config(tiny_config(n_enc=2, n_dec=2), [("ap", 12), ("behavior", 2)])
    return ParamLayout(ec), ec


def _no_sync_worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "multi_modal_foundation_model_amd", "src"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from multi_modal_foundation_model_amd.ddp import EngineDDP
    lay, ec = _layout()
    eng = AccumulatingFakeEngine(lay, ec)
    ddp = EngineDDP(eng, bucket_bytes=16 << 10)          # small buckets -> several collectives
    issued, real = [], dist.all_reduce

    def counting(*a, **kw):
        issued.append(1)
        return real(*a, **kw)
    dist.all_reduce = counting
    per_group, G = [], []
    for grp in range(GROUPS):
        before = len(issued)
        for i in range(MICRO):
            grads = _micro_grads(lay, rank, grp * MICRO + i)
            if i < MICRO - 1:
                with ddp.no_sync():
                    eng.run_backward(grads, accumulate=i > 0)
                assert ddp.works == [] and len(issued) == before          # no collective, nothing for finish to wait for
            else:
                eng.run_backward(grads, accumulate=i > 0)
        assert ddp.sync and ddp.works == []
        per_group.append(len(issued) - before)
        G.append(eng.G.clone().numpy())
    assert ddp.collectives == len(issued)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), G=np.stack(G), per_group=np.asarray(per_group), buckets=len(ddp.buckets.buckets))
    dist.barrier()
    dist.destroy_process_group()


def test_no_sync_one_set_of_collectives_per_group_gloo(tmp_path):
    world = 2
    mp.spawn(_no_sync_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [np.load(tmp_path / f"rank{i}.npz") for i in range(world)]
    buckets = int(r[0]["buckets"])
    assert buckets >= 3
    for x in r:
        assert x["per_group"].tolist() == [buckets] * GROUPS                 # per group, not per backward
    np.testing.assert_array_equal(r[0]["G"], r[1]["G"])
    lay, _ = _layout()
    for grp in range(GROUPS):
        sums = []
        for rank in range(world):
            micro = [_micro_grads(lay, rank, grp * MICRO + i) for i in range(MICRO)]
            sums.append({k: micro[0][k] + micro[1][k] for k in micro[0]})
        G = torch.from_numpy(r[0]["G"][grp])
        for k in lay.entries:
            want = (sums[0][k] + sums[1][k]) * (1.0 / world)                  # gloo: SUM over ranks, then the 1 / world scale
            assert torch.equal(lay.view(G, k), want), (grp, k)
