"""Data parallelism for the engine: bucketed gradient all-reduce on RCCL over xGMI, overlapped
with the rest of backward.

Replaces what `accelerator.prepare(model)` becomes under a multi-process launch in the reference
(torch DDP, train_multi_modal.py:177,195).  Semantics kept: every rank runs its own batch through
a full replica and the gradient applied is the MEAN over ranks of the per-rank gradients of the
per-rank-normalised losses (mm.py:237) — not the gradient of a globally normalised loss.  One
process per GPU; the only collective on the path is this all-reduce (9.4 M fp32 values = 37.6 MB).

MI355X specifics: the flat gradient buffer is laid out in forward order, so backward completes it
back to front and each bucket is ONE contiguous range -> one large collective per bucket, no
gather/scatter copies.  xGMI is point-to-point (7 links/GPU): a few multi-MB buckets keep every
link busy while backward continues; the last bucket (the tokenisers) cannot overlap.  RCCL runs
the collective on its own stream; `work.wait()` only makes the compute stream wait, not the host.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import List, Optional

import torch
import torch.distributed as dist


def backward_order(layout, cfg) -> List[str]:
    return (["head"] + [f"decoder.{i}" for i in reversed(range(cfg.n_dec))] + ["bridge"]
            + [f"encoder.{i}" for i in reversed(range(cfg.n_enc))] + ["embed"])


class GradBuckets:
    """Contiguous ranges of the flat gradient buffer, in the order backward completes them."""

    def __init__(self, layout, cfg, bucket_bytes: int = 8 << 20):
        seg = {n: (s, e) for n, s, e in layout.segments}
        order = backward_order(layout, cfg)
        self.buckets = []          # (last_segment_name, start, end)
        cur_hi = cur_lo = None
        for name in order:
            s, e = seg[name]
            if cur_hi is None:
                cur_lo, cur_hi = s, e
            else:
                assert e == cur_lo or e <= cur_lo, "segments must be adjacent, descending"
                cur_lo = s
            if (cur_hi - cur_lo) * 4 >= bucket_bytes or name == order[-1]:
                self.buckets.append((name, cur_lo, cur_hi))
                cur_hi = cur_lo = None
        self.trigger = {name: (lo, hi) for name, lo, hi in self.buckets}


def trainable_spans(layout, buckets, trainable):
    """What each bucket all-reduces when only the parameters named in `trainable` take a gradient: {the bucket's trigger segment:
    (start, end) from its first to its last trainable parameter, or None where it has none (no collective)}.  A bucket all of whose
    parameters are trainable keeps its whole range, padding included: with everything trainable the ranges are the buckets'.
    buckets: GradBuckets.buckets.  A pure function of the layout and the names: no engine, no device."""
    trainable, out = set(trainable), {}
    for name, lo, hi in buckets:
        inside = [(off, off + int(math.prod(shape)), k in trainable) for k, (off, shape) in layout.entries.items() if lo <= off < hi]
        live = [(a, b) for a, b, on in inside if on]
        if len(live) == len(inside):
            out[name] = (lo, hi)
        else:
            out[name] = (min(a for a, _ in live), max(b for _, b in live)) if live else None
    return out


class EngineDDP:
    """Attach to an Engine: all-reduce each gradient bucket as soon as backward has produced it.

    With frozen parameters (requires_grad = False) a bucket all-reduces only the span from its first to its last trainable parameter,
    and a bucket without one issues no collective (`trainable_spans`; the engine's backward computes nothing there).  The spans follow
    the freeze pattern of the last forward.  EVERY RANK MUST FREEZE THE SAME PARAMETERS: ranks whose patterns differ would issue
    collectives of different sizes, or different numbers of them, and hang.

    Gradient accumulation: a backward under `no_sync()` issues no collective and leaves its gradient in G; the first backward outside
    the context (the caller skipped zero_grad(), so the engine adds into G) all-reduces the accumulated G bucket by bucket, as each
    segment's add completes.  Without `no_sync` an accumulating backward all-reduces every time, as torch DDP does.  EVERY RANK MUST
    CLOSE ITS GROUPS AT THE SAME BATCHES, for the same reason as above: a rank still inside `no_sync` issues no collective and the
    others would wait for it."""

    def __init__(self, engine, process_group=None, bucket_bytes: int = 8 << 20, broadcast: bool = True):
        if getattr(engine.cfg, "sessions", None):
            raise NotImplementedError("EngineDDP over a model with per-session layers (use_session) is not built: ranks hold different "
                                      "sessions, and whether a session is absent from a step is not a local fact")
        self.engine, self.pg = engine, process_group
        self.world = dist.get_world_size(process_group)
        self.buckets = GradBuckets(engine.layout, engine.cfg, bucket_bytes)
        self.works = []
        self.sync = True                    # False inside no_sync()
        self.collectives = 0                # all-reduces issued so far
        self._spans = {None: dict(self.buckets.trigger)}      # freeze pattern -> trainable_spans
        backend = dist.get_backend(process_group)
        self.avg_op = dist.ReduceOp.AVG if backend == "nccl" else None
        if broadcast:                       # replicas start identical (rank 0's parameters), like torch DDP
            dist.broadcast(engine.P, src=0, group=process_group)
            engine.refresh_weights()
        engine.grad_ready_hooks.append(self.on_segment)
        engine.backward_done_hooks.append(self.finish)

    @contextlib.contextmanager
    def no_sync(self):
        """Backwards inside the context issue no collective (torch DDP's no_sync): the gradient stays local until the first backward
        outside it."""
        old, self.sync = self.sync, False
        try:
            yield
        finally:
            self.sync = old

    def on_segment(self, name: str):
        if not self.sync or name not in self.buckets.trigger:
            return
        pattern = getattr(self.engine, "_pattern", None)      # the freeze pattern of the last forward (None: all trainable)
        if pattern not in self._spans:                        # a new freeze pattern: recomputed once, kept with the few others
            if len(self._spans) > 8:
                self._spans = {None: self._spans[None]}
            names = [k for k, on in zip(self.engine.layout.entries, pattern) if on]
            self._spans[pattern] = trainable_spans(self.engine.layout, self.buckets.buckets, names)
        rng = self._spans[pattern][name]
        if rng is None:
            return
        lo, hi = rng
        g = self.engine.G[lo:hi]
        self.collectives += 1
        if self.avg_op is not None:
            self.works.append((dist.all_reduce(g, op=self.avg_op, group=self.pg, async_op=True), None))
        else:
            self.works.append((dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.pg, async_op=True), g))

    def finish(self):
        for w, g in self.works:
            w.wait()
            if g is not None:
                g.mul_(1.0 / self.world)
        self.works = []


class DataParallelModel(torch.nn.Module):
    """What `Accelerator.prepare(model)` returns under a multi-process launch."""

    def __init__(self, module, process_group=None, bucket_bytes: int = 8 << 20):
        super().__init__()
        self.module = module
        self._pg, self._bucket_bytes, self._ddp = process_group, bucket_bytes, None
        self._no_sync = 0                    # depth of no_sync() contexts

    def forward(self, *a, **kw):
        eng = self.module.engine()           # builds / re-adopts the engine from the module's current parameters
        if self._ddp is None or self._ddp.engine is not eng:
            # like torch DDP's constructor: rank 0's parameters are broadcast BEFORE the first forward, so every replica's
            # first loss and gradient are taken at the same parameters even if the replicas were initialised differently
            self._ddp = EngineDDP(eng, self._pg, self._bucket_bytes, broadcast=True)
            self._ddp.sync = self._no_sync == 0          # built inside no_sync(): the group's first forward
        return self.module(*a, **kw)

    @contextlib.contextmanager
    def no_sync(self):
        """torch DDP's no_sync: backwards inside the context keep their gradient local (EngineDDP.no_sync).  Before the first
        forward there is no engine to tell yet, and nothing to hold back."""
        self._no_sync += 1
        if self._ddp is not None:
            self._ddp.sync = False
        try:
            yield
        finally:
            self._no_sync -= 1
            if self._ddp is not None:
                self._ddp.sync = self._no_sync == 0

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.module, name)


class Accelerator:
    """The slice of accelerate.Accelerator the reference uses: `.device` and `.prepare(model)`
    (train_multi_modal.py:177,195; trainer/base.py:55,60-61,257).  One process per GPU; rank and
    world size come from the torchrun environment."""

    def __init__(self, backend: Optional[str] = None):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if torch.cuda.is_available():
            torch.cuda.set_device(self.local_rank)
            self.device = torch.device("cuda", self.local_rank)
        else:
            self.device = torch.device("cpu")
        if self.world > 1 and not dist.is_initialized():
            dist.init_process_group(backend or ("nccl" if self.device.type == "cuda" else "gloo"))

    @property
    def is_main_process(self):
        return self.rank == 0

    def prepare(self, model):
        model = model.to(self.device)
        return DataParallelModel(model) if self.world > 1 else model
