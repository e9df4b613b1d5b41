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

Per-session layers (use_session; `session_sync=True`): the session block is NOT part of the dense buckets.  Ranks hold
different sessions, so the sessions of a step are agreed by one MAX all-reduce of a presence vector, and only the spans of the sessions
some rank touched are packed (mmfm_span_gather), all-reduced in one collective per block (read-out, read-in) and copied back
(mmfm_span_scatter): torch DDP's rule with find_unused_parameters=True.
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
    """Contiguous ranges of the flat gradient buffer, in the order backward completes them.
    cut_sessions: the session layers (the tail of the `head` and of the `embed` segment, ParamLayout.session) leave the dense ranges:
    both segments end in front of their first session_* entry, and `embed` becomes a bucket of its own (the bucket it would have joined
    lies behind its session block, so the two are no longer adjacent).  A layout without session entries gives the same buckets either way."""

    def __init__(self, layout, cfg, bucket_bytes: int = 8 << 20, cut_sessions: bool = False):
        seg = {n: (s, e) for n, s, e in layout.segments}
        order = backward_order(layout, cfg)
        self.buckets = []          # (last_segment_name, start, end)
        cur_hi = cur_lo = prev = None
        for name in order:
            s, e = seg[name]
            first = min((off for k, (off, _) in layout.entries.items() if k.startswith("session_") and s <= off < e), default=None)
            if cut_sessions and first is not None:
                if cur_hi is not None and e != cur_lo:            # (never for `head`, the first segment of the order)
                    raise AssertionError("segments must be adjacent, descending")
                if cur_hi is not None:                            # close the open bucket in front of the session block
                    self.buckets.append((prev, cur_lo, cur_hi))
                    cur_hi = cur_lo = None
                e = first
            prev = name
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


def session_slots(sessions):
    """The presence vector's slots: {(modality, session index): position}, stitched modalities in the order of `sessions`
    (EngineConfig.sessions: modality -> neuron counts), sessions in index order.  Its length is the total number of sessions."""
    return {(mod, k): i for i, (mod, k) in enumerate((mod, k) for mod, sizes in sessions.items() for k in range(len(sizes)))}


def session_of(name):
    """(which, modality, session index) of a session parameter's name `session_{in,out}.{modality}.{k}.{weight,bias}`, else None."""
    if not name.startswith("session_"):
        return None
    head, rest = name.split(".", 1)
    mod, k, _ = rest.rsplit(".", 2)
    return head[len("session_"):], mod, int(k)


SPAN_PAD = 4         # packed spans start on multiples of 4 elements: with the layout's 32-byte slots both sides of every copy are 16-byte aligned


def session_span_rows(layout, which, union, live, trainable=None):
    """The span table of one session block (`which`: "out" - the read-out layers, tail of `head` - or "in", tail of `embed`) for the
    sessions in `union` (a set of (modality, session index)): rows (g_off, s_off, len, live) in layout order, which is (modality,
    session, weight, bias) order.  s_off is the running sum of the lengths, each rounded up to SPAN_PAD: the same on every rank, because
    it depends on the union and the layout alone.  live(name) -> bool says whether THIS rank's span holds a gradient (else it enters the
    sum as zeros and is never read); trainable: the names that take a gradient (None: all) - a frozen parameter has no row.
    Returns (rows, names, packed length).  A pure function: no engine, no device."""
    rows, names, s_off = [], [], 0
    for name, (off, shape) in layout.entries.items():
        ses = session_of(name)
        if ses is None or ses[0] != which or (ses[1], ses[2]) not in union or (trainable is not None and name not in trainable):
            continue
        n = int(math.prod(shape))
        rows.append((off, s_off, n, int(bool(live(name)))))
        names.append(name)
        s_off += (n + SPAN_PAD - 1) // SPAN_PAD * SPAN_PAD
    return rows, names, s_off


def session_sync_rule(layout, sessions, local, grad_none, trainable=None):
    """The rule of a synchronising backward over per-session layers, for all ranks at once (what EngineDDP does piecewise on each):
    local[r]: the sessions (modality, index) with a sample in any forward of rank r's group; grad_none[r]: the session parameters whose
    .grad is None on rank r when the closing backward starts.  Returns dict(union=U, tables={r: {"out": rows, "in": rows}},
    updated=the names that end with .grad = the mean over ranks on every rank, kept=the names whose .grad no rank touches).
    A span is live on rank r where the session is in local[r] (this group wrote or accumulated it) or its .grad is not None (an earlier
    group left a gradient there, as on one process); dead spans enter the mean as zeros."""
    slots = session_slots(sessions)
    union = set().union(*[set(l) for l in local]) & set(slots)
    tables, updated = {}, []
    for r, (loc, none) in enumerate(zip(local, grad_none)):
        live = lambda name, loc=set(loc), none=set(none): session_of(name)[1:] in loc or name not in none
        tables[r] = {w: session_span_rows(layout, w, union, live, trainable)[0] for w in ("out", "in")}
    for w in ("out", "in"):
        updated += session_span_rows(layout, w, union, lambda name: True, trainable)[1]
    kept = [k for k in layout.entries if session_of(k) is not None and session_of(k)[1:] not in union]
    return dict(union=union, tables=tables, updated=updated, kept=kept)


def session_table_digest(cfg):
    """32 bytes that differ where two ranks' session tables differ: the stitched modalities, their shared widths P, every session's
    neuron count and stitch_bias."""
    import hashlib
    widths = dict(cfg.mods)
    desc = repr([(mod, int(widths[mod]), tuple(int(n) for n in sizes)) for mod, sizes in cfg.sessions.items()] + [bool(cfg.stitch_bias)])
    return hashlib.sha256(desc.encode()).digest()


def check_session_tables(digest, process_group=None, device=None):
    """One all-gather of every rank's session_table_digest; ValueError on EVERY rank where they are not all the same."""
    mine = torch.tensor(list(digest), dtype=torch.uint8, device=device)
    got = [torch.empty_like(mine) for _ in range(dist.get_world_size(process_group))]
    dist.all_gather(got, mine, group=process_group)
    differ = [r for r, t in enumerate(got) if not torch.equal(t.cpu(), got[0].cpu())]
    if differ:
        raise ValueError(f"EngineDDP(session_sync=True): the session tables (modalities, sizes, stitch_bias, P) of ranks {differ} differ from "
                         "rank 0's: every rank must build the model over the same sessions in the same order")


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
    others would wait for it.

    Per-session layers (`session_sync=True`; without it a model with sessions is refused).  A group is the backwards since the last
    synchronising one; L is the set of sessions with a sample in any forward of this rank's group, U the union of L over the ranks.
    Every parameter of a session in U ends on every rank with .grad = the mean over ranks of what each rank's .grad would be on one
    process (zeros where it would be None) - also on a rank whose batches never held the session, which then updates it like the
    others.  A session outside U keeps its .grad (None stays None) and FusedAdamW skips it.  Per group ONE presence collective (int32
    MAX over one slot per session), issued asynchronously behind the forward of the synchronising step and read when `head` fires; then
    per block (read-out at `head`, read-in at `embed`) a gather of U's spans into a packed buffer, one all-reduce, and the scatter
    after its wait().  Nothing is issued inside no_sync(): L only accumulates.  DESIGN.md 3ab."""

    def __init__(self, engine, process_group=None, bucket_bytes: int = 8 << 20, broadcast: bool = True, session_sync: bool = False):
        sessions = getattr(engine.cfg, "sessions", None)
        if sessions and not session_sync:
            raise NotImplementedError("EngineDDP over a model with per-session layers (use_session) is not built: ranks hold different "
                                      "sessions, and whether a session is absent from a step is not a local fact - pass session_sync=True "
                                      "for the sparse session all-reduce")
        self.engine, self.pg = engine, process_group
        self.world = dist.get_world_size(process_group)
        self.sessions = dict(sessions) if sessions and session_sync else None
        self.buckets = GradBuckets(engine.layout, engine.cfg, bucket_bytes, cut_sessions=self.sessions is not None)
        self.works = []
        self.sync = True                    # False inside no_sync()
        self.collectives = 0                # gradient all-reduces issued so far (dense buckets and packed session blocks)
        self.session_collectives = 0        # ... the packed session blocks among them
        self.presence_collectives = 0       # presence all-reduces (one per group)
        self.last_union = None              # U of the last synchronising backward: a sorted list of (modality, session index)
        self._spans = {None: dict(self.buckets.trigger)}      # freeze pattern -> trainable_spans
        backend = dist.get_backend(process_group)
        self.avg_op = dist.ReduceOp.AVG if backend == "nccl" else None
        if self.sessions:
            dev = engine.device if backend == "nccl" else None            # collectives on the group's own backend
            check_session_tables(session_table_digest(engine.cfg), process_group, dev)
            self._slots = session_slots(self.sessions)
            self._local = set()             # L: the sessions of this rank's group so far
            self._presence = None           # (work, tensor) of the presence collective in flight
            self._presence_dev = dev
            self._block = {w: self._make_block(w) for w in ("out", "in")}
            engine.forward_done_hooks.append(self.on_forward)
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

    # ------------------------------------------------------------------ per-session layers
    def _make_block(self, which):
        """The static buffers of one session block, allocated once at the capacity of the whole block: the packed staging buffer, the
        device span table and its pinned host twin."""
        eng = self.engine
        rows, _, total = session_span_rows(eng.layout, which, set(self._slots), lambda name: True)
        cap = max(1, len(rows))
        pin = torch.cuda.is_available()
        return dict(stage=torch.zeros(max(total, SPAN_PAD), dtype=torch.float32, device=eng.device),
                    table=torch.zeros(cap, 4, dtype=torch.int64, device=eng.device),
                    host=torch.zeros(cap, 4, dtype=torch.int64, pin_memory=pin), uploaded=None, n=0)

    def _present(self):
        """The sessions of the engine's last forward (its local fact: `Engine._absent` names the parameters of the others)."""
        absent = self.engine._absent
        kind = "weight"
        return {(mod, k) for (mod, k) in self._slots if f"session_in.{mod}.{k}.{kind}" not in absent}

    def _issue_presence(self):
        v = torch.zeros(len(self._slots), dtype=torch.int32)
        for key in self._local:
            v[self._slots[key]] = 1
        if self._presence_dev is not None:
            v = v.to(self._presence_dev, non_blocking=True)
        self.presence_collectives += 1
        self._presence = (dist.all_reduce(v, op=dist.ReduceOp.MAX, group=self.pg, async_op=True), v)

    def on_forward(self):
        """Behind every forward that takes a gradient: L grows; outside no_sync() this is the group's closing step and the presence
        collective starts here, to be read as late as `head`."""
        self._local |= self._present()
        if not self.sync:
            return
        if self._presence is not None:      # a forward whose backward never ran: its collective is completed and dropped (on every rank)
            self._presence[0].wait()
        self._issue_presence()

    def _read_union(self):
        if self._presence is None:          # the forward ran inside no_sync(), its backward outside: agreed now
            self._local |= self._present()
            self._issue_presence()
        work, v = self._presence
        work.wait()
        self._presence = None
        got = v.cpu().tolist()              # (nccl: the one host wait of the step, as late as the first session span needs it)
        self.last_union = sorted(key for key, i in self._slots.items() if got[i])

    def _session_block(self, which):
        """Gather the spans of U's sessions of one block and all-reduce the packed buffer; finish() scatters it back."""
        from . import ops as K
        eng, blk = self.engine, self._block[which]
        pattern = getattr(eng, "_pattern", None)
        trainable = None if pattern is None else {k for k, on in zip(eng.layout.entries, pattern) if on}
        local = self._local
        has_grad = lambda name: name in eng.params and eng.params[name].grad is not None        # (read before this backward hands out)
        live = lambda name: session_of(name)[1:] in local or has_grad(name)
        rows, _, total = session_span_rows(eng.layout, which, set(self.last_union), live, trainable)
        blk["n"] = len(rows)
        if not rows:                        # every rank has the same U and the same freeze pattern: none of them issues anything
            return
        if blk["uploaded"] is not None:     # the pinned table is rewritten only behind its last upload
            blk["uploaded"].synchronize()
        K.span_table(rows, eng.G.numel(), blk["stage"].numel(), out=blk["host"])
        blk["table"].copy_(blk["host"], non_blocking=True)
        if blk["host"].is_pinned():
            blk["uploaded"] = torch.cuda.Event()
            blk["uploaded"].record()
        K.span_gather(eng.G, blk["stage"], blk["table"], len(rows))
        packed = blk["stage"][:total]
        self.collectives += 1
        self.session_collectives += 1
        after = lambda: K.span_scatter(blk["stage"], eng.G, blk["table"], len(rows))
        if self.avg_op is not None:
            self.works.append((dist.all_reduce(packed, op=self.avg_op, group=self.pg, async_op=True), None, after))
        else:
            self.works.append((dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=self.pg, async_op=True), packed, after))

    def on_segment(self, name: str):
        if not self.sync:
            return
        self._dense(name)
        if self.sessions and name in ("head", "embed"):       # the session blocks are the tails of these two segments
            if name == "head":
                self._read_union()
            self._session_block("out" if name == "head" else "in")

    def _dense(self, name: str):
        if name not in self.buckets.trigger:
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
            self.works.append((dist.all_reduce(g, op=self.avg_op, group=self.pg, async_op=True), None, None))
        else:
            self.works.append((dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.pg, async_op=True), g, None))

    def finish(self):
        for w, g, after in self.works:
            w.wait()
            if g is not None:
                g.mul_(1.0 / self.world)
            if after is not None:
                after()
        self.works = []
        if self.sessions and self.sync:
            # the group is closed: the engine hands out .grad for every session of U (also those this rank never saw) and leaves the
            # others' alone - `absent` now means absent on every rank.  The next forward sets the local fact again
            union = set(self.last_union)
            self.engine._absent = frozenset(k for k in self.engine.layout.entries if session_of(k) is not None and session_of(k)[1:] not in union)
            self._local = set()


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
            self._ddp = EngineDDP(eng, self._pg, self._bucket_bytes, broadcast=True, session_sync=bool(getattr(eng.cfg, "sessions", None)))
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
