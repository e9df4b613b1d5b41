"""Fused AdamW over the engine's flat parameter buffer.

Drop-in for `torch.optim.AdamW(params, lr, betas, eps, weight_decay)` (reference: train_multi_modal.py:197-202, stepping at
trainer/base.py:196-198): same constructor arguments, same `param_groups` (so `OneCycleLR` keeps rewriting every group's `lr` and
`betas[0]`), same update rule as torch's single-tensor AdamW, same per-parameter step counts.  `zero_grad()` is O(1) per parameter: the
next backward overwrites the flat gradient buffer.

What it takes:
  * any number of param groups, each with its own lr / betas / eps / weight_decay;
  * any subset of the engine's parameters (a frozen trunk); a parameter whose .grad is None is skipped, as torch skips it;
  * max_grad_norm: the 2-norm of the gradients being updated is measured on the device (one sum-of-squares launch and its closing
    launch) and the update multiplies each gradient by clip_coef = min(1, max_norm / (norm + 1e-6)) - torch.nn.utils.clip_grad_norm_'s
    formula.  UNLIKE torch's function this never rewrites the gradients: the flat buffer and every p.grad keep the un-clipped values;
  * skip_nonfinite: a step whose gradient norm is inf or NaN changes nothing on the device.  The host cannot know without a
    synchronisation and step() has none, so the host's step counts advance all the same - UNLIKE torch.amp.GradScaler, which does not
    count a skipped step.  The next real update therefore takes the bias correction of one step later.

The default construction (one group, every parameter, no clipping, no skipping) issues exactly one mmfm_adamw_step per step; everything
else goes through the range table (mmfm_adamw_step_ranges).  last_grad_norm(), grad_norms() and skipped_steps() read the device record
and are the only calls that synchronise.
"""
from __future__ import annotations

import math

import torch

from . import ops as K


def adamw_hyper_row(lr, betas, eps, weight_decay, step, grad_scale=1.0):
    """The 8 floats of mmfm_adamw_step's hyper vector (include/mmfm.h), in double; step is 1-based."""
    b1, b2 = betas
    return (1.0 - lr * weight_decay, 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step), eps, grad_scale)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, engine=None, grad_scale=1.0,
                 max_grad_norm=None, skip_nonfinite=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        seen = set()
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) in seen:
                    raise ValueError("FusedAdamW: a parameter appears twice (within one group or in two groups)")
                seen.add(id(p))
        if max_grad_norm is not None and not (float(max_grad_norm) > 0 and math.isfinite(float(max_grad_norm))):
            max_grad_norm = None                 # torch: an infinite max_norm never clips; nothing to launch for it
        self.engine = engine
        self.grad_scale = grad_scale
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._t = 0                     # steps taken (those that updated at least one parameter)
        self._steps = None              # name -> updates taken by that parameter; None: every owned parameter is at _t
        self._m = self._v = self._hyper = None
        self._ring, self._ring_ev, self._ring_i = [], [], 0      # pinned staging slots for the per-step scalars
        self._bound = None              # (engine, its adoption count) the owned list below was built for
        self._owned = []                # (name, parameter, offset, numel, group index), in buffer order
        self._covers_all = False
        self._sig, self._tab, self._tab_names = None, None, []   # the range table of the current (parameter -> hyper row) map
        self._loaded_steps = None
        self._skips_before = 0          # skipped steps counted by tables of an engine this optimiser no longer steps
        self.pre_step_hooks = []        # e.g. the DDP wrapper's "wait for the all-reduce" hook

    def attach(self, engine):
        self.engine = engine
        return self

    def _bind(self):
        eng = self.engine
        if eng is None:
            raise RuntimeError("FusedAdamW needs the model's engine: call opt.attach(model.engine()) after the first forward, "
                               "or construct it through make_optimizer(model, ...)")
        if self._m is None or self._m.numel() != eng.P.numel() or self._m.device != eng.P.device:
            self._m, self._v = torch.zeros_like(eng.P), torch.zeros_like(eng.P)
            self._hyper = None          # allocated with its pinned staging ring at the first step (_upload_hyper)
        key = (eng, eng.adoptions)
        if self._bound is None or self._bound[0] is not key[0] or self._bound[1] != key[1]:
            names = {id(p): name for name, p in eng.params.items()}
            owned = []
            for gi, g in enumerate(self.param_groups):
                for p in g["params"]:
                    name = names.get(id(p))
                    if name is None:
                        raise RuntimeError("FusedAdamW owns a tensor that is not one of the engine's parameters (model.parameters())")
                    off, shape = eng.layout.entries[name]
                    owned.append((name, p, int(off), int(math.prod(shape)), gi))
            owned.sort(key=lambda o: o[2])
            self._owned, self._covers_all = owned, len(owned) == len(eng.params)
            self._bound, self._sig, self._tab = key, None, self._carry_skips(None)
            if self._loaded_steps is not None:
                self._steps, self._loaded_steps = self._named_steps(self._loaded_steps), None
        return eng

    def _alloc_hyper(self, rows, device):
        """Device hyper table [rows][8] and its pinned staging ring.  The host may run many steps ahead of the GPU: each async H2D copy
        of the scalars gets its own pinned slot, reused only after the copy that last read it has completed."""
        for ev in self._ring_ev:
            if ev is not None:
                ev.synchronize()
        self._hyper = torch.zeros(rows * 8, device=device)
        self._ring = [torch.zeros(rows * 8).pin_memory() for _ in range(16)]
        self._ring_ev = [None] * 16

    def _upload_hyper(self, rows):
        """rows: list of 8-tuples.  Returns the device table (async copy through the ring)."""
        if self._hyper is None or self._hyper.numel() != 8 * len(rows) or self._hyper.device != self._m.device:
            self._alloc_hyper(len(rows), self._m.device)
        i = self._ring_i = (self._ring_i + 1) % len(self._ring)
        if self._ring_ev[i] is not None:
            self._ring_ev[i].synchronize()
        h = self._ring[i]
        if len(rows) == 1:
            h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7] = rows[0]
        else:
            h.copy_(torch.tensor(rows, dtype=torch.float64).reshape(-1))
        self._hyper.copy_(h, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring_ev[i] = ev
        return self._hyper

    def _carry_skips(self, new_tab):
        """The skipped-step count lives in the table's device record: a new table inherits it (device-to-device, no sync)."""
        old = self._tab
        if old is not None and old.workspace is not None:
            if new_tab is None:
                self._skips_before += old.record()["skipped"]      # engine change: rare, may sync
            else:
                new_tab.workspace[16:24].copy_(old.workspace[16:24])
        return new_tab

    def _named_steps(self, steps):
        return {name: int(steps.get(name, 0)) for name, *_ in self._owned}

    # ------------------------------------------------------------------ checkpoint (resume, absent upstream)
    def state_dict(self):
        """torch's state_dict plus the fused state: the step count `t`, the per-parameter step counts `steps` (name -> count, None while
        every owned parameter is at `t`) and the flat first / second moment buffers (engine layout).  Without them a resume would restart
        the bias correction at t = 1 with zero moments."""
        sd = super().state_dict()
        steps = self._steps if self._loaded_steps is None else self._loaded_steps
        sd["fused"] = dict(t=self._t, steps=None if steps is None else dict(steps),
                           m=None if self._m is None else self._m.detach().cpu().clone(),
                           v=None if self._v is None else self._v.detach().cpu().clone())
        return sd

    def load_state_dict(self, state_dict):
        fused = state_dict.get("fused")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "fused"})
        if fused is None:
            raise KeyError("FusedAdamW.load_state_dict: no 'fused' entry (moments / step count): not a FusedAdamW checkpoint")
        self._t = int(fused["t"])
        steps = fused.get("steps")              # absent in checkpoints written before per-parameter counts: every parameter at t
        self._steps, self._loaded_steps = None, None
        if steps is not None:
            if self._bound is not None:
                self._steps = self._named_steps(steps)
            else:
                self._loaded_steps = dict(steps)
        if fused["m"] is not None:
            eng = self._bind()
            if fused["m"].numel() != eng.P.numel():
                raise ValueError(f"checkpoint moments have {fused['m'].numel()} elements, the engine's flat buffer {eng.P.numel()}")
            self._m.copy_(fused["m"].to(self._m.device))
            self._v.copy_(fused["v"].to(self._v.device))

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        eng = self._bind()
        # torch skips parameters whose .grad is None: after zero_grad() and before the next backward that is all of them
        # (the flat gradient buffer still holds the previous step's values - they must not be applied twice)
        owned = self._owned
        live = [o for o in owned if o[1].grad is not None]
        if not live:
            return loss
        for hook in self.pre_step_hooks:
            hook()
        pw = eng.Pw if eng.dtype == "bf16" else None
        plain = (len(live) == len(owned) and self._covers_all and self._steps is None and len(self.param_groups) == 1
                 and self.max_grad_norm is None and not self.skip_nonfinite)
        if plain:           # the reference's optimiser: one launch over the whole buffer, alignment padding included
            self._t += 1
            g = self.param_groups[0]
            hyper = self._upload_hyper([adamw_hyper_row(g["lr"], g["betas"], g["eps"], g["weight_decay"], self._t, self.grad_scale)])
            K.adamw_step(eng.P, eng.G, self._m, self._v, pw, eng.P.numel(), hyper)
            return loss
        if len(live) != len(owned) and self._steps is None:
            self._steps = {o[0]: self._t for o in owned}
        # one hyper row per distinct (group, step count of this update); in ordinary training that is one row per group
        rows, sig = {}, []
        for o in live:
            key = (o[4], (self._t if self._steps is None else self._steps[o[0]]) + 1)
            sig.append((o[2], rows.setdefault(key, len(rows))))
        sig = tuple(sig)
        if sig != self._sig:            # the set of updated parameters (or how they share rows) changed: new table, uploaded once
            tab = K.OptimRanges([(o[2], o[2] + o[3], r) for o, (_, r) in zip(live, sig)], eng.P.numel(), len(rows), device=eng.P.device)
            self._tab, self._sig, self._tab_names = self._carry_skips(tab), sig, [o[0] for o in live]
        hyper = self._upload_hyper([adamw_hyper_row(g["lr"], g["betas"], g["eps"], g["weight_decay"], t, self.grad_scale)
                                    for (gi, t) in rows for g in (self.param_groups[gi],)])
        measured = self.max_grad_norm is not None or self.skip_nonfinite
        if measured:
            K.grad_sumsq_ranges(eng.G, self._tab, coef_in=self.grad_scale, max_norm=self.max_grad_norm or 0.0,
                                skip_nonfinite=self.skip_nonfinite)
        K.adamw_step_ranges(eng.P, eng.G, self._m, self._v, pw, self._tab, hyper, clipped=measured, skip_nonfinite=self.skip_nonfinite)
        self._t += 1
        if self._steps is not None:
            for o in live:
                self._steps[o[0]] += 1
        return loss

    # ------------------------------------------------------------------ the device record (each of these synchronises)
    def _record(self):
        if self._tab is None or not (self.max_grad_norm is not None or self.skip_nonfinite):
            raise RuntimeError("no gradient norm was measured: construct with max_grad_norm or skip_nonfinite and take a step first")
        return self._tab.record()

    def last_grad_norm(self):
        """2-norm of the gradients the last step() updated with (after grad_scale, before clipping)."""
        return math.sqrt(self._record()["total"])

    def grad_norms(self):
        """name -> 2-norm of that parameter's gradient at the last step()."""
        return {name: math.sqrt(s) for name, s in zip(self._tab_names, self._record()["range_sumsq"])}

    def last_clip_coef(self):
        return self._record()["clip_coef"]

    def skipped_steps(self):
        """Steps skip_nonfinite left out so far."""
        return self._skips_before + self._record()["skipped"]

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None


def freeze_parameters(model, patterns):
    """requires_grad_(False) on every parameter of `model` whose name matches one of the fnmatch `patterns` (None or empty: nothing is
    frozen).  Names are the module's own (`encoder.0.attn.query.weight`), with or without a data-parallel wrapper around it.  Returns the
    frozen names; a pattern that matches no parameter is an error.  Call it before the optimiser is made: the engine launches only the
    backward the trainable parameters need (Engine.backward_report), the optimiser skips the frozen ones."""
    import fnmatch
    patterns = [patterns] if isinstance(patterns, str) else list(patterns or [])
    named = dict(getattr(model, "module", model).named_parameters())
    frozen = []
    for pat in patterns:
        hit = [k for k in named if fnmatch.fnmatchcase(k, pat)]
        if not hit:
            raise ValueError(f"freeze pattern {pat!r} matches no parameter (names look like {next(iter(named))!r})")
        frozen += [k for k in hit if k not in frozen]
    for k in frozen:
        named[k].requires_grad_(False)
    return [k for k in named if k in frozen]


def make_optimizer(model, lr, weight_decay, eps, param_groups=None, max_grad_norm=None, skip_nonfinite=False):
    """What train_multi_modal.py:197-202 builds, fused.  The engine is bound lazily at the first step.  param_groups: torch's list of
    dicts ({"params": [...], "lr": ..., "weight_decay": ...}); None: one group over model.parameters(), as the reference builds."""
    opt = FusedAdamW(model.parameters() if param_groups is None else param_groups, lr=lr, weight_decay=weight_decay, eps=eps,
                     max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    inner = getattr(model, "module", model)
    opt._model = inner
    orig_bind = opt._bind

    def bind():
        if opt.engine is None or opt.engine is not inner._engine:
            opt.engine = inner.engine()
        return orig_bind()
    opt._bind = bind
    return opt
