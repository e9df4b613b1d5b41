#!/usr/bin/env python3
"""Generate tests/golden/grad_accum_curve.json: the reference model driven by the standard gradient-accumulation loop.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_grad_accum_goldens.py

Per run (k = 3 and k = 4 over the same batches): the tiny model (oracle.make_goldens.tiny_model_cfg, model seed 7) on the TINY shape
(B = 2, T = 8, 12 + 2 channels, dropout 0), 4 epochs of 8 batches, batch j of epoch e being the synthetic batch of data seed
SEED_BASE + 8 e + j.  Groups of k consecutive batches, the epoch's last group closing short (k = 3: 3, 3, 2; k = 4: 4, 4); per batch of
a group of r `(loss / r).backward()`, per group `opt.step(); sch.step(); opt.zero_grad()` with make_opt's AdamW + OneCycleLR over
total_steps = epochs x groups per epoch.  The objective is sampled per batch as oracle.make_goldens.run_curve samples it per step.
Stored: every batch's loss and objective, the group sizes, (lr, beta1) at every optimiser step, the norm of every parameter's
accumulated gradient after the first group (before its step) and the final parameter norms, both in named_parameters order (params).
"""
import math
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

EPOCHS, BATCHES, MODEL_SEED = 4, 8, 7


def group_sizes(n_batches, k):
    return [k] * (n_batches // k) + ([n_batches % k] if n_batches % k else [])


def run(k, seed_base):
    """The record of one run, or None where a batch's reference loss is NaN (the caller moves the seed base)."""
    model = G.build_model(G.tiny_model_cfg(), G.TINY["n_ap"], G.TINY["n_beh"], seed=MODEL_SEED)
    model.train()
    sizes = group_sizes(BATCHES, k)
    opt, sch = G.make_opt(model, EPOCHS * len(sizes))
    random.seed(42)
    torch.manual_seed(1234)
    rec = dict(k=k, epochs=EPOCHS, batches_per_epoch=BATCHES, group_sizes=sizes, total_steps=EPOCHS * len(sizes), seed_base=seed_base,
               model_seed=MODEL_SEED, **G.TINY, params=[n for n, _ in model.named_parameters()], loss=[], objective=[], lr=[], beta1=[],
               first_group_grad_norm=None, final_param_norm=None)
    index = 0
    for _ in range(EPOCHS):
        for r in sizes:
            for _ in range(r):
                obj = random.sample(["encoding", "decoding", "token_masking"], 1)[0]
                out = model(G.make_mod_dict(G.synth_batch(seed=seed_base + index, **G.TINY), obj))
                if math.isnan(float(out.loss)):
                    return None
                (out.loss / r).backward()
                rec["loss"].append(float(out.loss))
                rec["objective"].append(obj)
                index += 1
            if rec["first_group_grad_norm"] is None:
                rec["first_group_grad_norm"] = [float(p.grad.double().norm()) for _, p in model.named_parameters()]
            rec["lr"].append(opt.param_groups[0]["lr"])
            rec["beta1"].append(opt.param_groups[0]["betas"][0])
            opt.step()
            sch.step()
            opt.zero_grad()
    rec["final_param_norm"] = [float(p.detach().double().norm()) for _, p in model.named_parameters()]
    print(f"    k = {k}: groups {sizes}, {len(rec['lr'])} optimiser steps, loss {rec['loss'][:2]} ... {rec['loss'][-1]}")
    return rec


if __name__ == "__main__":
    seed_base = 0
    while True:
        runs = {f"k{k}": run(k, seed_base) for k in (3, 4)}
        if all(v is not None for v in runs.values()):
            break
        seed_base += 1000
        print(f"    a batch's reference loss is NaN: seed base moved to {seed_base}")
    G.save_json("grad_accum_curve.json", runs)
