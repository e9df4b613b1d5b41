#!/usr/bin/env python3
"""Generate the softmax cross-entropy fixtures under tests/golden/ by running the reference's own MultiModal on three-modality
batches whose third modality is categorical, with the loss restated in tests/ce_refs.py dropped into its `loss_mod`.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.  The mirror's `multi_modal` package collides with the
reference's by name, so nothing of the mirror is imported here: the loss is tests/ce_refs.py's plain-torch restatement in a module.

    python scripts/make_softmax_ce_goldens.py

softmax_ce_fwd_bwd.npz  per case (tests/ce_refs.py CE_CASES: `choice`, a per-trial label of 3 classes with bins (8, 8, 1), class weights
                        and smoothing 0.1 - a segmented plan; `state`, a per-bin label of 5 classes with bins (8, 8, 8), plain - the
                        uniform plan; tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0, n_modality = 3, B = 3, model seed 7,
                        data seed 3, masker seed 11) x (given eval masks, token_masking): loss, per-modality n / loss / preds / masks,
                        the norm of every gradient (order: meta params); every gradient tensor in full for choice / eval_masks; the
                        case's batch; the state dict's keys and shapes, the parameter names and the initial parameters by hash.
softmax_ce_curve.json   per case 50 AdamW + OneCycle steps, the objective sampled per step, step s on the batch of data seed s.
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ce_refs as R  # noqa: E402
from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

FULL_GRAD = "choice/eval_masks"


class RefSoftmaxCE(torch.nn.Module):
    """tests/ce_refs.py's e = - w t' log_softmax(p) as a `loss_mod` entry of the reference (in the predictions' dtype)."""

    def __init__(self, weight, eps):
        super().__init__()
        self.weight, self.eps = None if weight is None else torch.tensor(weight, dtype=torch.float32), eps

    def forward(self, preds, targets):
        return R.ce_elem(preds, targets.to(preds.dtype), self.weight, self.eps)


def build_model(case):
    c = R.CE_CASES[case]
    cfg = G.tiny_model_cfg(max_F=8, n_modality=3)
    torch.manual_seed(R.CE_MODEL_SEED)
    enc = {mod: G.EncoderEmbedding(hidden_size=32, n_channel=n, config=cfg.encoder) for mod, n in c["mods"]}
    dec = {mod: G.DecoderEmbedding(hidden_size=32, n_channel=n, output_channel=n, config=cfg.decoder) for mod, n in c["mods"]}
    model = G.MultiModal(enc, dec, avail_mod=[mod for mod, _ in c["mods"]], config=cfg, share_modality_embeddings=True)
    model.loss_mod[c["mods"][2][0]] = RefSoftmaxCE(c["weight"], c["eps"])
    return model


def record_step(arrs, model, case, obj, full):
    p = f"{case}/{obj}"
    model.zero_grad(set_to_none=True)
    torch.manual_seed(R.CE_MASKER_SEED)
    md = R.ce_mod_dict(case, R.ce_batch(case), obj)
    out = model(md)
    out.loss.backward()
    arrs[f"{p}/loss"] = G.npify(out.loss)
    for mod, _ in R.CE_CASES[case]["mods"]:
        arrs[f"{p}/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
        arrs[f"{p}/n/{mod}"] = G.npify(out.mod_n_examples[mod])
        arrs[f"{p}/preds/{mod}"] = G.npify(out.mod_preds[mod])
        arrs[f"{p}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
    arrs[f"{p}/grad_norm"] = np.array([float(prm.grad.double().norm()) for _, prm in model.named_parameters()])
    if full:
        for k, prm in model.named_parameters():
            arrs[f"{p}/grad/{k}"] = G.npify(prm.grad)
    print("   ", p, float(out.loss), {m: int(v) for m, v in out.mod_n_examples.items()})


def curve(case, steps=50):
    model = build_model(case)
    opt, sch = G.make_opt(model, steps)
    model.train()
    random.seed(42)
    torch.manual_seed(1234)
    losses, objs = [], []
    for step in range(steps):
        obj = random.sample(list(R.CE_OBJECTIVES), 1)[0]
        out = model(R.ce_mod_dict(case, R.ce_batch(case, seed=step), obj))
        out.loss.backward()
        opt.step()
        sch.step()
        opt.zero_grad()
        losses.append(float(out.loss))
        objs.append(obj)
    print("    curve", case, losses[:2], "...", losses[-1])
    return dict(loss=losses, objective=objs, model_seed=R.CE_MODEL_SEED, case=case, total_steps=steps, B=R.CE_B)


if __name__ == "__main__":
    meta = dict(B=R.CE_B, H=32, heads=4, inter=64, max_F=8, model_seed=R.CE_MODEL_SEED, data_seed=R.CE_DATA_SEED, masker_seed=R.CE_MASKER_SEED,
                cases=[], objectives=list(R.CE_OBJECTIVES), full_grad=FULL_GRAD, state={}, params={}, init={},
                spec={k: dict(mods=[list(m) for m in v["mods"]], T=list(v["T"]), weight=None if v["weight"] is None else list(v["weight"]),
                              eps=v["eps"]) for k, v in R.CE_CASES.items()})
    arrs = {}
    for case in R.CE_CASES:
        model = build_model(case)
        model.train()
        G.init_by_hash(arrs, meta, case, model)
        for mod, d in R.ce_batch(case).items():
            for k, v in d.items():
                arrs[f"batch/{case}/{mod}/{k}"] = G.npify(v)
        for obj in R.CE_OBJECTIVES:
            record_step(arrs, model, case, obj, f"{case}/{obj}" == FULL_GRAD)
            meta["cases"].append(f"{case}/{obj}")
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("softmax_ce_fwd_bwd.npz", **arrs)
    G.save_json("softmax_ce_curve.json", {case: curve(case) for case in R.CE_CASES})
