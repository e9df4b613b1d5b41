#!/usr/bin/env python3
"""Generate the modality-segment fixtures under tests/golden/ by running the reference on batches whose modalities differ in length,
time stamps and padding.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_mod_segments_goldens.py

mod_segments_fwd_bwd.npz  per case (tests/mod_segments.py CASES: per-modality bins, stamps, padding and the decoder mask switches, on
                          the tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0, B = 3, model seed 7, data seed 3, masker
                          seed 11) x the three objectives, what oracle.make_goldens.record_step stores: loss, per-modality n / loss /
                          preds / masks, the norm of every gradient (order: meta params); every gradient tensor in full for
                          ALL / token_masking; the case's batch (batch/<case>/<mod>/inputs | ts | attn); the state dict's keys and
                          shapes, the parameter names and the initial parameters by hash (init_by_hash).  A case / objective whose
                          reference loss is NaN (n = 0) is listed in meta nan.
mod_segments_curve.json   50 AdamW + OneCycle steps on ALL by oracle.make_goldens.run_curve's recipe (the objective is sampled per
                          step), step s on the ragged batch of data seed s.
"""
import json
import math
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import mod_segments as S  # noqa: E402
from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

FULL_GRAD, FULL_GRAD_CASES = "token_masking", ("ALL",)


def build_model(case):
    sw = S.CASES[case]
    return G.build_model(G.tiny_model_cfg(max_F=S.TINY["max_F"], sep=sw.get("sep", False), causal=sw.get("causal", False)),
                         S.TINY["n_ap"], S.TINY["n_beh"], seed=S.MODEL_SEED)


def ragged(fn):
    """Run fn with oracle.make_goldens' batch and mod_dict builders standing in for ragged ones: synth_batch hands the data seed on,
    make_mod_dict builds the case's batch of that seed."""
    def run(case, *a, **kw):
        with mock.patch.object(G, "synth_batch", lambda *_, seed, **__: seed), \
                mock.patch.object(G, "make_mod_dict", lambda seed, obj: S.make_mod_dict(S.case_batch(case, seed), obj)):
            return fn(case, *a, **kw)
    return run


@ragged
def record_case(case, arrs, meta):
    model = build_model(case)
    model.train()
    G.init_by_hash(arrs, meta, case, model)
    for mod, d in S.case_batch(case).items():
        for k, v in d.items():
            arrs[f"batch/{case}/{mod}/{k}"] = G.npify(v)
    for obj in S.OBJECTIVES:
        p = f"{case}/{obj}"
        full = obj == FULL_GRAD and case in FULL_GRAD_CASES
        G.record_step(arrs, model, S.DATA_SEED, p, obj, lambda k: full)
        if math.isnan(float(arrs[f"{p}/loss"])):
            meta["nan"].append(p)
        meta["cases"].append(p)


@ragged
def curve(case):
    model = build_model(case)
    l, o = G.run_curve(model, 50, S.TINY["B"], None, S.TINY["n_ap"], S.TINY["n_beh"], total_steps=50)
    print("    curve", case, l[:2], "...", l[-1])
    return dict(loss=l, objective=o, model_seed=S.MODEL_SEED, case=case, total_steps=50, **S.TINY)


if __name__ == "__main__":
    meta = dict(**S.TINY, H=32, heads=4, inter=64, model_seed=S.MODEL_SEED, data_seed=S.DATA_SEED, masker_seed=S.MASKER_SEED, cases=[],
                nan=[], switches=S.CASES, full_grad=FULL_GRAD, full_grad_cases=list(FULL_GRAD_CASES), state={}, params={}, init={})
    arrs = {}
    for case in S.CASES:
        record_case(case, arrs, meta)
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("mod_segments_fwd_bwd.npz", **arrs)
    G.save_json("mod_segments_curve.json", {"ALL": curve("ALL")})
