#!/usr/bin/env python3
"""Generate the context-window fixtures under tests/golden/ by running the reference with the one line it leaves undone filled in.

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.  Nothing of the mirror is imported.

The reference's forward_mask_encoder composes  self_mask | (context_mask & key padding)  with context_mask = ones under a TO DO.
`windowed` wraps that method of the reference's own MultiModal: it calls the original and puts the window over the tokens' time stamps
where the ones were,  eye | (band & returned mask)  - the same thing, because the returned mask is eye | key padding and eye absorbs
band & eye - with band[b, i, j] = lo <= stamp[b][j] - stamp[b][i] <= hi and (lo, hi) the translation of (context.forward,
context.backward) that tests/test_context_window_cpu.py proves against the reference's create_context_mask (for one modality on arange
stamps the band IS create_context_mask).  forward_decoder hands the same mask to cross-attention, as upstream; the decoder's own mask is
untouched.  Everything else is the reference's forward as it stands.

    python scripts/make_context_window_goldens.py

context_window_fwd_bwd.npz  per case of tests/context_window.py CASES (tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0,
                            B = 3, model seed 7, data seed 3, masker seed 11) x the three objectives, what
                            oracle.make_goldens.record_step stores; every gradient tensor in full for SEG / token_masking; the case's
                            batch; parameter names, state-dict keys and the initial parameters by hash; for EVAL_CASES one eval-mode
                            forward (encoding): loss, per-modality loss / n / preds.  One modal_filter case (FILTER: encoder spikes,
                            decoder behaviour, behaviour's stamps reversed and shifted): decoding and token_masking.
context_window_curve.json   50 AdamW + OneCycle steps with context (0, 2) by oracle.make_goldens.run_curve's recipe.
"""
import json
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import context_window as W  # noqa: E402
import context_window_refs as CW  # noqa: E402
import mod_segments as S  # noqa: E402
from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)


def windowed(model, ctx):
    """The reference model with its encoder mask windowed over time stamps (module docstring)."""
    lo, hi = CW.translate(*ctx)
    orig = model.forward_mask_encoder

    def forward_mask_encoder(mod_dict):
        tokens, emb, mask, attn, mod_mask = orig(mod_dict)
        pos = torch.cat([d["inputs_timestamp"] for d in mod_dict.values()], dim=1)
        eye = torch.eye(attn.shape[1], dtype=attn.dtype)[None]
        return tokens, emb, mask, eye | (CW.band(lo, hi, pos).to(attn.dtype) & attn), mod_mask
    model.forward_mask_encoder = forward_mask_encoder
    return model


def build_model(ctx):
    return windowed(G.build_model(G.tiny_model_cfg(max_F=W.TINY["max_F"]), W.TINY["n_ap"], W.TINY["n_beh"], seed=W.MODEL_SEED), ctx)


def ragged(fn):
    """Run fn with oracle.make_goldens' batch and mod_dict builders standing in for the case's: synth_batch hands the data seed on,
    make_mod_dict builds the case's batch of that seed."""
    def run(case, *a, **kw):
        with mock.patch.object(G, "synth_batch", lambda *_, seed, **__: seed), \
                mock.patch.object(G, "make_mod_dict", lambda seed, obj: S.make_mod_dict(W.case_batch(case, seed), obj)):
            return fn(case, *a, **kw)
    return run


@ragged
def record_case(case, arrs, meta):
    model = build_model(W.CASES[case]["ctx"])
    model.train()
    G.init_by_hash(arrs, meta, case, model)
    for mod, d in W.case_batch(case).items():
        for k, v in d.items():
            arrs[f"batch/{case}/{mod}/{k}"] = G.npify(v)
    for obj in W.OBJECTIVES:
        full = obj == W.FULL_GRAD and case in W.FULL_GRAD_CASES
        G.record_step(arrs, model, W.DATA_SEED, f"{case}/{obj}", obj, lambda k: full)
        meta["cases"].append(f"{case}/{obj}")
    if case in W.EVAL_CASES:
        model.eval()
        with torch.no_grad():
            out = model(S.make_mod_dict(W.case_batch(case), "encoding"))
        arrs[f"{case}/eval/loss"] = G.npify(out.loss)
        for mod in W.MODS:
            arrs[f"{case}/eval/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
            arrs[f"{case}/eval/n/{mod}"] = G.npify(out.mod_n_examples[mod])
            arrs[f"{case}/eval/preds/{mod}"] = G.npify(out.mod_preds[mod])
        print("   ", case, "eval", float(out.loss))


def record_filter(arrs, meta):
    """The modal_filter case (tests/context_window.py FILTER): the reference built with the tokeniser dicts of train_multi_modal.py under
    the filter (the encoder's tokenisers, then the decoder's: construction order = RNG contract), windowed; records over the decoder's
    modalities what record_step stores, with every gradient tensor for token_masking."""
    f = W.FILTER
    case = f["case"]
    cfg = G.tiny_model_cfg(max_F=W.TINY["max_F"])
    chan = dict(ap=W.TINY["n_ap"], behavior=W.TINY["n_beh"])
    torch.manual_seed(W.MODEL_SEED)
    enc = {m: G.EncoderEmbedding(hidden_size=cfg.encoder.transformer.hidden_size, n_channel=chan[m], config=cfg.encoder) for m in f["input"]}
    dec = {m: G.DecoderEmbedding(hidden_size=cfg.decoder.transformer.hidden_size, n_channel=chan[m], output_channel=chan[m],
                                 config=cfg.decoder) for m in f["output"]}
    model = windowed(G.MultiModal(enc, dec, avail_mod=list(W.MODS), config=cfg, share_modality_embeddings=True), f["ctx"])
    model.train()
    G.init_by_hash(arrs, meta, case, model)
    for mod, d in W.case_batch(case).items():
        for k, v in d.items():
            arrs[f"batch/{case}/{mod}/{k}"] = G.npify(v)
    for obj in f["objectives"]:
        p = f"{case}/{obj}"
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        md = S.make_mod_dict(W.case_batch(case), obj)
        out = model(md)
        assert list(out.mod_loss) == f["output"]
        out.loss.backward()
        arrs[f"{p}/loss"] = G.npify(out.loss)
        for mod in out.mod_loss:
            arrs[f"{p}/mod_loss/{mod}"] = G.npify(out.mod_loss[mod])
            arrs[f"{p}/n/{mod}"] = G.npify(out.mod_n_examples[mod])
            arrs[f"{p}/preds/{mod}"] = G.npify(out.mod_preds[mod])
        for mod in W.MODS:
            arrs[f"{p}/mask/{mod}"] = G.npify(md[mod]["inputs_mask"])
        arrs[f"{p}/grad_norm"] = np.array([float(prm.grad.double().norm()) for _, prm in model.named_parameters()])
        if obj == W.FULL_GRAD:
            for k, prm in model.named_parameters():
                arrs[f"{p}/grad/{k}"] = G.npify(prm.grad)
        meta["cases"].append(p)
        print("   ", p, float(out.loss.detach()))


def curve():
    c = W.CURVE
    model = windowed(G.build_model(G.tiny_model_cfg(max_F=W.TINY["max_F"]), c["n_ap"], c["n_beh"], seed=W.MODEL_SEED), c["ctx"])
    l, o = G.run_curve(model, c["steps"], c["B"], c["T"], c["n_ap"], c["n_beh"], total_steps=c["steps"])
    print("    curve", l[:2], "...", l[-1])
    return dict(loss=l, objective=o, model_seed=W.MODEL_SEED, total_steps=c["steps"], **{k: c[k] for k in ("B", "T", "n_ap", "n_beh")},
                ctx=list(c["ctx"]))


if __name__ == "__main__":
    meta = dict(**W.TINY, H=32, heads=4, inter=64, model_seed=W.MODEL_SEED, data_seed=W.DATA_SEED, masker_seed=S.MASKER_SEED, cases=[],
                switches={k: dict(v, ctx=list(v["ctx"])) for k, v in W.CASES.items()}, full_grad=W.FULL_GRAD,
                full_grad_cases=list(W.FULL_GRAD_CASES), eval_cases=list(W.EVAL_CASES),
                modal_filter=dict(W.FILTER, ctx=list(W.FILTER["ctx"]), objectives=list(W.FILTER["objectives"])), state={}, params={}, init={})
    arrs = {}
    for case in W.CASES:
        record_case(case, arrs, meta)
    record_filter(arrs, meta)
    arrs["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G.save_npz("context_window_fwd_bwd.npz", **arrs)
    G.save_json("context_window_curve.json", curve())
