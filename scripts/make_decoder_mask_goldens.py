#!/usr/bin/env python3
"""Generate the decoder-mask fixture under tests/golden/ by importing the reference with `decoder.decoder_causal_mask` /
`decoder.decoder_sep_mask` set (mm.py:178-194).

TEST INFRASTRUCTURE ONLY, like oracle/make_goldens.py (whose helpers it imports and does not change): runs where the reference
checkout exists (MMFM_REFERENCE), never on the GPU box, and stores data only.

    python scripts/make_decoder_mask_goldens.py

decoder_mask_scalars.json   a dh-32 model on the default sequence length, so that the decoder self-attention of the HIP engine runs on
                            the fast kernels (csrc/attention_fast.hip) with CAUSAL / SEP: H = 256, 8 heads, inter 512, 1 encoder and
                            2 decoder layers, max_F = T = 100, 24 + 2 channels (L = 200, the modality boundary at 100 lies inside
                            key tile 3), dropout 0, B = 4 with two right-padded samples.  Per case (causal, sep, causal_sep) and
                            objective: loss, per-modality loss and n, the absolute sum of the predictions and the norm of every
                            gradient by parameter name.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import make_goldens as G  # noqa: E402  (chdirs into the reference and puts it on sys.path)

CFG = dict(H=256, heads=8, inter=512, n_enc=1, n_dec=2, max_F=100)
B, T, N_AP, N_BEH = 4, 100, 24, 2
PAD = [0, 3, 0, 10]
MODEL_SEED, DATA_SEED, MASK_SEED = 42, 5, 1
CASES = {"causal": dict(causal=True), "sep": dict(sep=True), "causal_sep": dict(causal=True, sep=True)}


def main():
    res = dict(meta=dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, pad=PAD, model_seed=MODEL_SEED, data_seed=DATA_SEED, mask_seed=MASK_SEED,
                         cases={k: dict(causal=bool(v.get("causal", False)), sep=bool(v.get("sep", False))) for k, v in CASES.items()},
                         **CFG),
               cases={})
    batch = G.synth_batch(B, T, N_AP, N_BEH, seed=DATA_SEED, pad=PAD)
    for name, kw in CASES.items():
        model = G.build_model(G.tiny_model_cfg(dropout=0.0, emb_dropout=0.0, **CFG, **kw), N_AP, N_BEH, seed=MODEL_SEED)
        model.eval()
        res["cases"][name] = {}
        for obj in ("encoding", "decoding", "token_masking"):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(MASK_SEED)
            out = model(G.make_mod_dict(batch, obj))
            out.loss.backward()
            res["cases"][name][obj] = dict(
                loss=float(out.loss), mod_loss={m: float(v) for m, v in out.mod_loss.items()},
                n={m: int(v) for m, v in out.mod_n_examples.items()},
                pred_abssum={m: float(v.double().abs().sum()) for m, v in out.mod_preds.items()},
                grad_norm={k: float(p.grad.double().norm()) for k, p in model.named_parameters()})
            print("   ", name, obj, res["cases"][name][obj]["loss"])
    G.save_json("decoder_mask_scalars.json", res)


if __name__ == "__main__":
    main()
