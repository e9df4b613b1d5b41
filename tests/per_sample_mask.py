"""Shared by tests/test_per_sample_mask_*.py and scripts/make_per_sample_mask_goldens.py: the case table of
tests/golden/per_sample_mask_fwd_bwd.npz - the batch and the explicit per-sample token masks of each case - on the batches and mod_dicts
of tests/mod_segments.py, and the torch restatement of the mask products and of the stitch pair under a per-sample keep mask that the
kernel tests use as their reference.  Plain torch, no model code: the script feeds the same dicts to the reference."""
import torch

import edge_refs as E
import mod_segments as S
import mod_segments_refs as S_refs

OBJECTIVES, MODS, TINY = S.OBJECTIVES, S.MODS, S.TINY
MODEL_SEED, DATA_SEED = S.MODEL_SEED, S.DATA_SEED

# case -> T / stamps / pad / sep / causal: as tests/mod_segments.py CASES; masks: per modality and sample the masked bins (an explicit
# eval_mask, so that no case depends on a lucky draw; None: the masker draws); objectives: what is recorded.  A mask may name a padded
# bin: mask & attn takes it out, as upstream
CASES = {
    # sample 0 unmasked, the others masked: today's model zeroes nothing, and samples 1, 2 are scored on tokens they see
    "S0_OPEN": dict(T=(8, 8), masks=(((), (1, 4, 5), (0, 2, 7)), ((), (2, 3), (6,)))),
    # sample 0 fully masked, the others partly: today's model blinds every sample everywhere
    "S0_FULL": dict(T=(8, 8), masks=((tuple(range(8)), (0, 3), (5, 6, 7)), (tuple(range(8)), (1,), (2, 4)))),
    # bin 3 of the spikes masked in every sample (a dead bin under keep_any), the rest differs
    "BIN_ALL": dict(T=(8, 8), masks=(((3,), (3, 6), (0, 3)), ((1,), (), (1, 5)))),
    # padding on sample 0 and on sample 2 (shared bins: both modalities carry the same attention mask); masks reach into the padding.
    # encoding / decoding: the all-ones mask & attn leaves sample 0's padded bins unmasked and the others' masked - the two modes differ
    "PAD": dict(T=(8, 8), pad=((2, 0, 1), (2, 0, 1)), masks=(((0, 6, 7), (2, 7), (4,)), ((5,), (0, 1), (7,))),
                objectives=OBJECTIVES),
    # the masker's own draw (token_masking): the script asserts that sample 0's mask differs from another sample's
    "DRAWN": dict(T=(8, 8), masks=None),
    # a segmented batch (8, 5) with per-modality masks, stamps and padding
    "SEG": dict(T=(8, 5), stamps="shifted", pad=((0, 2, 0), (2, 0, 1)), masks=(((1,), (0, 5), (2, 3, 7)), ((0, 4), (), (1,)))),
    # causal + sep decoder masks
    "CAUSAL_SEP": dict(T=(8, 8), sep=True, causal=True, masks=(((2,), (0, 1, 2), (7,)), ((), (4, 5), (0,)))),
}
FULL_GRAD, FULL_GRAD_CASES = "token_masking", ("PAD",)
# modal_filter: the encoder has spikes only, the decoder behaviour only - each side stitches under its own modality's masks
FILTER = dict(case="FILTER", T=(8, 8), masks=(((1, 2), (), (0, 6, 7)), ((), (3, 4), (0, 1, 2, 3, 4, 5, 6, 7))), input=["ap"],
              output=["behavior"], objectives=("token_masking",))
EVAL_CASES = ("S0_OPEN", "SEG")              # one eval-mode forward each under the case's explicit masks
CURVE = dict(B=3, T=8, n_ap=12, n_beh=2, steps=50)


def switches(case):
    return FILTER if case == FILTER["case"] else CASES[case]


def case_batch(case, seed=DATA_SEED):
    sw = switches(case)
    return S.ragged_batch(TINY["B"], sw["T"], TINY["n_ap"], TINY["n_beh"], seed, sw.get("stamps", "arange"), sw.get("pad"), TINY["max_F"])


def explicit_masks(batch, masks):
    """mod -> eval_mask int64 shaped like the modality's inputs (only [:, :, 0] is read), 1 at the bins `masks` names per sample."""
    out = {}
    for i, mod in enumerate(MODS):
        em = torch.zeros_like(batch[mod]["inputs"], dtype=torch.int64)
        for b, bins in enumerate(masks[i]):
            em[b, list(bins)] = 1
        out[mod] = em
    return out


def mod_dict(case, objective, seed=DATA_SEED):
    """The case's mod_dict: tests/mod_segments.py make_mod_dict, with the case's explicit masks as eval_mask under token_masking."""
    batch = case_batch(case, seed)
    md = S.make_mod_dict(batch, objective)
    masks = switches(case)["masks"]
    if objective == "token_masking" and masks is not None:
        for mod, em in explicit_masks(batch, masks).items():
            md[mod]["eval_mask"] = em
    return md


# ---------------------------------------------------------------------------------------------- the kernels' reference, in torch
def mask_products(masks, attns, channels, row0=False):
    """What mmfm_mask_prep_rows writes, from one int64 mask [B, T_j] and attention mask [B, T_j] per slot: tokmask, keypad, keep u8 [B, L],
    keep_any u8 [L], mod_id u8 [L], count int64 [M].  v = mask & attn (mm.py:270); keep = (v != 1), upstream's `== 1` per sample.
    row0 = True is the injected fault: every sample under sample 0's row, today's keep0."""
    v = torch.cat([m & a for m, a in zip(masks, attns)], dim=1)
    keep = (v != 1)
    if row0:
        keep = keep[:1].expand_as(keep)
    return dict(tokmask=(v != 0).to(torch.uint8), keypad=(torch.cat(list(attns), dim=1) != 0).to(torch.uint8), keep=keep.to(torch.uint8),
                keep_any=keep.any(0).to(torch.uint8),
                mod_id=torch.cat([torch.full((m.shape[1],), j, dtype=torch.uint8) for j, m in enumerate(masks)]).to(v.device),
                count=torch.stack([(m & a).sum() * n for m, a, n in zip(masks, attns, channels)]).to(torch.int64))


def stitch_fwd(tok, mod_row, pos, ts, keep, off, max_F):
    """edge_refs.stitch_fwd sample by sample, each under its own keep row: (x, emb, mag), each [B, T, H] fp64, the slice
    [:, off:off + T] of the [B, L, H] outputs.  keep is the whole [B, L]."""
    B, T = ts.shape
    tk = tok.view(B, T, -1)
    parts = [E.stitch_fwd(tk[b], mod_row, pos, ts[b:b + 1], keep[b, off:off + T], 0, max_F) for b in range(B)]
    return tuple(torch.cat([p[i] for p in parts], 0) for i in range(3))


def stitch_bwd(dx, dextra, ts, keep, drop_keep, p, off, max_F):
    """mod_segments_refs.stitch_bwd for the slot at offset off with every row kept - d_mod, d_pos and their bounds do not depend on the
    keep mask - and d_tok[b*T + t] = keep[b, off + t] * dropout'(dx[b, off + t]) under the sample's own row.  The same dict."""
    B, T = ts.shape
    r = S_refs.stitch_bwd(dx, dextra, ts, torch.ones(keep.shape[1], dtype=torch.uint8, device=keep.device), drop_keep, p, off, max_F)
    r["d_tok"] = r["d_tok"] * E.f64(keep[:, off:off + T]).reshape(B * T)[:, None]
    return r
