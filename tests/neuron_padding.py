"""Shared by tests/test_neuron_padding_*.py and scripts/make_neuron_padding_goldens.py: the case table of
tests/golden/neuron_padding_fwd_bwd.npz, its batches - spikes padded with -1 as the loader pads them, with the space_attn_mask to match -
and the mod_dict a trainer with training.neuron_padding builds.  Plain torch, no model code: the script feeds the same dicts to the
reference's pieces."""
import torch

import input_masking as IM
import mod_segments as S

TINY = dict(IM.TINY)                       # B 3, T 8, 12 neurons, 2 behaviours, max_F 8
MODEL_SEED, DATA_SEED, MASKER_SEED = 7, 3, 11
PAD_VALUE = -1.0
# case -> objective (the trainer's training_mode) or mode (an input-masking mode: masking_mode on every modality); n: real channels per
# sample; side: where the padding sits; T: bins of (ap, behavior); pad: right-padded bins per sample of (ap, behavior)
CASES = {
    "enc_right": dict(objective="encoding", n=(12, 7, 0)),              # one sample with every channel real, one with none
    "dec_right": dict(objective="decoding", n=(12, 7, 0)),
    "tok_right": dict(objective="token_masking", n=(12, 7, 0)),
    "tok_left": dict(objective="token_masking", n=(5, 12, 9), side="left"),
    "enc_left": dict(objective="encoding", n=(0, 12, 4), side="left"),
    "enc_timepad": dict(objective="encoding", n=(9, 12, 6), pad=((0, 2, 0), (0, 2, 0))),
    "enc_ragged": dict(objective="encoding", n=(12, 7, 3), T=(8, 5)),
    "enc_allpad": dict(objective="encoding", n=(0, 0, 0)),              # nothing is a target: 0 / 0
    "im_temporal": dict(mode="temporal", n=(12, 7, 0)),                 # a [B,T,1] target mask: the row mask of the chan form
    "im_neuron": dict(mode="neuron", n=(12, 7, 3)),                     # a [B,1,N] target mask: AND-ed, the element form
    # the masker corrupts the inputs itself (noise and kept values under its mask): staging zeroes the padded channels alone
    "im_real_draw": dict(mode="neuron", n=(12, 7, 3), masker=dict(zero_ratio=0.5, random_ratio=1.0)),
    "im_real_draw_rows": dict(mode="temporal", n=(12, 7, 0), masker=dict(zero_ratio=0.5, random_ratio=1.0)),
}
FULL_GRAD = ("enc_right", "im_neuron")
CURVE_SESSIONS = (12, 9, 6)                # n_k of the curve's three sessions; step s is a batch of session s % 3
CURVE_STEPS = 50


def set_masker(masker, case=None):
    """tests/input_masking.py's masker settings with the case's overrides."""
    IM.set_masker(masker)
    for k, val in (CASES[case].get("masker", {}) if case else {}).items():
        setattr(masker, k, val)


def channel_mask(n, n_ap=TINY["n_ap"], side="right"):
    """space_attn_mask [B, n_ap] int64 as collate.py emits it: sample b has n[b] real channels at the low (right padding) or the high
    (left padding) end."""
    v = torch.zeros(len(n), n_ap, dtype=torch.int64)
    for b, nb in enumerate(n):
        if side == "right":
            v[b, :nb] = 1
        else:
            v[b, n_ap - nb:] = 1
    return v


def pad_spikes(batch, v, value=PAD_VALUE):
    """The batch with the spike channels v clears set to the pad value, as the loader leaves them."""
    x = batch["ap"]["inputs"]
    batch["ap"]["inputs"] = torch.where(v[:, None, :] != 0, x, torch.full_like(x, value))
    return batch


def case_batch(case, seed=DATA_SEED, value=PAD_VALUE):
    """(batch of mod_segments.ragged_batch with padded spikes, space_attn_mask)."""
    sw = CASES[case]
    T = sw.get("T", (TINY["T"], TINY["T"]))
    v = channel_mask(sw["n"], side=sw.get("side", "right"))
    batch = S.ragged_batch(TINY["B"], T, TINY["n_ap"], TINY["n_beh"], seed, pad=sw.get("pad"), max_F=TINY["max_F"])
    return pad_spikes(batch, v, value), v


def curve_batch(step, value=PAD_VALUE):
    n = CURVE_SESSIONS[step % len(CURVE_SESSIONS)]
    v = channel_mask((n,) * TINY["B"])
    batch = S.ragged_batch(TINY["B"], (TINY["T"], TINY["T"]), TINY["n_ap"], TINY["n_beh"], step, max_F=TINY["max_F"])
    return pad_spikes(batch, v, value), v


def make_mod_dict(batch, v, objective=None, mode=None):
    """What a trainer with training.neuron_padding builds: the objective's mod_dict (or, for an input-masking mode, the one of
    tests/input_masking.py) with the batch's space_attn_mask in the `ap` entry.  v None: no key, the mod_dict it always was."""
    md = IM.make_mod_dict(batch, mode) if mode else S.make_mod_dict(batch, objective)
    if v is not None:
        md["ap"]["space_attn_mask"] = v.clone()
    return md


def case_mod_dict(case, batch, v):
    return make_mod_dict(batch, v, CASES[case].get("objective"), CASES[case].get("mode"))
