"""Shared by tests/test_input_masking_model_gpu.py and scripts/make_input_masking_goldens.py: the case table of
tests/golden/input_masking_fwd_bwd.npz, its batches, the masker settings and the mod_dict a trainer with mask_type: input builds.
Plain torch, no model code: the script feeds the same dicts to the reference's pieces."""
import numpy as np
import torch

import mod_segments as S

TINY = dict(B=3, T=8, n_ap=12, n_beh=2, max_F=8)
MODEL_SEED, DATA_SEED, MASKER_SEED = 7, 3, 11
REGION_MODES = ("inter-region", "intra-region")
CURVE_MODES = ["neuron", "inter-region", "intra-region", "temporal"]          # training.mask_mode of the curve, sampled per step
CURVE_STEPS = 50
# the masker's settings for every case (the YAML's, with what the modes beyond `temporal` need): channels / timesteps are valid for
# both modalities (2 behaviours, 8 bins); expand_prob 0.5 / max_timespan 2 exercise both time-span branches
MASKER = dict(ratio=0.3, zero_ratio=1.0, random_ratio=1.0, expand_prob=0.5, max_timespan=2, channels=[1], timesteps=[5, 6],
              mask_regions=["all"], target_regions=["all"], n_mask_regions=1, causal_zero=True, force_active=True)
# case -> mode, masker overrides, bins of (ap, behavior)
CASES = {mode: dict(mode=mode) for mode in ("temporal", "neuron", "random", "co-smooth", "forward-pred", "inter-region", "intra-region", "causal")}
CASES["real_draw"] = dict(mode="neuron", masker=dict(zero_ratio=0.5, random_ratio=1.0))       # the masker corrupts the inputs itself
CASES["ragged"] = dict(mode="neuron", T=(8, 5))
FULL_GRAD = ("neuron", "intra-region")


def regions(B, n_ap=TINY["n_ap"]):
    """[B, n_ap] region names: 12 neurons in 3 regions."""
    row = (["CA1"] * 5 + ["PO"] * 4 + ["LP"] * 3)[:n_ap]
    return np.array([row] * B)


def set_masker(masker, case=None):
    """The case's masker settings on a model's masker (either implementation: plain attributes)."""
    for k, v in dict(MASKER, **(CASES[case].get("masker", {}) if case else {})).items():
        setattr(masker, k, list(v) if isinstance(v, list) else v)


def case_batch(case=None, seed=DATA_SEED):
    T = CASES[case].get("T", (TINY["T"], TINY["T"])) if case else (TINY["T"], TINY["T"])
    return S.ragged_batch(TINY["B"], T, TINY["n_ap"], TINY["n_beh"], seed, max_F=TINY["max_F"])


def make_mod_dict(batch, mode):
    """mod_segments.make_mod_dict with the trainer's masking_mode on every modality and the regions of the spikes."""
    md = S.make_mod_dict(batch, "token_masking")
    for d in md.values():
        d["masking_mode"] = mode
    md["ap"]["inputs_regions"] = regions(batch["ap"]["inputs"].shape[0])
    return md
