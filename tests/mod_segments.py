"""Shared by tests/test_mod_segments_*.py and scripts/make_mod_segments_goldens.py: batches whose modalities differ in length, time
stamps and padding (the case table of tests/golden/mod_segments_fwd_bwd.npz) and the mod_dict upstream's trainer would build of them.
Plain torch, no model code: the script feeds the same dicts to the reference."""
import numpy as np
import torch

OBJECTIVES = ("encoding", "decoding", "token_masking")
MODS = ("ap", "behavior")
TINY = dict(B=3, n_ap=12, n_beh=2, max_F=8)
MODEL_SEED, DATA_SEED, MASKER_SEED = 7, 3, 11

# case -> T: bins of (ap, behavior); stamps: "arange" or "shifted" (behavior reversed and shifted per sample, all < max_F; ap arange);
# pad: right-padded bins per sample of (ap, behavior); sep / causal: decoder_sep_mask / decoder_causal_mask
CASES = {
    "LEN": dict(T=(8, 5)),
    "LEN_REV": dict(T=(5, 8)),
    "STATIC": dict(T=(8, 1)),
    "STAMPS": dict(T=(8, 8), stamps="shifted"),
    "PAD": dict(T=(8, 8), pad=((0, 2, 0), (3, 0, 1))),
    "ALL": dict(T=(8, 5), stamps="shifted", pad=((0, 2, 0), (2, 0, 1)), sep=True, causal=True),
    "ALL_SEP": dict(T=(8, 5), stamps="shifted", pad=((0, 2, 0), (2, 0, 1)), sep=True),
}


def ragged_batch(B, T, n_ap, n_beh, seed, stamps="arange", pad=None, max_F=8):
    """mod -> dict(inputs [B, T_mod, N_mod], ts [B, T_mod] int64, attn [B, T_mod] int64): Poisson(0.3) spikes and N(0, 1) behaviour from
    one generator (the recipe of oracle.mm_oracle.synth_batch, each modality at its own length)."""
    g = torch.Generator().manual_seed(seed)
    data = dict(ap=torch.poisson(torch.full((B, T[0], n_ap), 0.3), generator=g), behavior=torch.randn(B, T[1], n_beh, generator=g))
    out = {}
    for i, mod in enumerate(MODS):
        t = torch.arange(T[i], dtype=torch.int64)[None].repeat(B, 1)
        if stamps == "shifted" and mod == "behavior":
            t = (max_F - 1 - t + torch.arange(B, dtype=torch.int64)[:, None]) % max_F
        attn = torch.ones(B, T[i], dtype=torch.int64)
        for b, p in enumerate(pad[i] if pad else ()):
            if p:
                attn[b, T[i] - p:] = 0
        out[mod] = dict(inputs=data[mod], ts=t, attn=attn)
    return out


def case_batch(case, seed=DATA_SEED):
    sw = CASES[case]
    return ragged_batch(TINY["B"], sw["T"], TINY["n_ap"], TINY["n_beh"], seed, sw.get("stamps", "arange"), sw.get("pad"), TINY["max_F"])


def make_mod_dict(batch, objective):
    """What MultiModalTrainer._forward_model_outputs builds (trainer/base.py:51-103), each modality with its own bins: the eval masks
    are shaped like the modality's own inputs (only [:, :, 0] is read)."""
    md = {}
    n_ap = batch["ap"]["inputs"].shape[-1]
    for i, mod in enumerate(MODS):
        s = batch[mod]
        x = s["inputs"]
        d = dict(inputs_modality=torch.tensor(i), targets_modality=torch.tensor(i), inputs_attn_mask=s["attn"], inputs_timestamp=s["ts"],
                 targets_timestamp=s["ts"], eid="synthetic", num_neuron=n_ap, masking_mode=None, inputs=x.clone(), targets=x.clone())
        if mod == "ap":
            d["inputs_regions"] = np.full((x.shape[0], n_ap), "XX")
        if objective == "token_masking":
            d["eval_mask"] = None
        elif objective in ("encoding", "decoding"):
            on = (objective == "encoding") == (mod == "ap")
            d["eval_mask"] = (torch.ones_like if on else torch.zeros_like)(x).to(torch.int64)
        else:
            raise ValueError(objective)
        md[mod] = d
    return md
