"""Shared by tests/test_context_window_model_gpu.py and scripts/make_context_window_goldens.py: the case table of
tests/golden/context_window_fwd_bwd.npz - (context.forward, context.backward) and the batch of each case - on the batches and mod_dicts of
tests/mod_segments.py.  Plain torch, no model code: the script feeds the same dicts to the reference."""
import mod_segments as S

OBJECTIVES, MODS, TINY = S.OBJECTIVES, S.MODS, S.TINY
MODEL_SEED, DATA_SEED = S.MODEL_SEED, S.DATA_SEED

# case -> ctx: (context.forward, context.backward); T / stamps / pad: as tests/mod_segments.py CASES.  The first four share bins (one
# length, the same arange stamps, no padding): the uniform plan, where the window over time stamps lets a spike bin see the behaviour
# bins of the same stamps.  QUIRK: `backward: 0` is unbounded.  SEG: a segmented plan - behaviour reversed and shifted per sample, padding
CASES = {
    "W11": dict(ctx=(1, 1), T=(8, 8)),
    "CAUSAL": dict(ctx=(0, -1), T=(8, 8)),
    "QUIRK": dict(ctx=(2, 0), T=(8, 8)),
    "BACK3": dict(ctx=(-1, 3), T=(8, 8)),
    "SEG": dict(ctx=(1, 2), T=(8, 5), stamps="shifted", pad=((0, 2, 0), (2, 0, 1))),
}
FULL_GRAD, FULL_GRAD_CASES = "token_masking", ("SEG",)
# modal_filter under the window: the encoder has spikes only, the decoder behaviour only, and behaviour's stamps differ from the spikes'
# (reversed, shifted per sample) - cross-attention must window decoder query i by the ENCODER's stamp i on both sides (mm.py:210).
# `encoding` masks nothing in the decoder's modality (loss NaN, n = 0, as upstream): the two other objectives are recorded, every
# gradient tensor for token_masking
FILTER = dict(case="FILTER", ctx=(1, 2), T=(8, 8), stamps="shifted", pad=((0, 2, 0), (2, 0, 1)), input=["ap"], output=["behavior"],
              objectives=("decoding", "token_masking"))
EVAL_CASES = ("W11", "SEG")                  # one eval-mode forward each (objective: encoding)
CURVE = dict(ctx=(0, 2), B=2, T=8, n_ap=12, n_beh=2, steps=50)


def case_batch(case, seed=DATA_SEED):
    sw = FILTER if case == FILTER["case"] else CASES[case]
    return S.ragged_batch(TINY["B"], sw["T"], TINY["n_ap"], TINY["n_beh"], seed, sw.get("stamps", "arange"), sw.get("pad"), TINY["max_F"])
