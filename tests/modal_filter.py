"""Shared by tests/test_modal_filter_*.py: models whose encoder and decoder have tokenisers for different modality sets, built from the
switches tests/golden/modal_filter_fwd_bwd.npz records (scripts/make_modal_filter_goldens.py: case -> input / output / sep / causal /
share)."""
from conftest import load_npz
from helpers import build_model, model_config, tiny_config

CASES = ("DEC", "ENC", "AP", "BEH", "DEC_MASKS", "UNSHARED")
OBJECTIVES = ("encoding", "decoding", "token_masking")
BOTH = ["ap", "behavior"]
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("modal_filter_fwd_bwd.npz")
    return _Z


def switches(case):
    return fixture()[1]["switches"][case]


def case_model(case, n_ap=12, n_beh=2, seed=7, config=tiny_config, **kw):
    """The case's model: `config(**kw)` (tiny_config, or model_config for the YAML widths) with the case's decoder mask switches, and
    tokenisers for the case's modal_filter."""
    sw = switches(case)
    mc = config(sep=sw.get("sep", False), causal=sw.get("causal", False), **kw)
    return build_model(mc, n_ap, n_beh, seed=seed, modal_filter=dict(input=sw["input"], output=sw["output"]),
                       share_modality_embeddings=sw.get("share", True))


def engine_config(model, mods):
    """The EngineConfig MultiModal.engine() builds for `model` (needs no GPU)."""
    from multi_modal_foundation_model_amd.engine import EngineConfig
    return EngineConfig.from_model_config(model._model_config, mods, per_side=True, embedder_opts=True,
                                          enc_mods=[m for m in BOTH if m in model.encoder_embeddings],
                                          dec_mods=[m for m in BOTH if m in model.decoder_embeddings],
                                          share_mod_emb=model._share_mod_emb)


__all__ = ["CASES", "OBJECTIVES", "BOTH", "fixture", "switches", "case_model", "engine_config", "model_config", "tiny_config"]
