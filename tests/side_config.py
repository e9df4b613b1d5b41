"""Shared by tests/test_side_config_*.py: model configs whose `encoder.*` and `decoder.*` sections differ, built from the switches
tests/golden/side_config_fwd_bwd.npz records (scripts/make_side_config_goldens.py: case -> side -> section -> keys)."""
import copy

from conftest import load_npz
from helpers import model_config, tiny_config

CASES = ("HEADS", "INTER", "DROP0", "NORM", "NORM_R", "ACT", "EMB", "ALL")
OBJECTIVES = ("encoding", "decoding", "token_masking")
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("side_config_fwd_bwd.npz")
    return _Z


def with_sides(mc, switches):
    """`mc` (a DictConfig from helpers.model_config) with each side's sections updated: switches[side][section] = {key: value}."""
    from utils.config_utils import DictConfig
    m = copy.deepcopy(dict(mc))
    for side, secs in switches.items():
        for sec, upd in secs.items():
            m[side][sec].update(upd)
    return DictConfig(m)


def case_config(case, **kw):
    return with_sides(tiny_config(**kw), fixture()[1]["switches"][case])


def sides(enc=None, dec=None, enc_emb=None, dec_emb=None, **kw):
    """The YAML model under helpers.model_config(**kw) with `transformer` (enc, dec) and `embedder` (enc_emb, dec_emb) updates."""
    return with_sides(model_config(**kw), dict(encoder=dict(transformer=enc or {}, embedder=enc_emb or {}),
                                               decoder=dict(transformer=dec or {}, embedder=dec_emb or {})))
