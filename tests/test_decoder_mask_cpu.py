"""decoder.decoder_causal_mask / decoder.decoder_sep_mask on the host side (no GPU): the reference fixture
(tests/golden/decoder_mask_scalars.json, scripts/make_decoder_mask_goldens.py) loads, its cases and parameter names match the
module built from the same configuration, and the engine configuration carries both switches."""
import pytest

from conftest import load_json
from helpers import build_model, model_config
from multi_modal_foundation_model_amd.engine import EngineConfig

OBJECTIVES = ("encoding", "decoding", "token_masking")


def fixture_config(meta, case):
    return model_config(H=meta["H"], heads=meta["heads"], inter=meta["inter"], n_enc=meta["n_enc"], n_dec=meta["n_dec"], max_F=meta["max_F"],
                        dropout=0.0, emb_dropout=0.0, **meta["cases"][case])


def test_fixture_cases_and_shape():
    g = load_json("decoder_mask_scalars.json")
    meta = g["meta"]
    assert meta["cases"] == {"causal": dict(causal=True, sep=False), "sep": dict(causal=False, sep=True),
                             "causal_sep": dict(causal=True, sep=True)}
    assert set(g["cases"]) == set(meta["cases"])
    assert meta["H"] // meta["heads"] == 32 and 2 * meta["T"] == 200 and meta["max_F"] == meta["T"]      # dh 32, L = 200: the fast kernels
    for case in g["cases"].values():
        assert set(case) == set(OBJECTIVES)
        for c in case.values():
            assert set(c) == {"loss", "mod_loss", "n", "pred_abssum", "grad_norm"}
            assert all(isinstance(v, int) for v in c["n"].values())


@pytest.mark.parametrize("case", ["causal", "sep", "causal_sep"])
def test_fixture_parameter_names_match_module(case):
    g = load_json("decoder_mask_scalars.json")
    meta = g["meta"]
    model = build_model(fixture_config(meta, case), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    names = [k for k, _ in model.named_parameters()]
    for obj in OBJECTIVES:
        assert list(g["cases"][case][obj]["grad_norm"]) == names


@pytest.mark.parametrize("causal,sep", [(False, False), (True, False), (False, True), (True, True)])
def test_engine_config_carries_both_switches(causal, sep):
    c = EngineConfig.from_model_config(model_config(causal=causal, sep=sep), [("ap", 668), ("behavior", 2)])
    assert (bool(c.causal_mask), bool(c.sep_mask)) == (causal, sep)
