"""Modalities of different length, time stamps and padding, without a GPU: what tests/golden/mod_segments_* hold, the two guards of
MultiModal.forward (raised before an engine exists), what forward hands the engine for shared and for per-modality bins, and the
engine's batch key."""
import math

import numpy as np
import pytest
import torch

import mod_segments as S
from conftest import load_json, load_npz
from helpers import build_model, tiny_config
from oracle import mm_oracle as O


def test_fixture_covers_every_case_and_objective():
    z, meta = load_npz("mod_segments_fwd_bwd.npz")
    assert (meta["B"], meta["n_ap"], meta["n_beh"], meta["H"], meta["heads"], meta["inter"], meta["max_F"]) == (3, 12, 2, 32, 4, 64, 8)
    assert (meta["model_seed"], meta["data_seed"], meta["masker_seed"]) == (7, 3, 11) and meta["switches"] == {k: {a: (list(map(list, b)) if a == "pad" else list(b) if a == "T" else b) for a, b in v.items()} for k, v in S.CASES.items()}
    assert meta["cases"] == [f"{c}/{o}" for c in S.CASES for o in S.OBJECTIVES] and len(meta["cases"]) == 21
    for p in meta["cases"]:
        case = p.split("/")[0]
        T = S.CASES[case]["T"]
        nan = math.isnan(float(z[f"{p}/loss"]))
        assert nan == (p in meta["nan"])
        for i, (mod, n) in enumerate((("ap", 12), ("behavior", 2))):
            assert z[f"{p}/preds/{mod}"].shape == (3, T[i], n) and z[f"{p}/mask/{mod}"].shape == (3, T[i])
            assert int(z[f"{p}/n/{mod}"]) == int(z[f"{p}/mask/{mod}"].sum()) * n
        assert len(z[f"{p}/grad_norm"]) == len(meta["params"][case])
        stored = [k for k in z.files if k.startswith(f"{p}/grad/")]
        assert len(stored) == (len(meta["params"][case]) if p == "ALL/token_masking" else 0)
    for case in S.CASES:
        assert [k for k, _ in meta["state"][case]] and all(f"init/{h}" in z.files for h in meta["init"][case].values())
        for mod, d in S.case_batch(case).items():
            for k, v in d.items():
                np.testing.assert_array_equal(v.numpy(), z[f"batch/{case}/{mod}/{k}"])
    # the padding really sits where the case table says, sample 0 included
    attn = z["batch/ALL/behavior/attn"]
    assert attn.sum(1).tolist() == [3, 5, 4] and z["batch/ALL/ap/attn"].sum(1).tolist() == [8, 6, 8]
    assert z["batch/ALL/behavior/ts"].max() < 8 and z["batch/ALL/behavior/ts"][1].tolist() == [0, 7, 6, 5, 4]
    g = load_json("mod_segments_curve.json")["ALL"]
    assert len(g["loss"]) == len(g["objective"]) == 50 and set(g["objective"]) == set(S.OBJECTIVES) and all(math.isfinite(x) for x in g["loss"])


class EngineStub:
    """Stands where the engine would: records what forward hands over and ends the call."""
    class Reached(Exception):
        pass

    def forward(self, B, T, inputs, targets, masks, ts, attn, **kw):
        self.call = dict(B=B, T=T, ts=ts, attn=attn, shapes=[tuple(x.shape) for x in inputs])
        raise self.Reached


def forward_call(model, md, monkeypatch):
    stub = EngineStub()
    monkeypatch.setattr(model, "engine", lambda: stub)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    with pytest.raises(EngineStub.Reached):
        model(md)
    torch.set_rng_state(state)
    return stub.call


def test_uniform_batch_takes_the_shared_bins_path(monkeypatch):
    model = build_model(tiny_config(), 12, 2, seed=7)
    md = O.make_mod_dict(O.synth_batch(3, 8, 12, 2, seed=3, pad=[0, 2, 0]), "token_masking")
    call = forward_call(model, md, monkeypatch)
    assert call["T"] == 8 and isinstance(call["T"], int) and call["ts"] is md["ap"]["inputs_timestamp"] and call["attn"] is md["ap"]["inputs_attn_mask"]
    for key in ("inputs_timestamp", "inputs_attn_mask"):             # equal copies are shared bins too
        md["behavior"][key] = md["behavior"][key].clone()
    call = forward_call(model, md, monkeypatch)
    assert call["T"] == 8 and torch.is_tensor(call["ts"]) and torch.is_tensor(call["attn"])


@pytest.mark.parametrize("case", ["LEN", "STATIC", "STAMPS", "PAD"])
def test_ragged_batch_hands_the_engine_per_modality_segments(case, monkeypatch):
    model = build_model(tiny_config(), 12, 2, seed=7)
    md = S.make_mod_dict(S.case_batch(case), "token_masking")
    call = forward_call(model, md, monkeypatch)
    T = S.CASES[case]["T"]
    assert call["T"] == T and isinstance(call["T"], tuple) and call["shapes"] == [(3, T[0], 12), (3, T[1], 2)]
    assert all(a is md[m]["inputs_timestamp"] for a, m in zip(call["ts"], S.MODS)) and all(a is md[m]["inputs_attn_mask"] for a, m in zip(call["attn"], S.MODS))
    z, _ = load_npz("mod_segments_fwd_bwd.npz")                  # the masker's exact stream at each modality's own length
    for mod in S.MODS:
        np.testing.assert_array_equal(md[mod]["inputs_mask"].numpy(), z[f"{case}/token_masking/mask/{mod}"])


def test_sides_of_different_total_length_raise_before_the_engine(monkeypatch):
    model = build_model(tiny_config(), 12, 2, seed=7, modal_filter=dict(input=["ap"], output=["behavior"]))
    monkeypatch.setattr(model, "engine", lambda: pytest.fail("forward reached the engine"))
    with pytest.raises(RuntimeError, match="length 8 .* length 5 "):
        model(S.make_mod_dict(S.case_batch("LEN"), "encoding"))
    model = build_model(tiny_config(), 12, 2, seed=7, modal_filter=dict(input=["ap"], output=["behavior"]))
    call = forward_call(model, S.make_mod_dict(S.case_batch("STAMPS"), "decoding"), monkeypatch)       # 8 against 8: each side sums its own list
    assert call["T"] == (8, 8)


@pytest.mark.parametrize("key", ["targets", "inputs_timestamp", "inputs_attn_mask", "eval_mask"])
def test_a_modality_that_disagrees_with_itself_raises_value_error(key, monkeypatch):
    model = build_model(tiny_config(), 12, 2, seed=7)
    monkeypatch.setattr(model, "engine", lambda: pytest.fail("forward reached the engine"))
    md = S.make_mod_dict(S.case_batch("LEN"), "encoding")
    md["behavior"][key] = md["behavior"][key][:, :4]
    with pytest.raises(ValueError, match="behavior"):
        model(md)


def test_engine_batch_key():
    from multi_modal_foundation_model_amd.engine import Engine, EngineConfig
    eng = object.__new__(Engine)                                      # batch_key reads the modality list alone: no device needed
    eng.cfg = EngineConfig.from_model_config(tiny_config(), [("ap", 12), ("behavior", 2)], per_side=True, embedder_opts=True)
    ts, attn, ts2 = torch.zeros(3, 8), torch.ones(3, 8), torch.zeros(3, 8)
    assert eng.batch_key(8, ts, attn) == (8, ts, attn) and eng.batch_key((8, 8), [ts, ts], [attn, attn])[0] == 8
    assert eng.batch_key((8, 8), [ts, ts2], [attn, attn])[0] == (8, 8) and eng.batch_key((8, 5), [ts, ts2[:, :5]], attn)[0] == (8, 5)
    with pytest.raises(ValueError):
        eng.batch_key((8, 5, 1), ts, attn)
