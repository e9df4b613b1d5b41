"""Per-session layers without a GPU: config parsing and the refusals, the layout of the session parameters, trunk transfer between
two session mappings, the eid -> session index and run-table builders as pure functions, the argument checks of the three C entry
points (they return before any HIP call) and tests/session_stitch.py against torch autograd in fp64."""
import ctypes as C

import numpy as np
import pytest
import torch

import session_stitch as R
from helpers import build_model, tiny_config
from multi_modal.session_layers import read_stitch_config, session_ids
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K
from multi_modal_foundation_model_amd.engine import EngineConfig, ParamLayout

T_ = R.TINY


def config(**stitcher):
    mc = tiny_config(max_F=T_["max_F"])
    mc["use_session"] = True
    if stitcher:
        mc["stitcher"] = stitcher
    return mc


# ------------------------------------------------------------------------------------------------- config
def test_config_defaults_and_values():
    mc = config()
    use, st = read_stitch_config(mc)
    assert use and st.width == mc["encoder"]["embedder"]["n_channels"] and st.bias is True and list(st.mods) == ["ap"]
    use, st = read_stitch_config(config(width=8, bias=False, mods=["ap", "behavior"]))
    assert (st.width, st.bias, list(st.mods)) == (8, False, ["ap", "behavior"])
    assert read_stitch_config(tiny_config()) == (False, None)


@pytest.mark.parametrize("bad", [dict(width="8"), dict(width=0), dict(width=True), dict(bias="yes"), dict(mods="ap"), dict(mods=[]), dict(mods=["ap", "ap"]),
                                 dict(mods=[1])])
def test_config_values_of_the_wrong_type_are_refused(bad):
    with pytest.raises(ValueError, match="stitcher"):
        read_stitch_config(config(**bad))
    mc = tiny_config()
    mc["stitcher"] = bad                     # read with the switch off too: a wrong value never waits for the switch
    with pytest.raises(ValueError, match="stitcher"):
        read_stitch_config(mc)


def test_use_session_must_be_a_bool():
    mc = tiny_config()
    mc["use_session"] = "true"
    with pytest.raises(ValueError, match="use_session"):
        read_stitch_config(mc)


def test_sessions_keyword_is_required_with_the_switch_and_refused_without():
    with pytest.raises(ValueError, match="sessions"):
        build_model(config(width=8), 12, 2, seed=1)
    with pytest.raises(ValueError, match="use_session"):
        build_model(tiny_config(), 12, 2, seed=1, sessions=R.SESSIONS)
    for bad in ({}, {"a": 0}, {"a": True}, {3: 4}, [("a", 3)]):
        with pytest.raises(ValueError, match="sessions"):
            build_model(config(width=8), 12, 2, seed=1, sessions=bad)
    with pytest.raises(ValueError, match="stitcher.mods"):
        build_model(config(width=8, mods=["lfp"]), 12, 2, seed=1, sessions=R.SESSIONS)


# ------------------------------------------------------------------------------------------------- the module and the layout
def test_parameters_names_shapes_and_init_order():
    model = build_model(config(width=8), 12, 2, seed=R.MODEL_SEED, sessions=R.SESSIONS)
    plain = build_model(tiny_config(max_F=T_["max_F"]), 8, 2, seed=R.MODEL_SEED)            # the n_channel = P model without sessions
    names = [k for k, _ in model.named_parameters()]
    trunk = [k for k, _ in plain.named_parameters()]
    assert names[:len(trunk)] == trunk
    for (k, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), k                 # created last: every existing parameter has the plain model's bits
    want = [f"session_{w}.ap.{k}.{kind}" for w in ("in", "out") for k in range(3) for kind in ("weight", "bias")]
    assert names[len(trunk):] == want
    sd = model.state_dict()
    for k, n in enumerate(R.SESSIONS.values()):
        assert tuple(sd[f"session_in.ap.{k}.weight"].shape) == (n, 8) and tuple(sd[f"session_in.ap.{k}.bias"].shape) == (8,)
        assert tuple(sd[f"session_out.ap.{k}.weight"].shape) == (n, 8) and tuple(sd[f"session_out.ap.{k}.bias"].shape) == (n,)
    assert model.session_index == {"ses.12": 0, "ses.7": 1, "ses.1": 2}
    ref = R.RefLayers(list(R.SESSIONS.values()), 8)             # the restatement draws the same values in the same order
    torch.manual_seed(R.MODEL_SEED)
    again = build_model(config(width=8), 12, 2, seed=R.MODEL_SEED, sessions=R.SESSIONS)
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), sd.values())) and ref is not None
    nobias = build_model(config(width=8, bias=False), 12, 2, seed=R.MODEL_SEED, sessions=R.SESSIONS)
    assert not any(k.startswith("session_") and k.endswith(".bias") for k in nobias.state_dict())


def test_layout_segments_and_no_slot_with_the_switch_off():
    mc = config(width=8)
    mods = [("ap", 8), ("behavior", 2)]
    on = ParamLayout(EngineConfig.from_model_config(mc, mods, per_side=True, embedder_opts=True, sessions={"ap": (12, 7, 1)}))
    off = ParamLayout(EngineConfig.from_model_config(mc, mods, per_side=True, embedder_opts=True))
    assert not any(k.startswith("session_") for k in off.entries)
    seg = {name: (s, e) for name, s, e in on.segments}
    for k, (o, shape) in on.entries.items():
        if k.startswith("session_"):
            lo, hi = seg["embed" if k.startswith("session_in") else "head"]
            assert lo <= o and o + int(np.prod(shape)) <= hi and o % 8 == 0, k
    assert on.entries["session_out.ap.1.bias"][1] == (7,) and on.entries["session_in.ap.1.bias"][1] == (8,)
    # the trunk keeps the order it has without sessions; the session entries close their segments
    assert [k for k in on.entries if not k.startswith("session_")] == list(off.entries)
    assert EngineConfig.from_model_config(mc, mods, per_side=True, embedder_opts=True) == EngineConfig.from_model_config(mc, mods, per_side=True, embedder_opts=True, sessions=None)
    with pytest.raises(ValueError, match="sessions"):
        EngineConfig.from_model_config(mc, mods, per_side=True, embedder_opts=True, sessions={"lfp": (3,)})


def test_trunk_transfers_between_session_mappings():
    a = build_model(config(width=8), 12, 2, seed=1, sessions=R.SESSIONS)
    b = build_model(config(width=8), 12, 2, seed=2, sessions={"new.1": 5, "new.2": 9})
    trunk = {k: v for k, v in a.state_dict().items() if not k.startswith("session_")}
    res = b.load_state_dict(trunk, strict=False)
    assert not res.unexpected_keys and all(k.startswith("session_") for k in res.missing_keys) and len(res.missing_keys) == 8
    for k, v in trunk.items():
        assert torch.equal(b.state_dict()[k], v), k
    assert b.session_index == {"new.1": 0, "new.2": 1}
    from multi_modal_foundation_model_amd.optim import freeze_parameters
    freeze_parameters(b, ["session_in.*"])
    assert [k for k, p in b.named_parameters() if not p.requires_grad] == [k for k, _ in b.named_parameters() if k.startswith("session_in.")]


def test_ddp_refuses_session_layers():
    from multi_modal_foundation_model_amd.ddp import EngineDDP

    class E:
        cfg = EngineConfig.from_model_config(config(width=8), [("ap", 8), ("behavior", 2)], per_side=True, embedder_opts=True, sessions={"ap": (3, 2)})
    with pytest.raises(NotImplementedError, match="use_session"):
        EngineDDP(E())


# ------------------------------------------------------------------------------------------------- eid -> sid, the run table
def test_session_ids():
    index, sizes = {"a.x": 0, "b": 1, "c": 2}, (12, 7, 1)
    assert session_ids("b", 3, index, sizes, 12) == [1, 1, 1]
    assert session_ids(["c", "a.x", "c"], 3, index, sizes, 12) == [2, 0, 2]
    with pytest.raises(ValueError, match="'zz'"):
        session_ids(["a.x", "zz", "b"], 3, index, sizes, 12)
    with pytest.raises(ValueError, match="a.x"):
        session_ids(["b", "a.x"], 2, index, sizes, 11)             # the batch is narrower than a present session
    assert session_ids(["b", "c"], 2, index, sizes, 7) == [1, 2]  # ... absent ones do not matter
    with pytest.raises(ValueError):
        session_ids(["b"], 2, index, sizes, 12)
    with pytest.raises(ValueError):
        session_ids(None, 2, index, sizes, 12)


def entries(runs, B):
    live = int(runs[0])
    return [tuple(int(x) for x in runs[4 + B + 4 * i: 8 + B + 4 * i]) for i in range(live)], [int(x) for x in runs[4:4 + B]]


@pytest.mark.parametrize("sid, S, chunk, want_entries, want_order", [
    ([1, 1, 1, 1], 3, 4, [(1, 0, 4, 1)], [0, 1, 2, 3]),                                     # single session, one chunk: direct
    ([1, 1, 1, 1, 1], 3, 2, [(1, 0, 2, 3), (1, 2, 2, 0), (1, 4, 1, 0)], [0, 1, 2, 3, 4]),   # ... three chunks, the last ragged
    ([2, 0, 2, 0, 2], 3, 2, [(0, 0, 2, 1), (2, 2, 2, 2), (2, 4, 1, 0)], [1, 3, 0, 2, 4]),   # interleaved, session 1 absent
    ([3, 2, 1, 0], 4, 1, [(0, 0, 1, 1), (1, 1, 1, 1), (2, 2, 1, 1), (3, 3, 1, 1)], [3, 2, 1, 0]),      # all distinct
])
def test_run_table(sid, S, chunk, want_entries, want_order):
    B = len(sid)
    runs = K.session_runs(sid, S, chunk)
    assert runs.dtype == np.int32 and runs.size == L.lib().mmfm_session_runs_ints(B, S, chunk) == K.session_runs_ints(B, S, chunk)
    assert list(runs[:4]) == [len(want_entries), chunk, L.lib().mmfm_session_dw_chunks(B, S, chunk), B]
    got, order = entries(runs, B)
    assert got == want_entries and order == want_order
    assert not runs[4 + B + 4 * len(want_entries):].any()


def test_run_table_capacity_and_the_64_session_refusal():
    for B, S, chunk in [(1, 1, 1), (5, 3, 1), (6, 4, 2), (1024, 40, 16), (3, 100, 1), (200, 300, 1), (130, 500, 2)]:
        assert K.session_dw_chunks(B, S, chunk) == L.lib().mmfm_session_dw_chunks(B, S, chunk)
    K.session_runs(list(range(64)) * 2, 70, 2)                       # 64 distinct sessions fit
    with pytest.raises(ValueError, match="65 distinct sessions.*e7"):
        K.session_runs(list(range(65)), 70, 1, names=[f"e{k}" for k in range(70)])
    with pytest.raises(ValueError, match="outside"):
        K.session_runs([0, 3], 3, 1)
    assert K.session_dw_chunk(1024) == 16 and K.session_dw_chunk(4) == 1


# ------------------------------------------------------------------------------------------------- the C entry points' argument checks
@pytest.mark.parametrize("case", list(R.BAD_DESC) + list(R.BAD_FWD))
def test_forward_entry_points_refuse_bad_arguments_before_launching(case):
    kw, msg = (R.BAD_DESC.get(case) or R.BAD_FWD[case])
    d = R.fake_desc(L, **kw)
    for fn in (L.lib().mmfm_session_reduce, L.lib().mmfm_session_expand):
        assert fn(C.byref(d), R.FAKE, R.FAKE, None) == -1
        assert msg in L.lib().mmfm_last_error().decode()
    good = R.fake_desc(L)
    assert L.lib().mmfm_session_reduce(C.byref(good), None, R.FAKE, None) == -1 and L.lib().mmfm_session_expand(C.byref(good), R.FAKE, None, None) == -1
    assert L.lib().mmfm_session_reduce(None, R.FAKE, R.FAKE, None) == -1


@pytest.mark.parametrize("case", list(R.BAD_DESC) + ["NULL runs", "NULL dw", "chunk 0", "bias flag", "small workspace", "misaligned workspace", "db without b_off"])
def test_dw_refuses_bad_arguments_before_launching(case):
    lib = L.lib()
    need = lib.mmfm_session_dw_workspace(4, 8, 12, 3, 1)
    assert need == K.session_dw_chunks(4, 3, 1) * (12 * 8 + 12) * 4
    a = dict(d=R.fake_desc(L, **R.BAD_DESC[case][0]) if case in R.BAD_DESC else R.fake_desc(L), a=R.FAKE, q=R.FAKE, runs=R.FAKE, chunk=1, dw=R.FAKE, db=R.FAKE,
             flag=0, ws=R.FAKE, nbytes=need)
    a.update({"NULL runs": dict(runs=None), "NULL dw": dict(dw=None), "chunk 0": dict(chunk=0), "bias flag": dict(flag=2), "small workspace": dict(nbytes=need - 1),
              "misaligned workspace": dict(ws=R.FAKE + 4), "db without b_off": dict(d=R.fake_desc(L, b_off=None))}.get(case, {}))
    assert lib.mmfm_session_dw(C.byref(a["d"]), a["a"], a["q"], a["runs"], a["chunk"], a["dw"], a["db"], a["flag"], a["ws"], a["nbytes"], None) == -1
    assert lib.mmfm_last_error().decode().startswith("mmfm_session_dw")
    for bad in ((0, 8, 12, 3, 1), (4, 0, 12, 3, 1), (4, 8, 12, 3, 0)):
        assert lib.mmfm_session_dw_workspace(*bad) == -1


def test_header_declares_the_feature_macro():
    with open(L.HEADER_PATH) as f:
        src = f.read()
    assert "#define MMFM_SESSION_LINEAR 1" in src and "#define MMFM_VERSION 401" in src
    for name in ("mmfm_session_reduce", "mmfm_session_expand", "mmfm_session_dw", "mmfm_session_dw_workspace", "mmfm_session_dw_chunks", "mmfm_session_runs_ints"):
        assert name in L.header_symbols() and name in L._PROTOS


# ------------------------------------------------------------------------------------------------- the restatement against autograd (fp64)
@pytest.mark.parametrize("mixname", R.MIXES)
@pytest.mark.parametrize("shape", R.SHAPES[:1] + R.SHAPES[3:])
def test_references_against_autograd(shape, mixname):
    B, T, P, N_max, base = shape
    sizes = R.session_sizes(B, base)
    sid = R.mix(mixname, B, len(base))
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(B, T, N_max)
    for b, k in enumerate(sid):
        x[b, :, sizes[k]:] = float("nan")                       # never read
    Win, bin_ = [rnd(n, P).requires_grad_() for n in sizes], [rnd(P).requires_grad_() for _ in sizes]
    Wout, bout = [rnd(n, P).requires_grad_() for n in sizes], [rnd(n).requires_grad_() for n in sizes]
    u = R.read_in(x, sid, sizes, Win, bin_)
    ref, _, _ = R.reduce_ref(x, sid, sizes, Win, bin_)
    assert torch.allclose(u, ref, rtol=1e-12, atol=1e-12) and bool(torch.isfinite(u).all())
    f = rnd(B, T, P).requires_grad_()
    pred = R.read_out(f, sid, sizes, Wout, bout, N_max)
    ref, _, _ = R.expand_ref(f, sid, sizes, Wout, bout, N_max)
    assert torch.allclose(pred, ref, rtol=1e-12, atol=1e-12)
    v = R.channel_mask(sid, sizes, N_max)
    assert all(bool((pred[b, :, sizes[k]:] == 0).all()) and int(v[b].sum()) == sizes[k] for b, k in enumerate(sid))
    # gradients: du / dW_in / db_in from a cotangent on u, df / dW_out / db_out from one on pred
    du, dpred = rnd(B, T, P), rnd(B, T, N_max)
    present = sorted(set(sid))
    gin = torch.autograd.grad(u, [Win[k] for k in present] + [bin_[k] for k in present], du)
    gout = torch.autograd.grad(pred, [f] + [Wout[k] for k in present] + [bout[k] for k in present], dpred)
    xz = torch.nan_to_num(x)
    rin, rout = R.dw_ref(xz, du, sid, sizes), R.dw_ref(dpred, f.detach(), sid, sizes)
    for i, k in enumerate(present):
        assert torch.allclose(gin[i], rin[k]["dW"], rtol=1e-10, atol=1e-10) and torch.allclose(gin[len(present) + i], rin[k]["db_q"], rtol=1e-10, atol=1e-10)
        assert torch.allclose(gout[1 + i], rout[k]["dW"], rtol=1e-10, atol=1e-10) and torch.allclose(gout[1 + len(present) + i], rout[k]["db_a"], rtol=1e-10, atol=1e-10)
    df, _, _ = R.reduce_ref(dpred, sid, sizes, [w.detach() for w in Wout], None)          # df = dpred . Wout: the reduce form without a bias
    assert torch.allclose(gout[0], df, rtol=1e-10, atol=1e-10)
    absent = set(range(len(sizes))) - set(sid)
    assert all(Win[k].grad is None for k in absent)
