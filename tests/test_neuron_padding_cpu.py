"""Neuron padding (space_attn_mask with MultiModal.neuron_padding), host side: the header's feature macro and exports, the switch on
the model, the builders, the trainer and the entry script, the multi-session synthetic loader, the combination of element masks with
a channel mask against brute-force expansion, the plan key, and the evaluation driver's pass-through.  No GPU involved."""
import itertools
import re

import numpy as np
import pytest
import torch

from helpers import build_model, load_config, tiny_config

B, T, N = 3, 8, 12


def test_header_feature_macro_and_exports():
    from multi_modal_foundation_model_amd import _lib as L
    with open(L.HEADER_PATH) as f:
        src = f.read()
    assert re.search(r"^#define MMFM_LOSS_CHAN 1$", src, flags=re.M) and re.search(r"^#define MMFM_VERSION 401$", src, flags=re.M)
    names = {"mmfm_masked_loss_chan_workspace", "mmfm_masked_loss_chan_fwd", "mmfm_masked_loss_chan_bwd"}
    assert names <= set(L.header_symbols()) and names <= set(L._PROTOS)
    # the prototypes agree with the header's parameter lists: as many arguments, plus the stream
    flat = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in names:
        params = re.search(name + r"\s*\(([^)]*)\)", flat).group(1).split(",")
        assert len(params) == len(L._PROTOS[name][1]), name
    lib = L.lib()
    assert lib.mmfm_version() == 401
    # partials: 1024 floats, then 1024 int64 counts - the element form's layout
    assert lib.mmfm_masked_loss_chan_workspace(102400, 668) == 1024 * 4 + 1024 * 8 == lib.mmfm_masked_loss_elem_workspace(102400, 668)
    assert lib.mmfm_masked_loss_chan_workspace(15, 3) == 16 + 4 * 8


def test_argument_checks_come_before_any_hip_call():
    """Refused arguments return -1 with a text, without a device."""
    from multi_modal_foundation_model_amd import _lib as L
    lib = L.lib()
    assert lib.mmfm_masked_loss_chan_fwd(0, 1, 0.0, 0, None, None, None, 8, 8, 24, 12, None, 12, None, None, None, 0, None) == -1
    assert b"mmfm_masked_loss_chan_fwd: null pointer" in lib.mmfm_last_error()
    assert lib.mmfm_masked_loss_chan_bwd(0, 1, 0.0, 0, None, None, None, 8, 8, 24, 12, None, 12, None, None, None, None) == -1
    assert b"mmfm_masked_loss_chan_bwd: null pointer" in lib.mmfm_last_error()
    one = 8                                                    # any non-null address: the checks below fail before it is read
    for change, text in ((dict(dtype=3), b"bad dtype"), (dict(kind=7), b"bad kind"), (dict(R=25), b"bad arguments"), (dict(mask_ld=-8), b"bad arguments"),
                         (dict(chan_ld=-12), b"bad arguments"), (dict(chan_ld=5), b"bad arguments"), (dict(mask_ld=3), b"bad arguments")):
        a = dict(dtype=0, kind=1, mask_ld=8, R=24, chan_ld=12)
        a.update(change)
        rc = lib.mmfm_masked_loss_chan_bwd(a["dtype"], a["kind"], 0.0, 0, one, one, one, a["mask_ld"], 8, a["R"], 12, one, a["chan_ld"], one, one, one, None)
        assert rc == -1 and text in lib.mmfm_last_error(), (change, lib.mmfm_last_error())
    assert lib.mmfm_masked_loss_chan_fwd(0, 1, 0.0, 0, one, one, one, 8, 8, 24, 12, one, 12, one, one, 16, 8, None) == -1
    assert b"workspace" in lib.mmfm_last_error()


def test_chan_ld():
    from multi_modal_foundation_model_amd import ops as K
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    assert K.chan_ld(u8(3, 12), 12) == 12 and K.chan_ld(u8(1, 12), 12) == 0
    for bad in (u8(3, 11), u8(12), u8(3, 1, 12), torch.zeros(3, 12, dtype=torch.bool), u8(12, 3).t()):
        with pytest.raises(ValueError, match="channel mask"):
            K.chan_ld(bad, 12)


def test_switch_defaults_off_and_is_a_constructor_keyword():
    from multi_modal.mm import MultiModal
    assert MultiModal.neuron_padding is False
    assert build_model(tiny_config(), 12, 2, seed=1).neuron_padding is False
    assert build_model(tiny_config(), 12, 2, seed=1, neuron_padding=True).neuron_padding is True
    a, b = build_model(tiny_config(), 12, 2, seed=1), build_model(tiny_config(), 12, 2, seed=1, neuron_padding=True)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())


def test_model_refuses_a_mask_of_another_shape_before_any_draw():
    model = build_model(tiny_config(), 12, 2, seed=1, neuron_padding=True)
    x, beh = torch.zeros(B, T, 12), torch.zeros(B, T, 2)
    ok = model._channel_masks({"ap": dict(inputs=x, space_attn_mask=torch.tensor([[1] * 7 + [0] * 5] * B)), "behavior": dict(inputs=beh)})
    assert set(ok) == {"ap"} and ok["ap"].dtype == torch.uint8 and tuple(ok["ap"].shape) == (B, 12) and int(ok["ap"].sum()) == 7 * B
    before = torch.get_rng_state()
    for bad in (torch.ones(B, 11), torch.ones(B + 1, 12), torch.ones(12), torch.ones(B, 1, 12)):
        with pytest.raises(ValueError, match="'ap'"):
            model({"ap": dict(inputs=x, space_attn_mask=bad), "behavior": dict(inputs=beh)})
    assert torch.equal(torch.get_rng_state(), before)


def _trainer(**training):
    from trainer.make import make_multimodal_trainer

    class Acc:
        device = torch.device("cpu")
    cfg = load_config()
    for k, v in training.items():
        cfg["training"][k] = v
    model = build_model(tiny_config(), 12, 2, seed=1)
    tr = make_multimodal_trainer(model=model, train_dataloader=[], eval_dataloader=[], optimizer=None, log_dir="/tmp", accelerator=Acc(),
                                 lr_scheduler=None, avail_mod=["ap", "behavior"], config=cfg,
                                 modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=False, num_neurons=[12])
    return tr, model


def test_trainer_key():
    assert "neuron_padding" not in load_config()["training"], "no YAML file carries the key"
    tr, model = _trainer()
    assert tr.neuron_padding is False and model.neuron_padding is False
    tr, model = _trainer(neuron_padding=True)
    assert tr.neuron_padding is True and model.neuron_padding is True
    assert _trainer(neuron_padding=False)[1].neuron_padding is False
    for bad in (1, "true", "yes", None, 0.0):
        with pytest.raises(ValueError, match="neuron_padding"):
            _trainer(neuron_padding=bad)


def test_trainer_puts_the_mask_into_the_ap_entry_and_needs_it():
    from multi_modal_foundation_model_amd.synthetic import synth_batch
    seen = {}

    def fake(mod_dict):
        seen.update(mod_dict)
        return "out"
    batch = synth_batch(B, T, 12, 2, seed=5)
    batch["space_attn_mask"][:, 9:] = 0
    tr, model = _trainer(neuron_padding=True)
    tr.model = fake
    assert tr._forward_model_outputs(dict(batch), masking_mode=None, training_mode="token_masking") == "out"
    assert seen["ap"]["space_attn_mask"] is batch["space_attn_mask"] and "space_attn_mask" not in seen["behavior"]
    short = {k: v for k, v in batch.items() if k != "space_attn_mask"}
    with pytest.raises(ValueError, match="space_attn_mask"):
        tr._forward_model_outputs(short, masking_mode=None, training_mode="token_masking")
    seen.clear()
    tr, model = _trainer()
    tr.model = fake
    tr._forward_model_outputs(dict(batch), masking_mode=None, training_mode="token_masking")
    assert "space_attn_mask" not in seen["ap"], "switch off: the mod_dict is what it always was"


def test_entry_script_flags():
    import train_multi_modal as tm
    args = tm.build_parser().parse_args([])
    assert args.neuron_padding is False and args.n_sessions == 1
    args = tm.build_parser().parse_args(["--neuron_padding", "--n_sessions", "40"])
    assert args.neuron_padding is True and args.n_sessions == 40


def test_multi_session_loader():
    from multi_modal_foundation_model_amd.synthetic import MultiSessionLoader, SyntheticLoader, session_sizes, synth_batch
    K_ = 3
    rng = np.random.default_rng(2024)
    sizes = [int(rng.integers(300, 669)) for _ in range(K_)]          # bench.py's multi-session recipe
    assert session_sizes(K_, 668) == sizes and len(set(sizes)) > 1 and all(300 <= n <= 668 for n in sizes)
    assert session_sizes(40, 668)[:K_] == sizes, "one draw per session, in order"
    loader = MultiSessionLoader(5, 2, T=4, n_ap=668, n_beh=2, n_sessions=K_, seed0=11)
    assert len(loader) == 5 and loader.sizes == sizes
    batches, again = list(loader), list(MultiSessionLoader(5, 2, T=4, n_ap=668, n_beh=2, n_sessions=K_, seed0=11))
    plain = list(SyntheticLoader(5, 2, T=4, n_ap=668, n_beh=2, seed0=11))
    assert len(batches) == 5
    for i, (b, b2, p) in enumerate(zip(batches, again, plain)):
        n = sizes[i % K_]
        assert set(b) == set(p) == set(synth_batch(2, 4, 668, 2, seed=0)), "the loader contract's keys"
        for k in b:
            same = torch.equal(b[k], b2[k]) if torch.is_tensor(b[k]) else b[k] == b2[k]
            assert same, f"batch {i} key {k}: not deterministic"
        assert b["eid"] == [f"session{i % K_}"] * 2
        assert tuple(b["spikes_data"].shape) == (2, 4, 668) and b["space_attn_mask"].dtype == torch.int64
        assert bool((b["spikes_data"][:, :, n:] == -1).all()) and bool((b["spikes_data"][:, :, :n] >= 0).all())
        assert torch.equal(b["spikes_data"][:, :, :n], p["spikes_data"][:, :, :n]), "the real channels are synth_batch's"
        assert torch.equal(b["target"], p["target"])
        assert bool((b["space_attn_mask"][:, :n] == 1).all()) and bool((b["space_attn_mask"][:, n:] == 0).all())
    with pytest.raises(ValueError):
        MultiSessionLoader(1, 2, n_ap=200)
    # SyntheticLoader and synth_batch stay what they were
    assert bool((plain[0]["space_attn_mask"] == 1).all()) and bool((plain[0]["spikes_data"] >= 0).all())


# ---- the elem x chan combination (plan.combine_chan) against brute-force expansion
ELEM_SHAPES = [(B, T, 1), (1, T, 1), (B, 1, N), (1, 1, N), (B, T, N), (1, T, N), (B, 1, 1), (1, 1, 1)]
CHAN_SHAPES = [(B, N), (1, N)]


def _rand(shape, seed, density=0.5):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < density).to(torch.uint8)


@pytest.mark.parametrize("real_draw", [False, True], ids=["engine_zeroes", "masker_corrupted"])
@pytest.mark.parametrize("vshape", CHAN_SHAPES)
@pytest.mark.parametrize("cshape,tshape", list(itertools.product(ELEM_SHAPES, ELEM_SHAPES)))
def test_combine_chan_is_the_expanded_product(cshape, tshape, vshape, real_draw):
    from multi_modal_foundation_model_amd.plan import combine_chan
    cm, tm, v = _rand(cshape, 1), _rand(tshape, 2), _rand(vshape, 3, 0.6)
    corrupted = torch.randn(B, T, N) if real_draw else None
    (cm2, tm2, cor2), chan = combine_chan((cm, tm, corrupted), v, B, T, N)
    full = lambda m: m.expand(B, T, N)
    vfull = v[:, None, :].expand(B, T, N)
    assert cor2 is corrupted and cm2.dtype == torch.uint8 and cm2.is_contiguous()
    if real_draw:
        # the masker corrupted the inputs itself - noise and kept values under cm: staging zeroes the padded channels and nothing else
        assert torch.equal(full(cm2), 1 - vfull) and tuple(cm2.shape) == (vshape[0], 1, N)
        staged = torch.where(full(cm2) != 0, torch.zeros(()), corrupted)
        assert torch.equal(staged, torch.where(vfull != 0, corrupted, torch.zeros(())))
    else:
        # the engine does the masker's zeroing: staging zeroes the masker's elements and every padded channel
        assert torch.equal(full(cm2), full(cm) | (1 - vfull))
        assert tuple(cm2.shape) == tuple(max(a, b) for a, b in zip(cshape, (vshape[0], 1, N)))
    # the loss mask is tm & v, as row mask x channel mask or as one compact element mask
    if tshape in ((B, T, 1), (1, T, 1)):
        assert tm2 is tm and chan is not None and torch.equal(chan, v) and chan.is_contiguous()
        got = full(tm2) & chan[:, None, :].expand(B, T, N)
    else:
        assert chan is None and tm2.dtype == torch.uint8 and tm2.is_contiguous()
        assert tuple(tm2.shape) == tuple(max(a, b) for a, b in zip(tshape, (vshape[0], 1, N)))
        got = full(tm2)
    assert torch.equal(got, full(tm) & vfull)
    assert all(s in (1, f) for m in (cm2, tm2) for s, f in zip(m.shape, (B, T, N))), "the results are compact element masks"


@pytest.mark.parametrize("vshape", CHAN_SHAPES)
def test_combine_chan_without_element_masks(vshape):
    from multi_modal_foundation_model_amd.plan import combine_chan
    v = _rand(vshape, 4, 0.6)
    (cm, tm, corrupted), chan = combine_chan(None, v, B, T, N)
    assert tm is None and corrupted is None and torch.equal(chan, v)
    assert tuple(cm.shape) == (vshape[0], 1, N) and cm.dtype == torch.uint8 and torch.equal(cm[:, 0, :], 1 - v)
    for bad in (v.bool(), v[:, :5], v[None], torch.zeros(2, N, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="channel mask"):
            combine_chan(None, bad, B, T, N)


def test_plan_key_without_a_channel_mask_is_todays():
    from multi_modal_foundation_model_amd.engine import Engine
    from multi_modal_foundation_model_amd.plan import mask_key
    ekey = (((B, 1, N), (B, 1, N)), None)
    assert mask_key(None, None) is None and mask_key(ekey, None) is ekey
    ckey = ((B, N), None)
    assert mask_key(ekey, ckey) not in (ekey, None) and mask_key(ekey, ckey) != mask_key(ekey, ((1, N), None))
    assert Engine.chan_key(None) is None
    assert Engine.chan_key([torch.zeros(B, N, dtype=torch.uint8), None]) == ckey

    class Cfg:
        mods = [("ap", N), ("behavior", 2)]

    class Stub:
        cfg = Cfg()
    elem = [(torch.zeros(B, 1, N, dtype=torch.uint8),) * 2 + (None,), None]
    for chan in (None, [None, None]):
        out = Engine.fold_chan(Stub(), B, T, elem, chan)
        assert out[0] is elem and out[1] is None and out[2] == ()
        assert Engine.fold_chan(Stub(), B, T, None, chan) == (None, None, ())
    # a channel mask on 'ap' alone: its staging mask, the chan form, and 'behavior' as it was
    v = _rand((B, N), 7)
    e2, c2, padded = Engine.fold_chan(Stub(), B, T, None, [v, None])
    assert padded == (0,) and e2[1] is None and c2[1] is None and torch.equal(c2[0], v) and e2[0][1] is None
    assert Engine.elem_key(Stub(), e2) == (((B, 1, N), None), None)
    with pytest.raises(ValueError):
        Engine.fold_chan(Stub(), B, T, None, [v])


def test_eval_mod_dict_passes_the_mask_through():
    from multi_modal_foundation_model_amd.synthetic import synth_batch
    from utils.eval_utils import eval_mod_dict
    model = build_model(tiny_config(), 12, 2, seed=1)
    batch = synth_batch(B, T, 12, 2, seed=5)
    batch["space_attn_mask"][:, 9:] = 0
    mask_result = dict(spikes=batch["spikes_data"], eval_mask=torch.zeros(B, T, 12, dtype=torch.int64))
    md = eval_mod_dict(model, batch, mask_result, "neuron")
    assert md["ap"]["space_attn_mask"] is batch["space_attn_mask"] and "space_attn_mask" not in md["behavior"]
    del batch["space_attn_mask"]
    assert "space_attn_mask" not in eval_mod_dict(model, batch, mask_result, "neuron")["ap"]


# ---- the reference fixture's own consistency (tests/golden/neuron_padding_*; scripts/make_neuron_padding_goldens.py)
def test_golden_is_consistent_with_its_case_table():
    import neuron_padding as NP
    from conftest import load_json, load_npz
    z, meta = load_npz("neuron_padding_fwd_bwd.npz")
    assert meta["cases"] == list(NP.CASES) and meta["full_grad"] == list(NP.FULL_GRAD)
    nan_cases = []
    for case, sw in NP.CASES.items():
        batch, v = NP.case_batch(case)
        for mod in ("ap", "behavior"):
            for k in ("inputs", "ts", "attn"):
                assert np.array_equal(z[f"batch/{case}/{mod}/{k}"], batch[mod][k].numpy()), (case, mod, k)
        assert np.array_equal(z[f"batch/{case}/space_attn_mask"], v.numpy())
        vb = v.numpy()[:, None, :] != 0
        x = z[f"batch/{case}/ap/inputs"]
        assert bool((x[np.broadcast_to(~vb, x.shape)] == NP.PAD_VALUE).all()) and bool((x[np.broadcast_to(vb, x.shape)] >= 0).all())
        # the staged spikes: padded channels zeroed whatever else happened to the inputs
        staged = z[f"{case}/inputs/ap"]
        assert bool((staged[np.broadcast_to(~vb, staged.shape)] == 0).all())
        if "objective" in sw:
            assert np.array_equal(staged, np.where(vb, x, 0.0))
            assert np.array_equal(z[f"{case}/inputs/behavior"], z[f"batch/{case}/behavior/inputs"])
        total_n, total = 0, 0.0
        for mod in ("ap", "behavior"):
            w, mask = z[f"{case}/w/{mod}"], z[f"{case}/mask/{mod}"]
            assert int(z[f"{case}/n/{mod}"]) == int(w.sum())
            if "objective" in sw:          # the loss mask is the token mask x the channel mask
                want = np.broadcast_to(mask[:, :, None], w.shape) * (np.broadcast_to(vb, w.shape) if mod == "ap" else 1)
                assert np.array_equal(w, want.astype(np.uint8)), (case, mod)
                assert bool((mask <= z[f"batch/{case}/{mod}/attn"]).all())
            else:                          # input masking: no token is masked, the masker's mask x the channel mask
                assert int(mask.sum()) == 0
                if mod == "ap":
                    assert bool((w[np.broadcast_to(~vb, w.shape)] == 0).all())
            total_n += int(w.sum())
            total += float(z[f"{case}/mod_loss/{mod}"])
        loss = float(z[f"{case}/loss"])
        if total_n == 0:
            nan_cases.append(case)
            assert np.isnan(loss) and bool(np.isnan(z[f"{case}/grad_norm"]).any())
        else:
            assert loss == pytest.approx(total / total_n, rel=1e-6) and bool(np.isfinite(z[f"{case}/grad_norm"]).all())
        assert len(z[f"{case}/grad_norm"]) == len(meta["params"][case])
        assert (f"{case}/grad/{meta['params'][case][0]}" in z.files) == (case in NP.FULL_GRAD)
    assert nan_cases == ["enc_allpad"]
    # a sample with every channel real and one with none; both sides; padded bins with padded channels; a segmented batch; both forms
    assert NP.CASES["enc_right"]["n"] == (12, 7, 0) and NP.CASES["tok_left"]["side"] == "left" and NP.CASES["enc_ragged"]["T"] == (8, 5)
    assert int(z["batch/enc_timepad/ap/attn"].sum()) < 24 and len({c.get("objective") for c in NP.CASES.values()} - {None}) == 3
    # head rows of channels no sample has: exactly zero in the reference too
    g = z["enc_right/grad/decoder_embeddings.ap.out.weight"]
    assert g.shape[0] == 12 and bool(np.isfinite(g).all())
    curve = load_json("neuron_padding_curve.json")
    assert curve["sessions"] == list(NP.CURVE_SESSIONS) and len(curve["loss"]) == curve["total_steps"] == NP.CURVE_STEPS
    assert len(set(curve["sessions"])) == 3 and bool(np.isfinite(curve["loss"]).all()) and set(curve["objective"]) == {"encoding", "decoding", "token_masking"}
    for s in (0, 1, 2):
        batch, v = NP.curve_batch(s)
        assert int(v[0].sum()) == NP.CURVE_SESSIONS[s] and bool((batch["ap"]["inputs"][:, :, NP.CURVE_SESSIONS[s]:] == NP.PAD_VALUE).all())
