"""Per-sample token masking (MMFM_TOKEN_MASK_ROWS, MultiModal.per_sample_mask) without a GPU: the header / binding
surface, the switch in its four layers, EngineConfig and the plan key with the switch off, the entry points' argument checks (they
return before any HIP call) and the torch restatement the kernel tests use as their reference (tests/per_sample_mask.py), proved
against autograd and shown to reject the fault it exists to catch: every sample under sample 0's mask."""
import ctypes as C
import re
from dataclasses import fields

import pytest
import torch

import per_sample_mask as P
from multi_modal_foundation_model_amd import _lib as L

NAMES = {"mmfm_mask_prep_rows", "mmfm_stitch_fwd_rows", "mmfm_stitch_bwd_rows"}


def test_header_macro_prototypes_and_library():
    with open(L.HEADER_PATH) as f:
        src = f.read()
    assert re.search(r"^#define MMFM_TOKEN_MASK_ROWS 1$", src, flags=re.M)
    assert NAMES <= set(L.header_symbols()) and NAMES <= set(L._PROTOS)
    lib = L.lib()
    assert all(hasattr(lib, n) for n in NAMES)
    # the argument lists: the segment forms', with keep_any behind keep / keep_ld and rec behind keep
    seg = L._PROTOS["mmfm_mask_prep_seg"][1]
    assert L._PROTOS["mmfm_mask_prep_rows"][1] == seg[:10] + [C.c_void_p] + seg[10:]
    fs, bs = L._PROTOS["mmfm_stitch_fwd_seg"][1], L._PROTOS["mmfm_stitch_bwd_seg"][1]
    assert L._PROTOS["mmfm_stitch_fwd_rows"][1] == fs[:6] + [C.c_int, C.c_void_p] + fs[6:]
    assert L._PROTOS["mmfm_stitch_bwd_rows"][1] == bs[:5] + [C.c_int, C.c_void_p] + bs[5:]


def test_rows_entry_points_check_their_arguments_before_any_hip_call():
    lib, p = L.lib(), 0x10000
    fwd = lambda dtype, keep_ld, rec, T, Ln, off: lib.mmfm_stitch_fwd_rows(dtype, p, p, p, p, p, keep_ld, rec, p, None, 3, T, Ln, off, 32, 8, None)
    bwd = lambda dtype, keep_ld, rec, T, Ln, off: lib.mmfm_stitch_bwd_rows(dtype, p, None, p, p, keep_ld, rec, L.NO_DROP, p, p, p, 0, 0, 3, T, Ln,
                                                                           off, 32, 8, p, 1 << 30, None)
    for fn in (fwd, bwd):
        for keep_ld in (1, 15, -16):
            assert fn(L.F32, keep_ld, None, 8, 16, 0) != 0 and b"keep_ld" in lib.mmfm_last_error()
        assert fn(L.F32, 16, None, 8, 16, 9) != 0 and b"leaves the sequence" in lib.mmfm_last_error()
        assert fn(L.BF16, 0, None, 8, 16, 9) != 0 and b"leaves the sequence" in lib.mmfm_last_error()
        assert fn(L.F32, 16, p, 8, 16, 8) != 0 and b"needs bf16" in lib.mmfm_last_error()
        assert fn(L.F32, 0, p, 8, 16, 0) != 0 and b"needs bf16" in lib.mmfm_last_error()
    seg = (C.c_int32 * 2)(4, 4)
    two = lambda *v: (C.c_void_p * 2)(*v)
    i64 = (C.c_int64 * 2)(1, 1)
    mp = lib.mmfm_mask_prep_rows
    assert mp(0, 2, seg, two(p, p), i64, two(p, p), i64, p, p, p, p, p, p, None) != 0 and b"bad shape" in lib.mmfm_last_error()
    assert mp(3, L.MAX_SEGMENTS + 1, seg, two(p, p), i64, two(p, p), i64, p, p, p, p, p, p, None) != 0 and b"bad shape" in lib.mmfm_last_error()
    assert mp(3, 2, seg, two(p, p), i64, two(p, p), i64, p, p, p, None, p, p, None) != 0 and b"null pointer" in lib.mmfm_last_error()
    assert mp(3, 2, seg, two(p, None), i64, two(p, p), i64, p, p, p, p, p, p, None) != 0 and b"slot 1" in lib.mmfm_last_error()


# ------------------------------------------------------------------------------------------------- the switch, layer by layer
def test_switch_defaults_off_and_is_a_constructor_keyword():
    from helpers import build_model, tiny_config
    from multi_modal.mm import MultiModal
    assert MultiModal.per_sample_mask is False
    a, b = build_model(tiny_config(), 12, 2, seed=1), build_model(tiny_config(), 12, 2, seed=1, per_sample_mask=True)
    assert a.per_sample_mask is False and b.per_sample_mask is True
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    for bad in (1, "true", None):
        with pytest.raises(ValueError, match="per_sample_mask"):
            build_model(tiny_config(), 12, 2, seed=1, per_sample_mask=bad)


def test_engine_config_carries_the_switch_and_is_todays_without_it():
    from helpers import tiny_config
    from multi_modal_foundation_model_amd.engine import EngineConfig
    mods = [("ap", 12), ("behavior", 2)]
    base = EngineConfig.from_model_config(tiny_config(), mods, per_side=True, embedder_opts=True)
    off = EngineConfig.from_model_config(tiny_config(), mods, per_side=True, embedder_opts=True, per_sample_mask=False)
    on = EngineConfig.from_model_config(tiny_config(), mods, per_side=True, embedder_opts=True, per_sample_mask=True)
    assert base.per_sample_mask is False and off == base and on.per_sample_mask is True and on != base and on == on
    assert "per_sample_mask" not in [f.name for f in fields(EngineConfig)], "the field list is what it was"
    kw = dict(hidden=32, heads=4, inter=64, n_enc=1, n_dec=1, max_F=8, mult=2, n_modality=2, embed_scale=1.0, embed_dropout=0.0, dropout=0.0,
              sep_mask=False, causal_mask=False, mods=mods)
    assert EngineConfig(**kw) == EngineConfig(**kw, per_sample_mask=False) != EngineConfig(**kw, per_sample_mask=True)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="per_sample_mask"):
            EngineConfig(**kw, per_sample_mask=bad)


def test_plan_key_gains_a_marker_and_is_todays_without_the_switch():
    from multi_modal_foundation_model_amd.engine import Engine

    class Cfg:
        context, per_sample_mask = None, False

    class Stub:
        cfg = Cfg()
    pat, elem = (True, False), (((2, 1, 12), (2, 1, 12)), None)
    assert Engine.plan_key(Stub(), 4, 8, True, True) == (4, 8, True, True)
    assert Engine.plan_key(Stub(), 4, (8, 5), True, True, pat) == (4, (8, 5), True, True, pat)
    assert Engine.plan_key(Stub(), 4, 8, False, False, None, elem) == (4, 8, False, False, None, elem)
    Stub.cfg.context = (0, 5)
    assert Engine.plan_key(Stub(), 4, 8, True, True) == (4, 8, True, True, None, None, ("window", -5, 0))
    Stub.cfg.per_sample_mask = True
    assert Engine.plan_key(Stub(), 4, 8, True, True) == (4, 8, True, True, None, None, ("window", -5, 0), ("rows",))
    Stub.cfg.context = None
    assert Engine.plan_key(Stub(), 4, 8, True, True) == (4, 8, True, True, None, None, ("rows",))
    assert Engine.plan_key(Stub(), 4, 8, True, True, pat, elem) == (4, 8, True, True, pat, elem, ("rows",))


def _trainer(**training):
    from helpers import build_model, load_config, tiny_config
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


def test_trainer_key_and_entry_script_flag():
    from helpers import load_config
    assert "per_sample_mask" not in load_config()["training"], "no YAML file carries the key"
    tr, model = _trainer()
    assert tr.per_sample_mask is False and model.per_sample_mask is False
    tr, model = _trainer(per_sample_mask=True)
    assert tr.per_sample_mask is True and model.per_sample_mask is True
    assert _trainer(per_sample_mask=False)[1].per_sample_mask is False
    for bad in (1, "true", "yes", None, 0.0):
        with pytest.raises(ValueError, match="per_sample_mask"):
            _trainer(per_sample_mask=bad)
    import train_multi_modal as tm
    assert tm.build_parser().parse_args([]).per_sample_mask is False
    assert tm.build_parser().parse_args(["--per_sample_mask"]).per_sample_mask is True


# ------------------------------------------------------------------------------------------------- the kernels' reference
B, MAX_F, H = 3, 8, 16
TS = (8, 5, 1)


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    masks = [(torch.rand(B, T, generator=g) > 0.5).long() for T in TS]
    masks[0][:, 3] = 1                                  # one bin masked in every sample
    masks[0][0, :3] = 0
    masks[0][1, :3] = 1                                 # ... and bins masked in some
    attns = [torch.ones(B, T, dtype=torch.int64) for T in TS]
    attns[0][0, 6:] = 0
    attns[1][2, 3:] = 0
    tss = [((torch.arange(T)[None] * (j + 1) + torch.arange(B)[:, None] * 3) % (MAX_F + 2) - 1) for j, T in enumerate(TS)]
    toks = [torch.randn(B * T, H, generator=g, dtype=torch.float64) for T in TS]
    rows = [torch.randn(H, generator=g, dtype=torch.float64) for _ in TS]
    poss = [torch.randn(MAX_F, H, generator=g, dtype=torch.float64) for _ in TS]
    return masks, attns, tss, toks, rows, poss


def test_mask_products_restate_keep_per_sample():
    masks, attns, _, _, _, _ = _inputs()
    chans = [12, 2, 4]
    r = P.mask_products(masks, attns, chans)
    Ln = sum(TS)
    v = torch.cat([m & a for m, a in zip(masks, attns)], 1)
    for b in range(B):
        for l in range(Ln):
            assert int(r["keep"][b, l]) == int(int(v[b, l]) != 1) and int(r["tokmask"][b, l]) == int(int(v[b, l]) != 0)
    for l in range(Ln):
        assert int(r["keep_any"][l]) == int(any(int(r["keep"][b, l]) for b in range(B)))
    assert int(r["keep_any"][3]) == 0 and int(r["keep_any"].sum()) == Ln - 1, "one dead bin: masked in every sample"
    assert r["count"].tolist() == [int((m & a).sum()) * n for m, a, n in zip(masks, attns, chans)]
    assert r["mod_id"].tolist() == [0] * 8 + [1] * 5 + [2]
    # at B = 1 the per-sample row IS sample 0's row: the two modes are one model
    one = P.mask_products([m[:1] for m in masks], [a[:1] for a in attns], chans)
    assert torch.equal(one["keep"], P.mask_products([m[:1] for m in masks], [a[:1] for a in attns], chans, row0=True)["keep"])
    assert torch.equal(one["keep"][0], one["keep_any"])
    # the injected fault differs on this batch
    assert not torch.equal(r["keep"], P.mask_products(masks, attns, chans, row0=True)["keep"])


def test_stitch_references_against_autograd_and_reject_row0():
    masks, attns, tss, toks, rows, poss = _inputs(1)
    keep = P.mask_products(masks, attns, [1, 1, 1])["keep"]
    bad = P.mask_products(masks, attns, [1, 1, 1], row0=True)["keep"]
    off, Ln = [0, 8, 13], sum(TS)
    g = torch.Generator().manual_seed(5)
    dx, dextra = (torch.randn(B, Ln, H, generator=g, dtype=torch.float64) for _ in range(2))
    drop = (torch.rand(B * TS[0], H, generator=g) > 0.2)
    rejected = 0
    for j, T in enumerate(TS):
        tok, row, pos = (t.clone().requires_grad_(True) for t in (toks[j], rows[j], poss[j]))
        idx = tss[j].clamp(0, MAX_F - 1)
        emb = row[None, None, :] + pos[idx]
        x = keep[:, off[j]:off[j] + T, None].double() * tok.view(B, T, H) + emb
        xr, er, mag = P.stitch_fwd(toks[j], rows[j], poss[j], tss[j], keep, off[j], MAX_F)
        torch.testing.assert_close(xr, x.detach(), rtol=0, atol=1e-13)
        torch.testing.assert_close(er, emb.detach(), rtol=0, atol=1e-13)
        assert bool((mag >= x.detach().abs() - 1e-12).all())
        # x takes dx, emb takes dextra as well (the context path): d_tok sees dx alone
        (x * dx[:, off[j]:off[j] + T]).sum().backward(retain_graph=True)
        d_tok = tok.grad.clone()
        (emb * dextra[:, off[j]:off[j] + T]).sum().backward()
        r = P.stitch_bwd(dx, dextra, tss[j], keep, None, 0.0, off[j], MAX_F)
        torch.testing.assert_close(r["d_tok"], d_tok, rtol=0, atol=1e-13)
        torch.testing.assert_close(r["d_mod"], row.grad, rtol=0, atol=1e-12)
        torch.testing.assert_close(r["d_pos"], pos.grad, rtol=0, atol=1e-12)
        assert bool((r["d_tok"].view(B, T, H)[keep[:, off[j]:off[j] + T] == 0] == 0).all())
        if j == 0:      # dropout' = keep / (1 - p) rides on d_tok alone
            rd = P.stitch_bwd(dx, dextra, tss[j], keep, drop, 0.2, off[j], MAX_F)
            torch.testing.assert_close(rd["d_tok"], d_tok * drop.double() / 0.8, rtol=0, atol=1e-13)
            torch.testing.assert_close(rd["d_mod"], r["d_mod"], rtol=0, atol=0)
        # the injected fault: row 0's mask for every sample
        xb = P.stitch_fwd(toks[j], rows[j], poss[j], tss[j], bad, off[j], MAX_F)[0]
        rb = P.stitch_bwd(dx, dextra, tss[j], bad, None, 0.0, off[j], MAX_F)
        if not torch.equal(bad[:, off[j]:off[j] + T], keep[:, off[j]:off[j] + T]):
            assert float((xb - x.detach()).abs().max()) > 1e-3 and float((rb["d_tok"] - d_tok).abs().max()) > 1e-3
            rejected += 1
    assert rejected >= 2


def test_case_table_masks_discriminate():
    """Every explicit case gives sample 0 a keep row that some other sample does not share on at least one side, and names what its
    comment says: S0_OPEN leaves sample 0 unmasked, S0_FULL masks all of it, BIN_ALL masks one bin everywhere."""
    for case in list(P.CASES) + [P.FILTER["case"]]:
        sw = P.switches(case)
        if sw["masks"] is None:
            continue
        md = P.mod_dict(case, "token_masking")
        v = {m: md[m]["eval_mask"][:, :, 0] & md[m]["inputs_attn_mask"] for m in P.MODS}
        assert any(not torch.equal(v[m][b], v[m][0]) for m in P.MODS for b in (1, 2)), case
    v = P.mod_dict("S0_OPEN", "token_masking")
    assert all(int(v[m]["eval_mask"][0].sum()) == 0 and int(v[m]["eval_mask"][1:].sum()) > 0 for m in P.MODS)
    v = P.mod_dict("S0_FULL", "token_masking")
    assert all(bool(v[m]["eval_mask"][0].all()) and not bool(v[m]["eval_mask"][1].all()) for m in P.MODS)
    v = P.mod_dict("BIN_ALL", "token_masking")["ap"]["eval_mask"][:, :, 0]
    assert bool(v[:, 3].all()) and sum(bool(v[:, t].all()) for t in range(8)) == 1
