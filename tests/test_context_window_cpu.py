"""The attention window over time stamps without a GPU: the (context.forward, context.backward) -> (lo, hi) translation against upstream's
create_context_mask, the brute-force allowed(b, q, k) of tests/context_window_refs.py, the header / binding surface (MMFM_ATTN_WINDOW, the
descriptor untouched, MMFM_VERSION 401) and mmfm_attn_win_family, which makes no HIP call."""
import ctypes as C
import re

import pytest
import torch

import attn_refs as AR
import attn_route_grid as G
import context_window_refs as CW
import dropout_refs as DR
from multi_modal_foundation_model_amd import _lib as L, ops
from multi_modal.mm_utils import create_context_mask


def test_translation_matches_create_context_mask():
    """(lo <= j - i <= hi) == create_context_mask(F, Bk, N)[i][j] over N in {1, 2, 4, 5, 33, 100} and F, Bk in {-1, 0, 1, 2, 5, N - 1, N, N + 3}:
    384 cases, the quirk `backward: 0` = unbounded among them; ops.context_window is the same translation."""
    n = 0
    for N in CW.GRID_N:
        idx = torch.arange(N)
        d = idx[None, :] - idx[:, None]                     # [i][j] = j - i
        for F in CW.grid_values(N):
            for Bk in CW.grid_values(N):
                lo, hi = CW.translate(F, Bk)
                assert ops.context_window(F, Bk) == (lo, hi)
                want = create_context_mask(F, Bk, N).bool()
                assert torch.equal((d >= lo) & (d <= hi), want), (N, F, Bk)
                assert torch.equal(CW.band(lo, hi, idx[None])[0], want)
                n += 1
    assert n == 384
    assert CW.translate(5, 0) == (-CW.INF, 5) and CW.translate(0, -1) == (-CW.INF, 0) and CW.translate(-1, 3) == (-3, CW.INF)
    assert (L.ATTN_WINDOW_INF, L.ATTN_POS_CLAMP) == (CW.INF, CW.POS_CLAMP) == (1 << 30, 1 << 29)


@pytest.mark.parametrize("bad", [(-2, 0), (0, -2), (1.0, 0), (0, "3"), (True, 0), (None, -1)])
def test_context_window_refuses_what_is_not_an_int_from_minus_one(bad):
    with pytest.raises(ValueError, match=r"context\.(forward|backward) must be an int >= -1"):
        ops.context_window(*bad)


def test_window_allowed_brute_force_on_the_library_s_translation():
    """window_allowed element by element against three nested loops, on stamps that are neither sorted nor unique, and its refusal of an
    empty row - for the windows of the kernel tests and for the intervals ops.context_window makes of config values, clamped as
    ops.attn_window clamps them."""
    Bn, Ln = 3, 41
    windows = list(CW.WINDOWS) + [(f"cfg{F}_{Bk}", 1) + ops.context_window(F, Bk) for F, Bk in ((0, -1), (2, 0), (-1, 3), (1, 1))]
    w = ops.attn_window(torch.zeros(1, 1, dtype=torch.int32), -(1 << 31) + 1, (1 << 31) - 1)
    assert (w.lo, w.hi) == (-CW.INF, CW.INF)
    kp = AR.keypad(Bn, Ln, "tile_start")
    for rec in CW.STAMP_RECIPES:
        pos = CW.clamp_pos(CW.stamps(rec, Bn, Ln))
        for name, flags, lo, hi in windows:
            want = torch.zeros(Bn, Ln, Ln, dtype=torch.bool)
            for b in range(Bn):
                for q in range(Ln):
                    for k in range(Ln):
                        dlt = int(pos[b, k]) - int(pos[b, q])
                        want[b, q, k] = bool((flags & 1) and q == k) or (bool(kp[b, k]) and lo <= dlt <= hi)
            if not bool(want.any(-1).all()):
                with pytest.raises(AssertionError, match="without an allowed key"):
                    CW.window_allowed(kp, flags, pos, lo, hi)
                continue
            assert torch.equal(CW.window_allowed(kp, flags, pos, lo, hi), want), (rec, name)
    # the all-covering window is the dense rule, on any stamps
    assert torch.equal(CW.window_allowed(kp, 1, pos, -CW.INF, CW.INF), DR.allowed_mask(kp, 1, Ln))
    with pytest.raises(AssertionError):
        CW.window_allowed(kp, 2, pos, -1, 1)


def test_stamp_recipes_are_what_pos_prep_takes():
    """Every recipe is a contiguous int64 [B, L] tensor that ops.attn_pos_prep accepts up to the launch (its own argument checks pass;
    without a GPU the call then fails in the library, on CPU tensors, not in the wrapper), and the clamp constants are the library's."""
    for rec in CW.STAMP_RECIPES:
        for Ln in (40, 72, 200, 224):
            p = CW.stamps(rec, 3, Ln)
            assert p.shape == (3, Ln) and p.dtype == torch.int64 and p.is_contiguous()
            with pytest.raises(TypeError, match="pos must be"):           # the stamps pass the wrapper's checks, the short pos does not
                ops.attn_pos_prep(3, [Ln], [p], torch.zeros(3, Ln - 1, dtype=torch.int32))
    assert CW.POS_CLAMP == L.ATTN_POS_CLAMP and CW.INF == L.ATTN_WINDOW_INF
    assert CW.stamps("two_mod", 2, 40)[0].tolist() == list(range(20)) * 2
    assert CW.stamps("two_mod", 2, 200)[1].tolist() == list(range(100)) * 2
    assert CW.stamps("shift7", 3, 8)[2].tolist() == list(range(14, 22))
    sh = CW.stamps("shuffled", 2, 72)
    assert sorted(sh[0].tolist()) == list(range(72)) and bool((sh[0, :32].diff() < 0).any()) and not torch.equal(sh[0], sh[1])
    huge = CW.stamps("huge", 3, 40)
    assert int(huge.abs().max()) > CW.POS_CLAMP and int(CW.clamp_pos(huge).abs().max()) == CW.POS_CLAMP


def test_header_macro_prototypes_and_untouched_descriptor():
    with open(L.HEADER_PATH) as f:
        src = f.read()
    assert re.search(r"^#define MMFM_ATTN_WINDOW 1$", src, flags=re.M) and re.search(r"^#define MMFM_VERSION 401$", src, flags=re.M)
    assert re.search(r"typedef struct \{ const int32_t\* pos; /\*.*?\*/ int lo, hi; \} mmfm_attn_window;", src)
    names = {"mmfm_attn_win_fwd", "mmfm_attn_win_bwd", "mmfm_attn_win_family", "mmfm_attn_pos_prep"}
    assert names <= set(L.header_symbols()) and names <= set(L._PROTOS)
    lib = L.lib()
    assert all(hasattr(lib, n) for n in names) and lib.mmfm_version() == 401
    assert [n for n, _ in L.AttnDesc._fields_] == ["dtype", "B", "heads", "Lq", "Lk", "dh", "q", "k", "v", "ldq", "ldk", "ldv", "o", "ldo", "lse", "keypad",
                                                  "mod_id", "flags", "scale", "drop_p", "drop_o", "d_o", "lddo", "dq", "dk", "dv", "lddq", "lddk",
                                                  "lddv", "keepbits"]
    assert [(n, t) for n, t in L.AttnWindow._fields_] == [("pos", C.c_void_p), ("lo", C.c_int), ("hi", C.c_int)]
    assert C.sizeof(L.AttnWindow) == 16


def _win(lo=-3, hi=3, pos=0x7770000):
    return L.AttnWindow(pos, lo, hi)


def test_win_family_without_a_gpu():
    """dh 32 with a keep-bit workspace (or without dropout) stays on the keep-bit dh-32 kernels, which have window forms; dh 64 / 128 with
    a workspace run BF16 / BF16_TILED (attention_long.hip has none); fp32 runs F32 / F32_TILED.  Forward and backward name the same
    family; NULL window = mmfm_attn_family."""
    M = L.ATTN_FAMILY_MASK
    both = lambda d, w: (ops.attn_win_family(d, w, False), ops.attn_win_family(d, w, True) & M)
    for dh, ws, drop, want_dense in ((32, True, 0.4, L.ATTN_FAMILY_KEEPBIT_DH32), (32, False, 0.0, L.ATTN_FAMILY_KEEPBIT_DH32),
                                     (64, True, 0.4, L.ATTN_FAMILY_KEEPBIT_LONG), (64, True, 0.0, L.ATTN_FAMILY_KEEPBIT_LONG)):
        d = G.desc(ops, L, L.BF16, dh, 200, 200, 1, workspace=ws, drop_p=drop)
        assert both(d, None) == (want_dense, want_dense) == (ops.attn_family(d), ops.attn_family(d, True) & M)
        want = L.ATTN_FAMILY_KEEPBIT_DH32 if dh == 32 else L.ATTN_FAMILY_BF16
        assert both(d, _win()) == (want, want)
    # dh 32 where the keep-bit kernels do not take the shape or lack the workspace dropout needs: the general bf16 kernels
    for d in (G.desc(ops, L, L.BF16, 32, 204, 204, 1, workspace=True, drop_p=0.4), G.desc(ops, L, L.BF16, 32, 200, 200, 1, drop_p=0.4),
              G.desc(ops, L, L.BF16, 32, 264, 264, 1, workspace=True)):
        assert both(d, _win()) == (L.ATTN_FAMILY_BF16, L.ATTN_FAMILY_BF16)
    d = G.desc(ops, L, L.BF16, 128, 200, 200, 0, workspace=True)
    assert both(d, _win()) == (L.ATTN_FAMILY_BF16_TILED, L.ATTN_FAMILY_BF16_TILED)
    d = G.desc(ops, L, L.BF16, 64, 1000, 1000, 0, workspace=True)
    assert both(d, _win()) == (L.ATTN_FAMILY_BF16_TILED, L.ATTN_FAMILY_BF16_TILED)
    d = G.desc(ops, L, L.F32, 32, 200, 200, 1)
    assert both(d, _win()) == (L.ATTN_FAMILY_F32, L.ATTN_FAMILY_F32)
    d = G.desc(ops, L, L.F32, 64, 600, 600, 0)
    assert both(d, _win()) == (L.ATTN_FAMILY_F32_TILED, L.ATTN_FAMILY_F32_TILED)


def test_pos_row_counts_in_the_lds_formulas():
    """The 4 bytes per position can only move a shape towards the tiled kernels, never the other way, and do so for both directions."""
    M = L.ATTN_FAMILY_MASK
    for dt, dh, tiled, resident in ((L.F32, 32, L.ATTN_FAMILY_F32_TILED, L.ATTN_FAMILY_F32), (L.BF16, 64, L.ATTN_FAMILY_BF16_TILED, L.ATTN_FAMILY_BF16)):
        for Ln in range(8, 1200, 8):
            d = G.desc(ops, L, dt, dh, Ln, Ln, 0)
            dense, win = ops.attn_family(d), ops.attn_win_family(d, _win())
            assert win == ops.attn_win_family(d, _win(), True) & M
            assert win in (tiled, resident) and (dense == win or (dense, win) == (resident, tiled)), (dt, dh, Ln, dense, win)


@pytest.mark.parametrize("backward", [False, True])
def test_win_family_refusals(backward):
    cases = [(G.desc(ops, L, L.BF16, 32, 200, 200, 2), _win(), "CAUSAL / SEP are not built under a window"),
             (G.desc(ops, L, L.F32, 32, 200, 200, 5), _win(), "CAUSAL / SEP are not built under a window"),
             (G.desc(ops, L, L.BF16, 32, 72, 40, 0), _win(), "a window needs Lq == Lk"),
             (G.desc(ops, L, L.F32, 32, 40, 40, 0), _win(pos=None), "window without pos")]
    for d, w, msg in cases:
        assert L.lib().mmfm_attn_win_family(C.byref(d), C.byref(w), int(backward)) < 0
        with pytest.raises(L.MmfmError, match=msg):
            ops.attn_win_family(d, w, backward)
    assert ops.attn_win_family(G.desc(ops, L, L.BF16, 32, 200, 200, 2), None, backward) & L.ATTN_FAMILY_MASK == L.ATTN_FAMILY_KEEPBIT_DH32


def test_pos_prep_checks_its_arguments_before_any_hip_call():
    seg = (C.c_int32 * 2)(4, 4)
    ts = (C.c_void_p * 2)(0x10000, 0x20000)
    fn = L.lib().mmfm_attn_pos_prep
    assert fn(0, 2, seg, ts, 0x30000, None) != 0 and b"bad shape" in L.lib().mmfm_last_error()
    assert fn(2, L.MAX_SEGMENTS + 1, seg, ts, 0x30000, None) != 0 and b"bad shape" in L.lib().mmfm_last_error()
    assert fn(2, 2, seg, ts, None, None) != 0 and b"null pointer" in L.lib().mmfm_last_error()
    assert fn(2, 2, seg, (C.c_void_p * 2)(0x10000, None), 0x30000, None) != 0 and b"slot 1" in L.lib().mmfm_last_error()
    assert fn(2, 2, (C.c_int32 * 2)(4, 0), ts, 0x30000, None) != 0 and b"slot 1" in L.lib().mmfm_last_error()
    with pytest.raises(TypeError):
        ops.attn_pos_prep(2, [4], [torch.zeros(2, 4, dtype=torch.int32)], torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.attn_pos_prep(2, [4], [torch.zeros(2, 4, dtype=torch.int64)], torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.attn_window(torch.zeros(2, 4, dtype=torch.int64), -1, 1)


# ------------------------------------------------------------------------------------------------- the switch and the config
def _cfg(forward, backward):
    from helpers import tiny_config
    cfg = tiny_config()
    cfg["context"]["forward"], cfg["context"]["backward"] = forward, backward
    return cfg


def test_switch_defaults_off_and_is_a_constructor_keyword():
    from helpers import build_model, tiny_config
    from multi_modal.mm import MultiModal
    assert MultiModal.context_mask is False
    assert build_model(tiny_config(), 12, 2, seed=1).context_mask is False
    assert build_model(tiny_config(), 12, 2, seed=1, context_mask=True).context_mask is True
    a, b = build_model(_cfg(0, 5), 12, 2, seed=1), build_model(_cfg(0, 5), 12, 2, seed=1, context_mask=True)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert a._context() is None and b._context() == (0, 5)
    assert build_model(tiny_config(), 12, 2, seed=1, context_mask=True)._context() is None, "(-1, -1) under the switch is no window"


def test_engine_config_reads_the_window_only_under_the_keyword():
    from helpers import tiny_config
    from multi_modal_foundation_model_amd.engine import EngineConfig
    mods = [("ap", 12), ("behavior", 2)]
    base = EngineConfig.from_model_config(tiny_config(), mods, per_side=True, embedder_opts=True)
    assert base.context is None
    # switch off: any context.* value is today's config, values nobody could honour included
    for F, Bk in ((0, 5), (0, -1), (-7, "x"), (None, 2.5)):
        assert EngineConfig.from_model_config(_cfg(F, Bk), mods, per_side=True, embedder_opts=True) == base
    # switch on: (-1, -1) is today's config; a window is another config; backward 0 is kept as written (it reads as unbounded)
    on = lambda F, Bk: EngineConfig.from_model_config(_cfg(F, Bk), mods, per_side=True, embedder_opts=True, context_window=True)
    assert on(-1, -1) == base and on(-1, -1).context is None
    assert on(0, 5).context == (0, 5) and on(0, 5) != base and on(0, 5) == on(0, 5) and on(0, 5) != on(0, 4)
    assert on(2, 0).context == (2, 0) and ops.context_window(2, 0) == (-CW.INF, 2)
    for F, Bk in ((-2, 0), (0, -2), (1.5, 0), (0, "3"), (True, 0), (None, -1)):
        with pytest.raises(ValueError, match=r"context\.(forward|backward) must be an int >= -1"):
            on(F, Bk)
    from dataclasses import fields
    assert "context" not in [f.name for f in fields(EngineConfig)], "the field list is what it was"


def test_plan_key_carries_the_window_and_is_todays_without_one():
    from multi_modal_foundation_model_amd.engine import Engine

    class Cfg:
        context = None

    class Stub:
        cfg = Cfg()
    pat, elem = (True, False), (((2, 1, 12), (2, 1, 12)), None)
    assert Engine.plan_key(Stub(), 4, 8, True, True) == (4, 8, True, True)
    assert Engine.plan_key(Stub(), 4, (8, 5), True, True, pat) == (4, (8, 5), True, True, pat)
    assert Engine.plan_key(Stub(), 4, 8, False, False, None, elem) == (4, 8, False, False, None, elem)
    Stub.cfg.context = (0, 5)
    assert Engine.plan_key(Stub(), 4, 8, True, True) == (4, 8, True, True, None, None, ("window", -5, 0))
    assert Engine.plan_key(Stub(), 4, 8, True, True)[-1] == ("window",) + CW.translate(0, 5)
    assert Engine.plan_key(Stub(), 4, 8, True, True, pat, elem)[:6] == (4, 8, True, True, pat, elem)


def _trainer(model_cfg=None, **training):
    from helpers import build_model, load_config, tiny_config
    from trainer.make import make_multimodal_trainer

    class Acc:
        device = torch.device("cpu")
    cfg = load_config()
    for k, v in training.items():
        cfg["training"][k] = v
    model = build_model(model_cfg or tiny_config(), 12, 2, seed=1)
    tr = make_multimodal_trainer(model=model, train_dataloader=[], eval_dataloader=[], optimizer=None, log_dir="/tmp", accelerator=Acc(),
                                 lr_scheduler=None, avail_mod=["ap", "behavior"], config=cfg,
                                 modal_filter=dict(input=["ap", "behavior"], output=["ap", "behavior"]), mixed_training=False, num_neurons=[12])
    return tr, model


def test_trainer_key_and_entry_script_flag():
    from helpers import load_config
    assert "context_mask" not in load_config()["training"], "no YAML file carries the key"
    tr, model = _trainer()
    assert tr.context_mask is False and model.context_mask is False
    tr, model = _trainer(_cfg(0, 20), context_mask=True)
    assert tr.context_mask is True and model.context_mask is True and model._context() == (0, 20)
    assert _trainer(context_mask=False)[1].context_mask is False
    for bad in (1, "true", "yes", None, 0.0):
        with pytest.raises(ValueError, match="context_mask"):
            _trainer(context_mask=bad)
    # switch on: a value that is not an int >= -1 is refused when the config is read; switch off: nobody looks
    with pytest.raises(ValueError, match=r"context\.backward must be an int >= -1"):
        _trainer(_cfg(0, -3), context_mask=True)
    assert _trainer(_cfg(0, -3))[1]._context() is None
    import train_multi_modal as tm
    assert tm.build_parser().parse_args([]).context_mask is False
    assert tm.build_parser().parse_args(["--context_mask"]).context_mask is True
