"""Input masking (mask_type: input with MultiModal.input_masking), host side: Masker.element_masks against Masker.forward - masks,
corrupted spikes, generator and `random` state - the switch on the model, the builders and the trainer, and the header's feature
macro.  No GPU involved."""
import random
import re

import numpy as np
import pytest
import torch

from helpers import build_model, load_config, tiny_config
from test_oracle_golden import default_masker_cfg

B, T, N = 3, 8, 12
REGIONS = np.array([["CA1"] * 5 + ["PO"] * 4 + ["LP"] * 3] * B)
MODES = ["temporal", "random_token", "causal", "neuron", "inter-region", "intra-region", "co-smooth", "forward-pred", "random"]
COMPACT = {"temporal": (B, T, 1), "random_token": (B, T, 1), "causal": (B, T, 1), "neuron": (B, 1, N), "inter-region": (B, 1, N),
           "intra-region": (B, 1, N), "co-smooth": (1, 1, N), "forward-pred": (1, T, 1), "random": (B, T, N)}


def masker(mode, **kw):
    from models.masker import Masker
    from utils.config_utils import DictConfig
    cfg = default_masker_cfg(mode=mode, expand_prob=0.5, max_timespan=3, channels=[1, 4, 7], timesteps=[2, 5], **kw)
    return Masker(DictConfig(cfg))


def spikes():
    return torch.poisson(torch.full((B, T, N), 1.5), generator=torch.Generator().manual_seed(3))


def run(fn, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    out = fn()
    return out, torch.get_rng_state(), random.getstate()


@pytest.mark.parametrize("jump", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_element_masks_are_forwards_masks(mode, jump, monkeypatch):
    monkeypatch.setenv("MMFM_MASKER_JUMP", jump)
    x = spikes()
    for seed in (0, 1, 2, 3):              # (expand_prob 0.5: both time-span branches of the token modes)
        (sp, tmask), g_ref, r_ref = run(lambda: masker(mode)(x.clone(), REGIONS), seed)
        (cm, tm, corrupted), g, r = run(lambda: masker(mode).element_masks(x, REGIONS), seed)
        assert corrupted is None and cm.dtype == tm.dtype == torch.uint8
        assert tuple(cm.shape) == tuple(tm.shape) == COMPACT[mode], (mode, cm.shape, tm.shape)
        assert torch.equal(tm.expand(B, T, N).to(torch.int64), tmask), f"{mode} seed {seed}: target mask"
        assert torch.equal(x * (cm.expand(B, T, N) == 0), sp), f"{mode} seed {seed}: spikes * ~cm"
        assert torch.equal(g, g_ref), f"{mode} seed {seed}: CPU generator state"
        assert r == r_ref, f"{mode} seed {seed}: random.getstate()"
        if mode not in ("intra-region", "causal"):
            assert torch.equal(cm, tm)
    assert torch.equal(x, spikes()), "element_masks must not modify its input"


def test_masks_differ_where_forward_says_so():
    x = spikes()
    (cm, tm, _), _, _ = run(lambda: masker("intra-region").element_masks(x, REGIONS), 0)
    assert bool((cm.int() - tm.int() >= 0).all()) and not torch.equal(cm, tm)
    (cm, tm, _), _, _ = run(lambda: masker("causal", ratio=0.9).element_masks(x, REGIONS), 0)
    assert bool((cm.int() - tm.int() >= 0).all())


@pytest.mark.parametrize("mode", ["temporal", "neuron", "intra-region", "random"])
def test_real_draw_path_is_forwards_corruption(mode):
    x = spikes()
    kw = dict(zero_ratio=0.5, random_ratio=1.0)
    (sp, tmask), g_ref, r_ref = run(lambda: masker(mode, **kw)(x.clone(), REGIONS), 5)
    (cm, tm, corrupted), g, r = run(lambda: masker(mode, **kw).element_masks(x, REGIONS), 5)
    assert corrupted is not None and torch.equal(corrupted, sp), "the corrupted spikes must be forward's bit for bit"
    assert not torch.equal(corrupted, x * (cm.expand(B, T, N) == 0)), "zero_ratio 0.5 must have drawn noise somewhere"
    assert torch.equal(tm.expand(B, T, N).to(torch.int64), tmask) and torch.equal(g, g_ref) and r == r_ref
    assert torch.equal(x, spikes())


def test_inactive_masker_masks_nothing():
    m = masker("temporal", ratio=0)
    before = torch.get_rng_state()
    cm, tm, corrupted = m.element_masks(spikes(), REGIONS)
    assert corrupted is None and tuple(cm.shape) == (1, 1, 1) and int(cm.sum()) == int(tm.sum()) == 0
    assert torch.equal(torch.get_rng_state(), before)


def test_switch_defaults_off_and_is_a_constructor_keyword():
    assert build_model(tiny_config(), 12, 2, seed=1).input_masking is False
    assert build_model(tiny_config(), 12, 2, seed=1, input_masking=True).input_masking is True


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
    with pytest.raises(ValueError, match="mask_type"):
        _trainer(input_masking=True)                      # the YAML's mask_type is embd
    tr, model = _trainer(input_masking=True, mask_type="input", mask_mode=["neuron", "temporal"])
    assert model.input_masking is True and tr.masking_schemes == ["neuron", "temporal"]
    assert _trainer(mask_type="input")[1].input_masking is False
    assert _trainer()[1].input_masking is False


def test_entry_script_flag():
    import train_multi_modal as tm
    assert tm.build_parser().parse_args([]).input_masking is False
    assert tm.build_parser().parse_args(["--input_masking"]).input_masking is True


def test_header_feature_macro_and_exports():
    from multi_modal_foundation_model_amd import _lib as L
    with open(L.HEADER_PATH) as f:
        src = f.read()
    assert re.search(r"^#define MMFM_LOSS_ELEM 1$", src, flags=re.M) and re.search(r"^#define MMFM_VERSION 401$", src, flags=re.M)
    names = {"mmfm_masked_loss_elem_workspace", "mmfm_masked_loss_elem_fwd", "mmfm_masked_loss_elem_bwd", "mmfm_stage_masked"}
    assert names <= set(L.header_symbols()) and names <= set(L._PROTOS)
    assert L.lib().mmfm_version() == 401
    # partials: 1024 floats, then 1024 int64 counts
    assert L.lib().mmfm_masked_loss_elem_workspace(102400, 668) == 1024 * 4 + 1024 * 8
    assert L.lib().mmfm_masked_loss_elem_workspace(15, 3) == 16 + 4 * 8


def test_elem_strides():
    from multi_modal_foundation_model_amd import ops as K
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    assert K.elem_strides(u8(3, 8, 12), 3, 8, 12) == (96, 12, 1)
    assert K.elem_strides(u8(3, 1, 12), 3, 8, 12) == (12, 0, 1)
    assert K.elem_strides(u8(3, 8, 1), 3, 8, 12) == (8, 1, 0)
    assert K.elem_strides(u8(1, 1, 12), 3, 8, 12) == (0, 0, 1)
    assert K.elem_strides(u8(1, 8, 1), 3, 8, 12) == (0, 1, 0)
    assert K.elem_strides(u8(3, 12, 8).transpose(1, 2), 3, 8, 12) == (96, 1, 8)
    for bad in (u8(3, 8), u8(2, 8, 12), torch.zeros(3, 8, 12, dtype=torch.bool)):
        with pytest.raises(ValueError):
            K.elem_strides(bad, 3, 8, 12)
