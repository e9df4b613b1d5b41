"""decoder.decoder_causal_mask / decoder.decoder_sep_mask through the whole model at dh = 64 (H = 128, 2 heads, three modalities,
L = 120): in bf16 training with dropout the decoder self-attention sites run on the keep-bit pair of csrc/attention_long.hip, whose
generator is the only writer of the sites' keep-bit buffers."""
import math

import pytest
import torch

from helpers import build_model_mods, make_optimizer, model_config
from model_checks import to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

MODS = [("ap", 24), ("behavior", 2), ("lfp", 8)]
B, T = 4, 40
CASES = {"causal": dict(causal=True), "sep": dict(sep=True), "causal_sep": dict(causal=True, sep=True)}


def make(**kw):
    model = build_model_mods(model_config(H=128, heads=2, inter=256, n_enc=1, n_dec=1, max_F=T, n_modality=3, dropout=0.2, **kw), MODS, seed=7)
    model.loss_mod["lfp"] = "mse"
    model.compute_dtype = "bf16"
    return model.cuda()


def batch():
    return O.synth_batch_mods(B, T, MODS, seed=3, pad=[0, 5, 0, 11])


def plan_calls(model):
    plan = model._engine._last
    return len(plan["fwd"]), sum(len(seg) for _, seg in plan["bwd"])


@pytest.fixture(scope="module")
def dense_calls():
    model = make().train()
    out = model(to_dev(O.make_mod_dict_mods(batch(), MODS, "ap")))
    out.loss.backward()
    torch.cuda.synchronize()
    return plan_calls(model)


@pytest.mark.parametrize("case", list(CASES))
def test_bf16_training_steps_draw_keep_bits_at_dh64(case, dense_calls):
    """Two training steps: loss and every gradient finite, the plan has the dense model's call counts, and the decoder self-attention
    forward filled its (zeroed) keep-bit buffer - on the general kernels, which hash, it stays as it was."""
    model = make(**CASES[case]).train()
    opt, sch = make_optimizer(model, 10)
    data = batch()

    def fwd_bwd():
        torch.manual_seed(11)
        out = model(to_dev(O.make_mod_dict_mods(data, MODS, "ap")))
        out.loss.backward()
        return out.loss.item()

    fwd_bwd()                                                    # the plan and its buffers exist
    opt.step(); sch.step(); opt.zero_grad()
    keeps = {k: v for k, v in model._engine.b.items() if k.endswith("/sa/keep")}
    dec = [k for k in keeps if k.startswith("dec")]
    assert dec, sorted(model._engine.b)
    L = len(MODS) * T
    tiles = B * 2 * ((L + 31) // 32) ** 2 * 128                  # the bit tiles lie in front of the buffer (include/mmfm.h)
    for v in keeps.values():
        v.zero_()
    torch.cuda.synchronize()
    for _ in range(2):
        loss = fwd_bwd()
        assert math.isfinite(loss)
        for k, prm in model.named_parameters():
            assert prm.grad is None or bool(torch.isfinite(prm.grad).all()), k
        opt.step(); sch.step(); opt.zero_grad()
    torch.cuda.synchronize()
    for k in dec:
        assert bool((keeps[k][:tiles] != 0).any()), f"{k}: the decoder self-attention forward left its keep-bit buffer untouched"
    assert plan_calls(model) == dense_calls


@pytest.mark.parametrize("case", list(CASES))
def test_bf16_eval_forward_without_workspace_is_finite(case):
    """Eval mode carries no keep-bit workspace: the general kernels run, as before."""
    model = make(**CASES[case]).eval()
    out = model(to_dev(O.make_mod_dict_mods(batch(), MODS, "ap")))
    assert math.isfinite(out.loss.item())
    for m, _ in MODS:
        assert bool(torch.isfinite(out.mod_preds[m].float()).all()), m
