"""decoder.decoder_causal_mask / decoder.decoder_sep_mask through the whole model on the MI355X, at a size whose decoder self-attention
runs on the dh = 32 fast kernels (csrc/attention_fast.hip): H = 256, 8 heads, L = 200 (tests/golden/decoder_mask_scalars.json,
produced from the reference by scripts/make_decoder_mask_goldens.py)."""
import math

import pytest
import torch

from conftest import load_json
from helpers import build_model, make_optimizer, model_config
from model_checks import cosine, to_dev
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

CASES = ["causal", "sep", "causal_sep"]


def fixture_model(meta, case, dtype="fp32", dropout=0.0):
    mc = model_config(H=meta["H"], heads=meta["heads"], inter=meta["inter"], n_enc=meta["n_enc"], n_dec=meta["n_dec"], max_F=meta["max_F"],
                      dropout=dropout, emb_dropout=0.0, **meta["cases"][case])
    model = build_model(mc, meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    model.compute_dtype = dtype
    return model.cuda()


def synth_fixture_batch(meta):
    return O.synth_batch(meta["B"], meta["T"], meta["n_ap"], meta["n_beh"], seed=meta["data_seed"], pad=meta["pad"])


@pytest.mark.parametrize("case", CASES)
def test_fp32_scalars_vs_reference_fixture(case):
    """fp32 parity mode against the reference's own forward / backward: the project's fp32 tolerances, integer n exact."""
    g = load_json("decoder_mask_scalars.json")
    meta = g["meta"]
    model = fixture_model(meta, case).eval()
    batch = synth_fixture_batch(meta)
    for obj in ("encoding", "decoding", "token_masking"):
        c = g["cases"][case][obj]
        model.zero_grad(set_to_none=True)
        torch.manual_seed(meta["mask_seed"])
        out = model(to_dev(O.make_mod_dict(batch, obj)))
        out.loss.backward()
        assert out.loss.item() == pytest.approx(c["loss"], rel=1e-5)
        for m in ("ap", "behavior"):
            assert int(out.mod_n_examples[m]) == c["n"][m]
            assert float(out.mod_preds[m].double().abs().sum()) == pytest.approx(c["pred_abssum"][m], rel=1e-4)
        for k, prm in model.named_parameters():
            assert float(prm.grad.double().norm()) == pytest.approx(c["grad_norm"][k], rel=5e-3, abs=1e-8), k


@pytest.mark.parametrize("case", CASES)
def test_bf16_tracks_fixture_and_fp32_engine(case):
    """bf16 storage / fp32 accumulate (decoder self-attention on the fast kernels with CAUSAL / SEP) vs the fp32 reference numbers and
    the fp32 engine in-process: 2e-2 on the loss, gradient direction cosine >= 0.99 per large tensor (bf16 has 8 significant bits)."""
    g = load_json("decoder_mask_scalars.json")
    meta = g["meta"]
    model, ref = fixture_model(meta, case, "bf16").eval(), fixture_model(meta, case).eval()
    batch = synth_fixture_batch(meta)
    for obj in ("encoding", "decoding"):
        c = g["cases"][case][obj]
        for m in (model, ref):
            m.zero_grad(set_to_none=True)
        out = model(to_dev(O.make_mod_dict(batch, obj)))
        out.loss.backward()
        out32 = ref(to_dev(O.make_mod_dict(batch, obj)))
        out32.loss.backward()
        assert out.loss.item() == pytest.approx(c["loss"], rel=2e-2)
        assert out.loss.item() == pytest.approx(out32.loss.item(), rel=2e-2)
        for mname in ("ap", "behavior"):
            assert int(out.mod_n_examples[mname]) == c["n"][mname]
        p16, p32 = dict(model.named_parameters()), dict(ref.named_parameters())
        for k in p32:
            if p32[k].grad.abs().max() > 0 and p32[k].numel() >= 4096:
                cs = cosine(p16[k].grad, p32[k].grad)
                assert cs > 0.99, f"{obj} {k}: cosine {cs}"


@pytest.mark.parametrize("case", CASES)
def test_bf16_training_step_draws_keep_bits_for_decoder_self_attention(case):
    """Training mode, bf16, transformer dropout 0.4: the decoder self-attention sites carry a keep-bit buffer, and with CAUSAL / SEP the
    forward must fill it (only the fast kernels' generator writes it: on the general kernels it stays as it was)."""
    meta = load_json("decoder_mask_scalars.json")["meta"]
    model = fixture_model(meta, case, "bf16", dropout=0.4).train()
    opt, sch = make_optimizer(model, 10)
    batch = synth_fixture_batch(meta)

    def step():
        torch.manual_seed(meta["mask_seed"])
        out = model(to_dev(O.make_mod_dict(batch, "encoding")))
        out.loss.backward()
        opt.step(); sch.step(); opt.zero_grad()
        return out.loss.item()

    step()                                                       # the plan and its buffers exist
    L = 2 * meta["T"]
    tiles = meta["B"] * meta["heads"] * ((L + 31) // 32) ** 2 * 128          # the bit tiles lie in front of the buffer (include/mmfm.h)
    keep = model._engine.b["dec0/sa/keep"][:tiles]
    keep.zero_()
    torch.cuda.synchronize()
    loss = step()
    torch.cuda.synchronize()
    assert math.isfinite(loss)
    assert bool((keep != 0).any()), "the decoder self-attention forward left its keep-bit buffer untouched"
