"""Live rows through the whole model: one bf16 training step with MMFM_LIVE_ROWS=1 against the same step with
MMFM_LIVE_ROWS=0, tiny model (1 + 1 layers, H = 32), B = 4, T = 12, dropout on.  `encoding` (every `ap` bin dead, every `behavior` bin
live) and `decoding` (the reverse): everything bit for bit, the updated parameters included - zeros were being summed.  `token_masking`
(some bins dead): loss, predictions, every forward buffer and the gradients that do not pass through a tokeniser's dY^T.X bit for bit;
the tokenisers' weight gradients sum the same terms in other groups, so gradients and updated parameters are compared at the bounds
model_checks.check_bf16 sets for a bf16 step against its oracle.  One case runs a modal_filter model whose two sides carry different
masks, hence different records."""
import pytest
import torch

import model_checks as MC
from helpers import build_model, make_optimizer, tiny_config
from modal_filter import case_model
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu
B, T, N_AP, N_BEH = 4, 12, 12, 2
# what the compact row space changes the layout of (the tokeniser's own buffers), and scratch
# (the attention keep-bit workspaces are allocated per site but written by the dh-32 / dh-64 kernels only: at this model's dh = 8 they
# hold whatever the allocator left)
SKIP = ("d/", "ws/", "tok_tmp", "encoder/a/", "decoder/a/", "encoder/z/", "decoder/z/", "live", "dec/live", "in_live/", "dec/in_live/")


def step(monkeypatch, live, objective, case=None, mask_seed=5):
    monkeypatch.setenv("MMFM_LIVE_ROWS", live)
    kw = dict(dropout=0.2, emb_dropout=0.1)
    model = case_model(case, N_AP, N_BEH, seed=7, **kw) if case else build_model(tiny_config(**kw), N_AP, N_BEH, seed=7)
    model.compute_dtype, model.engine_seed = "bf16", 77
    model.cuda().train()
    opt, _ = make_optimizer(model, 40, lr=1e-3)
    torch.manual_seed(mask_seed)
    md = MC.to_dev(O.make_mod_dict(O.synth_batch(B, T, N_AP, N_BEH, seed=3, pad=[0, 0, 2, 0]), objective))
    out = model(md)
    out.loss.backward()
    torch.cuda.synchronize()
    plan = model._engine._last
    names = [fn.__name__ for fn, _, _ in plan["fwd"]]
    assert ("mmfm_gemm_live" in names) == ("mmfm_live_bins" in names) == (live == "1")
    bufs = {k: v.clone() for k, v in plan["b"].items() if not k.startswith(SKIP) and not k.endswith("/keep")}
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    masked0 = {m: int(md[m]["inputs_mask"][0].cpu().sum()) for m in md}          # sample 0's masked bins, counted on the CPU
    return dict(out=out, bufs=bufs, grads=grads, params=params, masked0=masked0, keys=set(plan["b"]))


def same_forward(on, off):
    assert on["out"].loss.item() == off["out"].loss.item()
    for m in off["out"].mod_preds:
        assert torch.equal(on["out"].mod_preds[m], off["out"].mod_preds[m]), m
    assert set(on["bufs"]) == set(off["bufs"]) and any(k.startswith("x_enc") for k in on["bufs"]) and "context" in on["bufs"]
    bad = [k for k, v in off["bufs"].items() if not torch.equal(on["bufs"][k].view(torch.uint8), v.view(torch.uint8))]
    assert not bad, f"forward buffers that differ: {bad}"


@pytest.mark.parametrize("objective", ["encoding", "decoding"])
def test_all_dead_and_all_live_modalities_are_bit_identical(monkeypatch, objective):
    on, off = step(monkeypatch, "1", objective), step(monkeypatch, "0", objective)
    dead = "ap" if objective == "encoding" else "behavior"
    assert on["masked0"] == {dead: T, "behavior" if dead == "ap" else "ap": 0}
    same_forward(on, off)
    for k in off["params"]:
        assert torch.equal(on["grads"][k], off["grads"][k]), f"gradient {k}"
        assert torch.equal(on["params"][k], off["params"][k]), f"updated parameter {k}"
    # the dead modality's tokeniser linears: gradients exactly +0 on both sides
    for side in ("encoder", "decoder"):
        for lin in ("token_embed", "projection"):
            for wb in ("weight", "bias"):
                g = on["grads"][f"{side}_embeddings.{dead}.embedder.{lin}.{wb}"]
                assert not g.any() and not torch.signbit(g).any()


@pytest.mark.parametrize("case", [None, "DEC"])
def test_some_bins_dead_token_masking(monkeypatch, case):
    """case None: both modalities on both sides, one mask set.  DEC: the encoder over `ap`, the decoder over `behavior` - two mask sets,
    two records.  Masker seed 5: sample 0 has between 1 and T - 1 masked bins in every modality (asserted)."""
    on, off = step(monkeypatch, "1", "token_masking", case), step(monkeypatch, "0", "token_masking", case)
    assert on["masked0"] == off["masked0"] and all(0 < n < T for n in on["masked0"].values()), on["masked0"]
    assert ("dec/live" in on["keys"]) == (case == "DEC") and "live" in on["keys"] and "live" not in off["keys"]
    same_forward(on, off)
    regrouped = (".embedder.token_embed.", ".embedder.projection.")
    for k in off["grads"]:
        if not any(r in k for r in regrouped):
            assert torch.equal(on["grads"][k], off["grads"][k]), f"gradient {k}"
    ref = dict(loss=off["out"].loss.double())
    MC.check_bf16(MC.bf16_stats(on["out"], on["grads"], ref, {k: v.double() for k, v in off["grads"].items()}), "live vs full rows: gradients")
    MC.check_bf16(MC.bf16_stats(on["out"], on["params"], ref, {k: v.double() for k, v in off["params"].items()}), "live vs full rows: updated parameters")


@pytest.mark.parametrize("objective", ["encoding", "decoding"])
def test_forward_only_plan_is_bit_identical(monkeypatch, objective):
    """Evaluation under no_grad builds the forward-only plan from the same forward code: the same path, the same bits."""
    res = {}
    for live in ("1", "0"):
        monkeypatch.setenv("MMFM_LIVE_ROWS", live)
        model = build_model(tiny_config(), N_AP, N_BEH, seed=7)
        model.compute_dtype = "bf16"
        model.cuda().eval()
        md = MC.to_dev(O.make_mod_dict(O.synth_batch(B, T, N_AP, N_BEH, seed=3, pad=[0, 0, 2, 0]), objective))
        with torch.no_grad():
            out = model(md)
        torch.cuda.synchronize()
        eng = model._engine
        assert (B, T, False, False) in eng.plans and eng._last["bwd"] is None
        assert ("mmfm_gemm_live" in [fn.__name__ for fn, _, _ in eng._last["fwd"]]) == (live == "1")
        res[live] = out
    assert res["1"].loss.item() == res["0"].loss.item()
    for m in res["0"].mod_preds:
        assert torch.equal(res["1"].mod_preds[m], res["0"].mod_preds[m]), m
