"""The large-batch regime of the step plan (tests/large_regime.py), on the MI355X: B_BIG = 343 is the smallest batch of the
default shapes on the benchmark's side of every size gate - fused mask 15, weight-gradient pairing with every pair in one launch, grouped
context side, live rows, 256-wide streaming dW tiles on the tokenisers too, column blocks off, a second row pass in every row-owner
kernel - and at that size

  * the plan's regime record is the one of the benchmark's batch of 1024 (plans only, no step);
  * one training step (2 + 2 layers, default widths, dropout 0.4 / 0.2, padded trials, one of them in the last, ragged 128-row pass,
    no MMFM_* switch set) meets the fp64 oracle fed the step's own token masks and dropout multipliers: in bf16 per objective at the
    bounds of model_checks.check_bf16, in fp32 (`token_masking`) element-wise at the bounds of
    test_fp32_dropout_step_vs_oracle_fed_the_steps_masks;
  * the step is repeatable bit for bit, from a fresh model and under hipGraph replay.

Every step-vs-oracle test below B_BIG reaches these paths one forced switch at a time at B <= 16; the only whole step at this size compared
the engine with itself.  Each run happens once (module-scoped fixtures)."""
import numpy as np
import pytest
import torch

import large_regime as LR
import model_checks as MC
from helpers import build_model, model_config
from oracle import mm_oracle as O
from plan_sig import SWITCHES

pytestmark = pytest.mark.gpu

B, T, N_AP, N_BEH = LR.B_BIG, LR.T, LR.N_AP, LR.N_BEH
R = B * LR.MODS * T
N_ATTN_SITES = 2 + 2 * 2                  # self-attention per encoder layer; self- and cross-attention per decoder layer
OBJECTIVES = ("encoding", "token_masking", "decoding")


def config():
    return model_config(n_enc=2, n_dec=2)                # dropout as configured: 0.4 in the blocks, 0.2 behind the tokenisers


@pytest.fixture(scope="module", autouse=True)
def no_switches():
    """The automatic choice everywhere: no plan-time switch, no MMFM_LIVE_ROWS / MMFM_CTX_GROUP / MMFM_GRAPH for the whole module."""
    mp = pytest.MonkeyPatch()
    for k in SWITCHES + ("MMFM_LIVE_ROWS", "MMFM_CTX_GROUP", "MMFM_GRAPH"):
        mp.delenv(k, raising=False)
    yield
    mp.undo()


@pytest.fixture(scope="module")
def batch():
    """Trial 0 unpadded (its masks choose the dead time bins); padded trials in the first pass, in the middle, and the last trial, whose
    rows 68,400 .. 68,599 end in the ragged pass that starts at row 68,480."""
    assert R == 535 * 128 + 120 and (B - 1) * 200 < 535 * 128 < R
    pad = [0] * B
    pad[3], pad[15], pad[200], pad[B - 1] = 10, 37, 5, 37
    return O.synth_batch(B, T, N_AP, N_BEH, seed=2, pad=pad)


def plan_record(Bp):
    """regime_record of the bf16 training plan of the 2 + 2-layer model at batch Bp: the plan is built, no kernel of the step runs."""
    model = build_model(config(), N_AP, N_BEH, seed=3)
    model.compute_dtype = "bf16"
    model.cuda()
    eng = model.engine()
    rec = LR.regime_record(eng, eng._plan(Bp, T, True, True))
    del model, eng
    torch.cuda.empty_cache()
    return rec


@pytest.fixture(scope="module")
def bench_record():
    return plan_record(LR.B_BENCH)


def run(batch, objective, dtype):
    """One step and its oracle; what the tests read is copied out and the engine's pool is dropped."""
    out, named, ref, grads, eng = MC.engine_step_and_oracle(config(), N_AP, N_BEH, batch, objective, dtype, 3)
    res = dict(out=out, named=named, grads=grads, loss=ref["loss"].detach(), ref=dict(loss=ref["loss"].detach()),
               n={m: int(ref["mod_n_examples"][m]) for m in ("ap", "behavior")},
               mod_loss={m: ref["mod_loss"][m].detach() for m in ("ap", "behavior")},
               mod_preds={m: ref["mod_preds"][m].detach() for m in ("ap", "behavior")},
               record=LR.regime_record(eng, eng._last), sites=eng.dropout_sites(B, T),
               live=eng._last["b"]["live"][:, 0].cpu().tolist() if "live" in eng._last["b"] else None)
    for s in res["sites"]:
        s["keepbits"] = s.get("keepbits") is not None
    del eng, ref
    torch.cuda.empty_cache()
    return res


@pytest.fixture(scope="module", params=OBJECTIVES)
def bf16_run(request, batch):
    return request.param, run(batch, request.param, "bf16")


@pytest.fixture(scope="module")
def fp32_run(batch):
    return run(batch, "token_masking", "fp32")


# ------------------------------------------------------------------------------------------------ the regime
def test_regime_record_at_b_big_is_the_one_of_the_benchmark_batch(bench_record):
    """If this fails B_BIG is wrong (a gate lies between it and 1024), not the assertion."""
    rec = plan_record(B)
    diff = LR.record_diff(rec, bench_record)
    assert not diff, "\n".join(diff[:40])
    d = rec["decisions"]
    assert d == dict(fm=15, batch_red=False, pair_ok=True, ctx_group=True, live=True, use_keep=dict(encoder=True, decoder=True))
    fwd, bwd = rec["names"]["fwd"], [n for u, names in rec["names"].items() if u != "fwd" for n in names]
    assert fwd.count("mmfm_live_bins") == 1 and fwd.count("mmfm_gemm_live") == 8 and fwd.count("mmfm_rowgemm_groups") == 1
    assert rec["names"]["bwd/bridge"][0] == "mmfm_rowgemm_groups" and "mmfm_gemm_pair" in bwd and "mmfm_reduce_slabs_multi" not in bwd
    gates = [g for unit in rec["launches"].values() for g in unit]
    row_owner = [g for g in gates if g["fn"] in LR.ROW_OWNER]
    assert len(row_owner) >= 30 and all(g["second_pass"] and not g["column_blocks"] for g in row_owner)
    kernels = [k for g in gates for k in ([g["kernel"]] if "kernel" in g else [g["a"]["kernel"], g["b"]["kernel"]] if "a" in g else [])]
    assert "dw128" not in kernels and kernels.count("dw256") >= 20
    assert all(g["one_launch"] for g in gates if g["fn"] == "mmfm_gemm_pair")
    # the `ap` tokenisers' weight gradients (B T rows, two linears per side) stream wide tiles: what B = 327 (32,700 rows) does not do
    live_dw = [g for g in gates if g["fn"] == "mmfm_gemm_live" and not g["a_kcontig"]]
    assert len(live_dw) == 8 and sum(g["kernel"] == "dw256" for g in live_dw) == 4


# ------------------------------------------------------------------------------------------------ bf16 against the fp64 oracle
def test_bf16_step_vs_fp64_oracle(bf16_run, bench_record):
    """check_bf16's bounds (loss within 2e-2, gradient cosine > 0.995, > 0.98 under 256 elements, norm within 5e-2, key.bias skipped); the
    per-modality losses at the loss bound and the predictions (bf16 buffers of B x T x channels) at the tensor bounds (cosine > 0.995,
    norm within 5e-2); counts exact.
    Measured on the MI355X at B = 343 (loss error, min cosine >= 256 / < 256 elements, max norm error; predictions: min cosine, max norm error):
      encoding      1.8e-5, 0.999990 / 0.999976, 3.7e-3; predictions 0.999982, 8.0e-4
      token_masking 1.1e-5, 0.999990 / 0.999973, 3.5e-3; predictions 0.999982, 7.4e-4  (sample 0 keeps 72 / 77 of 100 bins live)
      decoding      1.7e-4, 0.999988 / 0.999999, 5.2e-3; predictions 0.999981, 5.4e-4"""
    objective, r = bf16_run
    diff = LR.record_diff(r["record"], bench_record)
    assert not diff, "\n".join(diff[:40])
    attn = [s for s in r["sites"] if s["kind"] == "attn"]
    assert len(attn) == N_ATTN_SITES and all(s["keepbits"] for s in attn)
    assert len(r["sites"]) == 4 + 2 * 3 + 2 * 5 and all(s["kind"] == "rowdrop" for s in r["sites"] if s["key"].endswith("/mlpdrop"))
    # live time bins of sample 0 per modality slot (ap, behavior): `encoding` masks every ap bin and no behavior bin, `decoding` the
    # reverse - there a modality is all dead or all live; under `token_masking` each slot keeps some bins and loses some, so the compact
    # row space differs from the full one
    print(f"{objective}: live bins of sample 0 per slot {r['live']}")
    if objective == "token_masking":
        assert all(0 < n < T for n in r["live"]), r["live"]
    else:
        assert r["live"] == ([0, T] if objective == "encoding" else [T, 0])
    out = r["out"]
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == r["n"][m]
        ml, ref_ml = out.mod_loss[m].item(), r["mod_loss"][m].item()
        p, ref_p = out.mod_preds[m].double(), r["mod_preds"][m]
        cos, nerr = MC.cosine(p, ref_p), abs(p.norm().item() / ref_p.norm().item() - 1)
        print(f"{objective} {m}: n {r['n'][m]}, mod_loss {ml} (oracle {ref_ml}), predictions cosine {cos:.6f}, norm error {nerr:.2e}")
        assert ml == pytest.approx(ref_ml, rel=2e-2, abs=1e-6)
        assert cos > 0.995 and nerr < 5e-2, (m, cos, nerr)
    MC.check_bf16(MC.bf16_stats(out, r["named"], r["ref"], r["grads"]), f"bf16, B = {B}, {objective}")


# ------------------------------------------------------------------------------------------------ fp32 against the fp64 oracle
def worst(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): np.testing.assert_allclose passes up to 1."""
    return float(((got.double() - ref.double()).abs() / (atol + rtol * ref.double().abs())).max())


def test_fp32_step_loss_and_predictions_vs_fp64_oracle(fp32_run):
    """The fp32 parity engine at R = 68,600 rows, `token_masking`, dropout on: loss rel 2e-5, per-modality loss rel 5e-5, n exact,
    predictions rtol 1e-4 / atol 2e-5 - the tolerances test_fp32_dropout_step_vs_oracle_fed_the_steps_masks set at 24 rows.
    Measured on the MI355X: loss rel 3.5e-8, per-modality loss 1.4e-8 / 3.0e-8, predictions worst |err| / (atol + rtol |ref|) 0.045 (ap) and
    0.028 (behavior); plain torch in fp32 on the same inputs, masks and multipliers: 3.5e-8, 0.046 and 0.024."""
    r, out = fp32_run, fp32_run["out"]
    assert r["record"]["decisions"]["fm"] == 0 and not r["record"]["decisions"]["live"] and not r["record"]["decisions"]["batch_red"]
    print(f"fp32 B = {B}: loss {out.loss.item()} oracle {r['loss'].item()} rel {abs(out.loss.item() / r['loss'].item() - 1):.2e}")
    for m in ("ap", "behavior"):
        print(f"  {m}: mod_loss rel {abs(out.mod_loss[m].item() / r['mod_loss'][m].item() - 1):.2e}, "
              f"predictions worst |err| / (2e-5 + 1e-4 |ref|) {worst(out.mod_preds[m], r['mod_preds'][m], 1e-4, 2e-5):.2e}")
    assert out.loss.item() == pytest.approx(r["loss"].item(), rel=2e-5)
    for m in ("ap", "behavior"):
        assert int(out.mod_n_examples[m]) == r["n"][m] > 0
        assert out.mod_loss[m].item() == pytest.approx(r["mod_loss"][m].item(), rel=5e-5, abs=1e-6)
        np.testing.assert_allclose(out.mod_preds[m].cpu().numpy(), r["mod_preds"][m].cpu().numpy(), rtol=1e-4, atol=2e-5)


def test_fp32_step_gradients_vs_fp64_oracle(fp32_run):
    """Every parameter gradient at rtol 2e-3, atol 3e-6 + 1e-4 max|ref|: slab sizing, split counts, the two-stage reductions and the
    column sums of the large regime under an element-wise tolerance.
    Measured on the MI355X: worst |err| / (atol + rtol |ref|) over the 120 tensors 1.2e-4 (decoder_embeddings.ap.out.weight); plain torch in
    fp32 on the same inputs, masks and multipliers is 9.4e-4 off the fp64 oracle (decoder.1.attn.value.weight): the engine's slab-wise sums
    are the more accurate of the two."""
    named, grads = fp32_run["named"], fp32_run["grads"]
    ratios = {k: worst(g, grads[k], 2e-3, 3e-6 + 1e-4 * float(grads[k].abs().max())) for k, g in named.items()}
    k = max(ratios, key=ratios.get)
    print(f"fp32 B = {B}: worst |err| / (atol + rtol |ref|) over {len(ratios)} gradients: {ratios[k]:.2e} at {k}")
    for k, g in named.items():
        r = grads[k].cpu().numpy()
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=2e-3, atol=3e-6 + 1e-4 * np.abs(r).max(), err_msg=k)


# ------------------------------------------------------------------------------------------------ repeatability
def test_two_fresh_models_give_the_same_bits(batch):
    """Fixed slab order, tickets, no float atomics: the same seeds give the same loss, predictions and gradients, bit for bit.  A
    mismatch is a race or an order dependence."""
    res = []
    for _ in range(2):
        model = build_model(config(), N_AP, N_BEH, seed=3)
        model.compute_dtype, model.engine_seed = "bf16", 77
        model.cuda().train()
        torch.manual_seed(5)
        out = model(MC.to_dev(O.make_mod_dict(batch, "token_masking")))
        out.loss.backward()
        torch.cuda.synchronize()
        res.append((out.loss.detach().clone(), {m: p.clone() for m, p in out.mod_preds.items()}, {k: p.grad.clone() for k, p in model.named_parameters()}))
        del model, out
        torch.cuda.empty_cache()
    (l0, p0, g0), (l1, p1, g1) = res
    assert torch.equal(l0, l1) and bool(torch.isfinite(l0))
    for m in p0:
        assert torch.equal(p0[m], p1[m]), m
    assert len(g0) > 100
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_graph_replay_matches_eager(monkeypatch):
    """Three optimiser steps in bf16 (eager, captured, replayed) with MMFM_GRAPH=1 against 0: the same losses and the same parameters."""
    def make_model():
        model = build_model(config(), N_AP, N_BEH, seed=3)
        model.compute_dtype, model.engine_seed = "bf16", 77
        return model
    MC.graph_replay_matches_eager(monkeypatch, make_model, dict(B=B, T=T, n_ap=N_AP, n_beh=N_BEH, total_steps=10), steps=3, params=True)
