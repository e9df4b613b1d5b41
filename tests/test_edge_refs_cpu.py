"""The fp64 references of tests/edge_refs.py against torch autograd in fp64 (and the committed mask fixture), and the
tolerance helpers against hand-made values.  No GPU: this file proves the yardstick tests/test_edge_kernels_gpu.py uses."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_refs as E
from conftest import load_npz
from oracle import mm_oracle as O

D = torch.float64


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D) * scale


def same(a, b, what, rtol=1e-12, atol=1e-13):
    assert a.dtype == D, f"{what}: the reference must return fp64, got {a.dtype}"
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {(a - b).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------------- stitch
@pytest.mark.parametrize("B,T,M,H,max_F", [(3, 7, 3, 36, 9), (2, 5, 2, 4, 1)])
def test_stitch_refs_match_embedding_autograd(B, T, M, H, max_F):
    g = torch.Generator().manual_seed(3)
    L = M * T
    ts = torch.randint(0, max_F, (B, T), generator=g)
    keep0 = (torch.rand(L, generator=g) > 0.3).to(torch.uint8)
    toks = [rnd(B * T, H, seed=10 + m).requires_grad_(True) for m in range(M)]
    mods = [rnd(H, seed=20 + m).requires_grad_(True) for m in range(M)]
    poss = [rnd(max_F, H, seed=30 + m).requires_grad_(True) for m in range(M)]
    e_ref = torch.cat([mods[m][None, None, :] + F.embedding(ts, poss[m]) for m in range(M)], 1)
    x_ref = O.zero_masked_tokens(torch.cat([t.view(B, T, H) for t in toks], 1), (1 - keep0.long())[None].expand(B, L)) + e_ref
    dx, dextra = rnd(B, L, H, seed=40), rnd(B, L, H, seed=41)
    keep = (torch.rand(M, B * T, H, generator=g) > 0.4).to(D)
    p = 0.4
    dropped = [F.dropout(t, 0.0) * keep[m] / (1 - p) for m, t in enumerate(toks)]       # a fixed keep mask in place of the random one
    x_drop = torch.cat([t.view(B, T, H) for t in dropped], 1) * keep0[None, :, None] + e_ref
    (x_drop * dx + e_ref * dextra).sum().backward()
    for m in range(M):
        x, emb, mag = E.stitch_fwd(toks[m].detach(), mods[m].detach(), poss[m].detach(), ts, keep0, m, max_F)
        same(x, x_ref[:, m * T:(m + 1) * T].detach(), "x")
        same(emb, e_ref[:, m * T:(m + 1) * T].detach(), "emb")
        assert (mag >= x.abs() - 1e-12).all()
        r = E.stitch_bwd(dx, dextra, ts, keep0, keep[m], p, m, max_F)
        same(r["d_tok"], toks[m].grad, "d_tok")
        same(r["d_mod"], mods[m].grad, "d_mod")
        same(r["d_pos"], poss[m].grad, "d_pos")
        assert r["n_mod"] == 2 * B * T and float(r["n_pos"].sum()) == 2 * B * T
        assert (r["abs_pos"] >= r["d_pos"].abs() - 1e-12).all() and (r["abs_mod"] >= r["d_mod"].abs() - 1e-12).all()
    # dextra = None, no dropout: the x path alone
    r = E.stitch_bwd(dx, None, ts, keep0, None, 0.0, 0, max_F)
    same(r["d_tok"], dx[:, :T].reshape(B * T, H) * keep0[:T].repeat(B)[:, None], "d_tok (no dropout)")
    same(r["d_mod"], dx[:, :T].sum((0, 1)), "d_mod (no dextra)")
    assert r["n_mod"] == B * T


def test_stitch_ref_clamps_stamps():
    ts = torch.tensor([[-3, 0, 2, 14]])
    pos, tok = rnd(9, 4, seed=1), rnd(4, 4, seed=2)
    x, emb, _ = E.stitch_fwd(tok, torch.zeros(4, dtype=D), pos, ts, torch.zeros(4, dtype=torch.uint8), 0, 9)
    same(emb[0], pos[[0, 0, 2, 8]], "clamped gather")
    same(x, emb, "keep0 = 0 drops the tokens")


# ------------------------------------------------------------------------------------------------- mask preparation
def test_mask_prep_ref_matches_reference_fixture():
    z, cases = load_npz("mask_index_ops.npz")
    attn = torch.from_numpy(z["attn"])
    B, T = attn.shape
    for key in cases:
        ms = [torch.from_numpy(z[f"{key}/in_mask/{m}"]) for m in ("ap", "behavior")]
        full = [m[:, :, None].repeat(1, 1, 3).contiguous() for m in ms]          # stride 3, un-anded
        full[1][:, :, 1:] = 1 - full[1][:, :, 1:]                                # the other channels must not be read
        tok, kpd, keep0, mod, cnt = E.mask_prep(full, [3, 3], attn, [5, 2])
        enc_mask = torch.from_numpy(z[f"{key}/enc_mask"])
        np.testing.assert_array_equal(tok.numpy(), enc_mask.numpy().astype(np.uint8))
        np.testing.assert_array_equal(kpd.numpy(), torch.cat([attn, attn], 1).numpy().astype(np.uint8))
        np.testing.assert_array_equal(mod.numpy(), z[f"{key}/enc_mod_mask"][0].astype(np.uint8))
        np.testing.assert_array_equal(keep0.numpy(), (enc_mask[0] != 1).numpy().astype(np.uint8))
        assert cnt.tolist() == [int(enc_mask[:, :T].sum()) * 5, int(enc_mask[:, T:].sum()) * 2] and cnt.dtype == torch.int64
        xs = [torch.from_numpy(z[f"{key}/in_x/{m}"]) for m in ("ap", "behavior")]
        np.testing.assert_array_equal((torch.cat(xs, 1) * keep0[None, :, None]).numpy(), z[f"{key}/enc_tokens"])


def test_mask_prep_ref_on_wide_mask_values():
    """Values outside {0, 1}: '& attn' first, then tokmask = (v != 0), keep0 = (v[0] != 1), count = channels * sum(v)."""
    attn = torch.tensor([[1, 1, 3, 3, 0], [1, 0, 0, 0, 0]])
    mk = torch.tensor([[0, 1, 2, 3, 3], [2, 1, 1, 1, 1]])
    tok, kpd, keep0, mod, cnt = E.mask_prep([mk], [1], attn, [7])
    assert tok.tolist() == [[0, 1, 1, 1, 0], [0, 0, 0, 0, 0]]
    assert kpd.tolist() == [[1, 1, 1, 1, 0], [1, 0, 0, 0, 0]]
    assert keep0.tolist() == [1, 0, 1, 1, 1] and mod.tolist() == [0] * 5
    assert cnt.tolist() == [7 * (1 + 2 + 3)]


# ------------------------------------------------------------------------------------------------- masked loss
@pytest.mark.parametrize("kind,N", [(0, 12), (1, 2)])
def test_masked_loss_refs_match_torch_losses(kind, N):
    B, T, M = 4, 5, 2
    R = B * T
    pred = rnd(R, N, seed=1, scale=2.0)
    tgt = torch.poisson(torch.full((R, N), 0.3, dtype=D)) if kind == 0 else rnd(R, N, seed=2)
    tokmask = (torch.rand(B, M * T, generator=torch.Generator().manual_seed(5)) < 0.4).to(torch.uint8)
    rowmask = tokmask[:, T:]                                                      # a strided [B, T] view, mask_ld = M*T
    crit = torch.nn.PoissonNLLLoss(reduction="none", log_input=True, full=False) if kind == 0 else torch.nn.MSELoss(reduction="none")
    pr = pred.clone().requires_grad_(True)
    mk = rowmask.reshape(R, 1).to(D).expand(R, N)
    other_sum, other_n = torch.tensor(3.0, dtype=D), 7                            # a second modality's share (mm.py:237)
    total = (crit(pr, tgt) * mk).sum()
    loss = (total + other_sum) / (mk.sum() + other_n)
    (0.5 * loss).backward()
    s, n, sabs, terr = E.masked_loss_sum(kind, pred, tgt, rowmask)
    same(s, total.detach(), "loss sum")
    assert n == int(mk.sum()) and float(sabs) >= abs(float(s)) and 0 < float(terr) < 1e-5 * float(sabs)
    cnt = torch.tensor([int(mk.sum()), other_n])
    l, inv_n = E.loss_finalize(torch.stack([s, other_sum]), cnt)
    same(l, loss.detach(), "loss")
    same(E.masked_loss_bwd(kind, pred, tgt, rowmask, torch.tensor([0.5]), inv_n), pr.grad, "dpred")
    # nothing masked anywhere: 0 / 0 = NaN and a NaN gradient, as autograd gives upstream
    none = torch.zeros(B, T, dtype=torch.uint8)
    pr = pred.clone().requires_grad_(True)
    mk0 = none.reshape(R, 1).to(D).expand(R, N)
    l0 = (crit(pr, tgt) * mk0).sum() / mk0.sum()
    l0.backward()
    s0, n0, _, _ = E.masked_loss_sum(kind, pred, tgt, none)
    lf, inv0 = E.loss_finalize(torch.stack([s0, s0]), torch.zeros(2, dtype=torch.int64))
    assert float(s0) == 0 and n0 == 0 and torch.isnan(lf) and torch.isnan(l0) and torch.isinf(inv0)
    d0 = E.masked_loss_bwd(kind, pred, tgt, none, torch.ones(1), inv0)
    assert torch.isnan(d0).all() and torch.isnan(pr.grad).all()


def test_fast_exp_bound_holds_for_a_plain_fp32_exp():
    """exp_rel_err is derived for __expf; a correctly rounded fp32 exp (half an ulp) must sit inside it everywhere on [-8, 8]."""
    p = torch.linspace(-8, 8, 200001, dtype=torch.float32)
    rel = ((torch.exp(p).double() - torch.exp(p.double())) / torch.exp(p.double())).abs()
    assert (rel <= E.exp_rel_err(p)).all()
    print(f"fp32 exp against fp64 on [-8, 8]: max relative error {rel.max().item():.3e} (bound at p = 0: {2 * E.U32:.3e})")


# ------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("B,M,T,H,destitch", [(3, 3, 5, 36, True), (3, 3, 5, 36, False), (1, 1, 1, 4, False)])
def test_layernorm_refs_match_autograd(B, M, T, H, destitch):
    L = M * T
    R = B * L
    dsL, dsT = (L, T) if destitch else (0, 0)
    x, g, b, dy, dres = rnd(R, H, seed=1, scale=2.0), rnd(H, seed=2), rnd(H, seed=3), rnd(R, H, seed=4), rnd(R, H, seed=5)
    x[0] = 2.0                                                                    # variance 0: eps alone sets rstd
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (H,), gr, br, 1e-5)
    y, mean, rstd = E.layernorm_fwd(x, g, b, 1e-5, dsL, dsT)
    to_mod = (lambda t: t.view(B, M, T, H).permute(1, 0, 2, 3).reshape(R, H)) if destitch else (lambda t: t)
    to_seq = (lambda t: t.view(M, B, T, H).permute(1, 0, 2, 3).reshape(R, H)) if destitch else (lambda t: t)
    same(y, to_mod(yr.detach()), "y")
    same(mean, x.mean(-1), "mean")
    same(rstd, 1 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5), "rstd")
    assert abs(float(rstd[0]) - 1e5 ** 0.5) < 1e-9
    yr.backward(to_seq(dy))                                                       # dy is laid out [M][B*T][H]
    r = E.layernorm_bwd(dy, x, g, dres, 1e-5, dsL, dsT)
    same(r["dx"], xr.grad + dres, "dx", rtol=1e-10, atol=1e-10)
    same(r["dgamma"], gr.grad, "dgamma", rtol=1e-10, atol=1e-10)
    same(r["dbeta"], br.grad, "dbeta")
    same(E.layernorm_bwd(dy, x, g, None, 1e-5, dsL, dsT)["dx"], xr.grad, "dx (no dres)", rtol=1e-10, atol=1e-10)
    assert r["n"] == R and (r["abs_gamma"] >= r["dgamma"].abs() - 1e-12).all() and (r["err_gamma"] > 0).all()


def test_destitch_perm_is_the_modality_gather():
    B, M, T = 3, 3, 5
    L = M * T
    mod_mask = torch.arange(M).repeat_interleave(T)[None].expand(B, L)
    seq = torch.arange(B * L).view(B, L)
    gathered = torch.cat([seq[mod_mask == m] for m in range(M)])                  # decoder_embeddings.py:95-97
    perm = E.destitch_perm(B * L, L, T, "cpu")
    assert torch.equal(gathered[perm], torch.arange(B * L))
    assert torch.equal(E.destitch_perm(7, 0, 0, "cpu"), torch.arange(7))


# ------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_adamw_ref_matches_torch_adamw(grad_scale):
    n = 1001
    p0 = rnd(n, seed=1)
    p, m, v = p0.clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=1e-4, weight_decay=0.01, eps=1e-8)
    po, mo, vo = p0.clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    for step in range(1, 8):
        g = rnd(n, seed=10 + step, scale=0.1)
        lr, b1 = O.onecycle(step - 1, 20)                                         # lr and beta1 change every step
        opt.param_groups[0]["lr"], opt.param_groups[0]["betas"] = lr, (b1, 0.999)
        ref.grad = g * grad_scale
        opt.step()
        E.adamw_step(p, g, m, v, torch.tensor(E.adamw_hyper(step, lr, b1, grad_scale=grad_scale), dtype=D))
        O.adamw_step(po, g * grad_scale, mo, vo, step, lr, b1)
        same(p, ref.data, f"p, step {step}")
        same(p, po, f"p against the oracle, step {step}")
        same(m, opt.state[ref]["exp_avg"], "m")
        same(v, opt.state[ref]["exp_avg_sq"], "v", atol=1e-18)


# ------------------------------------------------------------------------------------------------- reductions
def test_reduction_refs():
    x = rnd(37, 10, seed=1)
    s, n, a = E.colsum(x.float())
    assert s.dtype == D and n == 37
    same(s, x.float().double().sum(0), "colsum")
    same(a, x.float().double().abs().sum(0), "colsum abs")
    src = rnd(5 * 16, seed=2)
    prior = rnd(10, seed=3)
    s, n, a = E.reduce_slabs(src, 10, 5, 16, prior)                               # stride 16 > n = 10: the gaps are not read
    same(s, src.view(5, 16)[:, :10].sum(0) + prior, "reduce_slabs")
    assert n == 6


# ------------------------------------------------------------------------------------------------- the helpers themselves
def _bf16_neighbour(t, up):
    """The next bf16 value above / below (positive finite values)."""
    return (E.bits(t) + (1 if up else -1)).view(torch.bfloat16)


def test_bf16_helper_rejects_one_ulp_too_far():
    ref = rnd(4096, seed=7).abs() + 0.01
    out = ref.to(torch.bfloat16)                                                  # round to nearest even
    assert E.check_bf16(out, ref, 0.0, "rounded") <= 1.0
    away = out.double() >= ref                                                    # step one ulp further away from the reference
    far = torch.where(away, _bf16_neighbour(out, True), _bf16_neighbour(out, False))
    for i in range(0, 4096, 97):
        with pytest.raises(AssertionError, match="bf16 bound"):
            E.check_bf16(far[i:i + 1], ref[i:i + 1], 0.0, "one ulp too far")
    # truncation (round toward zero) of values just below the next bf16 number is out by almost a whole ulp
    t = torch.tensor([1.0 + 2.0 ** -7 - 2.0 ** -20], dtype=D)
    with pytest.raises(AssertionError):
        E.check_bf16(torch.tensor([1.0], dtype=torch.bfloat16), t, 0.0, "truncated")
    # e32 widens the bound by exactly that much, and a wrong dtype or a NaN is refused
    E.check_bf16(torch.tensor([1.0], dtype=torch.bfloat16), t, 2.0 ** -7, "with e32")
    with pytest.raises(AssertionError):
        E.check_bf16(torch.tensor([1.0]), torch.tensor([1.0], dtype=D), 0.0, "fp32 passed as bf16")
    with pytest.raises(AssertionError):
        E.check_bf16(torch.tensor([float("nan")], dtype=torch.bfloat16), torch.tensor([1.0], dtype=D), 1.0, "nan")


def test_sum_helper_holds_for_a_plain_fp32_sum_and_rejects_a_dropped_term():
    for n, scale in [(668, 1.0), (4100, 30.0), (204800, 1.0)]:
        t = rnd(n, 8, seed=n, scale=scale).float()                                # the terms, as stored fp32 values
        ref, cnt, sabs = E.colsum(t)
        assert E.check_sum(t.sum(0), ref, cnt, sabs, f"torch.sum of {n} fp32 terms") <= 1.0
        seq = torch.zeros(8)
        for row in t[:2000]:                                                      # recursive order, the bound's own worst case
            seq = seq + row
        r2, c2, a2 = E.colsum(t[:2000])
        assert E.check_sum(seq, r2, c2, a2, "recursive fp32 sum") <= 1.0
    t = (rnd(668, 4, seed=3).abs() + 0.5).float()
    ref, cnt, sabs = E.colsum(t)
    with pytest.raises(AssertionError, match="fp32 sum bound"):
        E.check_sum(t[:-1].sum(0), ref, cnt, sabs, "last term dropped")
    with pytest.raises(AssertionError):
        E.check_sum(t.double().sum(0), ref, cnt, sabs, "fp64 passed as fp32")


def test_close_and_exact_helpers():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=D)
    E.check_close(torch.tensor([1.0 + 1e-5, -2.0, 1e-5]), ref, (2e-5, 2e-5), "inside")
    with pytest.raises(AssertionError):
        E.check_close(torch.tensor([1.0 + 5e-5, -2.0, 0.0]), ref, (2e-5, 2e-5), "outside")
    with pytest.raises(AssertionError):
        E.check_close(torch.tensor([1.0, float("nan"), 0.0]), ref, (2e-5, 2e-5), "nan")
    E.check_elem(ref.to(torch.bfloat16), ref, (0.0, 0.0), "bf16 through check_elem")
    E.check_exact(torch.tensor([1, 2]), torch.tensor([1, 2]), "equal")
    with pytest.raises(AssertionError):
        E.check_exact(torch.tensor([1, 2]), torch.tensor([1, 3]), "differs")
    with pytest.raises(AssertionError):
        E.check_exact(torch.tensor([1, 2], dtype=torch.int32), torch.tensor([1, 2]), "dtype differs")
    assert math.isclose(E.HALF_ULP_BF16, torch.finfo(torch.bfloat16).eps / 2) and math.isclose(E.U32, torch.finfo(torch.float32).eps / 2)
