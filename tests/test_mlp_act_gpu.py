"""transformer.act = relu / silu / quick_gelu / gelu_new on the MI355X: the GEMM epilogues (fp32, bf16 128-tile, bf16 256-tile), the
fused MLP kernels (forward, one-launch backward, front half + rowgemm) against fp64 torch, and whole models against the reference's
own forward / backward (tests/golden/mlp_act_*, scripts/make_mlp_act_goldens.py)."""
import numpy as np
import pytest
import torch

from conftest import load_json, load_npz
from gemm_on import gemm_on
from helpers import build_model, make_optimizer, model_config, tiny_config
from model_checks import check_fixture_case, cosine, resume_roundtrip, run_curve, to_dev
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu
KINDS = {"relu": (L.MLP_RELU, 1.0), "silu": (L.MLP_SIGMOID, 1.0), "quick_gelu": (L.MLP_SIGMOID, 1.702), "gelu_new": (L.MLP_GELU_TANH, 1.0)}
K_TANH = (2.0 / np.pi) ** 0.5


def f_ref(kind, beta, u):
    u = u.double()
    if kind == L.MLP_RELU:
        return torch.relu(u)
    if kind == L.MLP_SIGMOID:
        return u * torch.sigmoid(beta * u)
    if kind == L.MLP_GELU_TANH:
        return 0.5 * u * (1 + torch.tanh(K_TANH * (u + 0.044715 * u ** 3)))
    return torch.nn.functional.gelu(u)


def df_ref(kind, beta, u):
    u = u.double().clone().requires_grad_(True)
    f_ref(kind, beta, u).backward(torch.ones_like(u))
    return u.grad


def bf(t):
    return t.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- GEMM epilogues
def special_rows(u):
    """Row 0: u = 0 exactly; row 1: |u| up to 1e4 (saturation; exp overflows inside the kernels)."""
    u[0] = 0.0
    u[1] = torch.linspace(-1e4, 1e4, u.shape[1])
    return u


# (M, N, K, dtype): fp32 kernel, bf16 128 tile (vector epilogue; N = 670: the scalar one), bf16 256 tile (K >= 512, enough tiles)
FAMILY = {"fp32": L.GEMM_FAMILY_F32, "bf16": L.GEMM_FAMILY_TILE128, "big": L.GEMM_FAMILY_BIG256}      # asserted of every launch (gemm_on)
SHAPES = [(300, 264, 128, "fp32"), (700, 520, 256, "bf16"), (300, 670, 256, "bf16"), (2048, 1024, 512, "big")]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[3]}-N{s[1]}")
@pytest.mark.parametrize("name", list(KINDS))
def test_gemm_act_epilogues(monkeypatch, shape, name):
    """Forward kind: C = f(A B^T + bias) and pre_out; gradient kind: C = (A B^T) * f'(u) with u = gradmul_pre.  Row 0 of A is zero
    (u = bias, u = 0 exactly in column 0); row 1 is a unit vector on column 0, which only it uses, and W's column 0 sweeps -1e4 .. 1e4,
    so the forward kinds see |u| up to 1e4 there (exp overflow inside the kernels); the gradient kinds get the same sweep."""
    kind, beta = KINDS[name]
    fwd, grad = K.GEMM_ACTS[kind]
    M, N, Kd, mode = shape
    if mode == "big":
        monkeypatch.setenv("MMFM_GEMM_BIG_MIN_TILES", "1")
    code = L.F32 if mode == "fp32" else L.BF16
    dt = torch.float32 if mode == "fp32" else torch.bfloat16
    gen = torch.Generator().manual_seed(3)
    A = torch.randn(M, Kd, generator=gen) * 0.3
    A[:2] = 0.0
    A[:, 0] = 0.0
    A[1, 0] = 1.0
    W = torch.randn(N, Kd, generator=gen) * 0.2
    W[:, 0] = torch.linspace(-1e4, 1e4, N)
    bias = torch.randn(N, generator=gen) * 3.0
    bias[0] = 0.0
    A, W = A.to(dt).cuda(), W.to(dt).cuda()
    bias = bias.cuda()
    C = torch.empty(M, N, dtype=dt, device="cuda")
    pre = torch.empty(M, N, dtype=dt, device="cuda")
    gemm_on(FAMILY[mode], A, W, C, M, N, Kd, lda=Kd, ldb=Kd, ldc=N, bias=bias, pre_out=pre, act=fwd, act_scale=beta, dtype=code)
    torch.cuda.synchronize()
    u = A.double() @ W.double().t() + bias.double()
    want = f_ref(kind, beta, u)
    tol = (1e-4, 1e-4) if mode == "fp32" else (1e-2, 2e-2)
    assert torch.isfinite(C.float()).all()
    torch.testing.assert_close(pre.double(), u, rtol=tol[0], atol=tol[1] if mode == "fp32" else 3e-2)
    # f against the stored pre-activation (bf16: the rounded u both sides)
    torch.testing.assert_close(C.double(), f_ref(kind, beta, pre.double()), rtol=tol[0], atol=tol[1])
    torch.testing.assert_close(C.double()[:2], want[:2], rtol=tol[0], atol=tol[1])
    assert u[1].abs().max().item() > 9e3
    if kind == L.MLP_RELU:
        assert C[0, 0] == 0                        # u = 0 exactly
    # gradient kind: u = special values, gradmul_pre = u
    us = special_rows(torch.randn(M, N, generator=gen) * 2.5).to(dt).cuda()
    D = torch.empty(M, N, dtype=dt, device="cuda")
    dY = (torch.randn(M, Kd, generator=gen) * 0.3).to(dt).cuda()
    dY[:2] = 0.0
    dY[:2, 0] = 1.0
    Wg = (torch.randn(N, Kd, generator=gen) * 0.2).to(dt).cuda()
    Wg[:, 0] = 1.0                                 # rows 0 / 1 of dY . Wg^T are exactly 1: D = f'(u) there
    gemm_on(FAMILY[mode], dY, Wg, D, M, N, Kd, lda=Kd, ldb=Kd, ldc=N, act=grad, act_scale=beta, gradmul_pre=us, dtype=code)
    torch.cuda.synchronize()
    assert torch.isfinite(D.float()).all()
    wantd = (dY.double() @ Wg.double().t()) * df_ref(kind, beta, us)
    torch.testing.assert_close(D.double(), wantd, rtol=tol[0], atol=tol[1] if mode == "fp32" else 3e-2)
    torch.testing.assert_close(D.double()[:2], df_ref(kind, beta, us[:2]), rtol=tol[0], atol=tol[1])
    if kind == L.MLP_RELU:
        assert (D[0] == 0).all()                   # torch's relu gradient at 0


# ---------------------------------------------------------------------------------------------- fused MLP kernels
def mlp_weights(scalenorm, seed=2):
    gen = torch.Generator().manual_seed(seed)
    Wu, bu = (torch.randn(512, 256, generator=gen) * 0.06).cuda(), (torch.randn(512, generator=gen) * 0.1).cuda()
    Wd, bd = (torch.randn(256, 512, generator=gen) * 0.04).cuda(), (torch.randn(256, generator=gen) * 0.1).cuda()
    gamma = (1 + 0.1 * torch.randn(256, generator=gen)).cuda()
    beta = (0.1 * torch.randn(256, generator=gen)).cuda()
    Wp = torch.zeros(512, 256, dtype=torch.bfloat16, device="cuda")
    WpT = torch.zeros(256, 512, dtype=torch.bfloat16, device="cuda")
    WpTP = torch.zeros(256, 512, dtype=torch.bfloat16, device="cuda")
    bp = torch.zeros(512, device="cuda")
    WdP = torch.zeros(256, 512, dtype=torch.bfloat16, device="cuda")
    WdT = torch.zeros(512, 256, dtype=torch.bfloat16, device="cuda")
    up = dict(W=Wu, bias=bu, Wp=Wp, WpT=WpT, WpTP=WpTP, bp=bp)
    if scalenorm:
        up.update(gamma=torch.tensor([16.0], device="cuda"), scalar_gain=True)
    else:
        up.update(gamma=gamma, beta=beta)
    table, n, tiles = K.prep_table([up, dict(W=Wd, WpP=WdP, WpT=WdT)], "cuda")
    K.prep_weights(table, n, tiles)
    torch.cuda.synchronize()
    return dict(Wp=Wp, WpT=WpT, WpTP=WpTP, bp=bp, WdP=WdP, WdT=WdT, Wd=bf(Wd), bd=bd)


def mlp_ref(kind, beta, xh, w, dy):
    """fp64: from the kernel's own x_hat: u, g, y - x, and t1 / du / d(x_hat) for dy."""
    xh = xh.double()
    u = xh @ w["Wp"].double().t() + w["bp"].double()
    g = f_ref(kind, beta, u)
    y = g @ w["Wd"].double().t() + w["bd"].double()
    dg = dy.double() @ w["Wd"].double()
    du = dg * df_ref(kind, beta, u)
    return u, g, y, du, du @ w["Wp"].double()


@pytest.mark.parametrize("norm", ["layernorm", "scalenorm"])
@pytest.mark.parametrize("name", list(KINDS))
def test_fused_mlp_forward_and_backward(name, norm):
    """Forward, the front half (t1, g, du) + rowgemm(ln_bwd) and (LayerNorm only) the one-launch backward, every row against fp64."""
    kind, beta = KINDS[name]
    sn = norm == "scalenorm"
    R, pad = 3000, 128
    gen = torch.Generator().manual_seed(4)
    x = bf((torch.randn(R, 256, generator=gen) * (1 + torch.rand(R, 1, generator=gen) * 3)).cuda())
    dy = bf((torch.randn(R, 256, generator=gen) * 0.1).cuda())
    w = mlp_weights(sn)
    # saturation: eight intermediate units get pre-activations far out on both sides (the norm bounds x_hat, not the bias)
    w["bp"][:8] = torch.tensor([-300.0, -100.0, -30.0, -10.0, 10.0, 30.0, 100.0, 300.0], device="cuda")
    y = torch.full((R + pad, 256), 5.0, dtype=torch.bfloat16, device="cuda")
    xh = torch.full((R + pad, 256), 5.0, dtype=torch.bfloat16, device="cuda")
    rs = torch.full((R + pad,), 5.0, device="cuda")
    K.mlp_fwd(K.mlp_desc(R, x=x, w_up=w["Wp"], b_up=w["bp"], w_down=w["WdP"], b_down=w["bd"], y=y, xhat=xh, rstd=rs, scalenorm=sn,
                         act=kind, act_beta=beta))
    torch.cuda.synchronize()
    assert (y[R:] == 5.0).all() and (xh[R:] == 5.0).all() and (rs[R:] == 5.0).all()
    xd = x.double()
    if sn:
        want_xh = xd / xd.norm(dim=-1, keepdim=True).clamp(min=1e-5)
    else:
        want_xh = (xd - xd.mean(-1, keepdim=True)) / (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    assert (xh[:R].double() - want_xh).abs().max().item() < 3e-2 * max(1.0, want_xh.abs().max().item())
    u, g, yd, du, dxh = mlp_ref(kind, beta, xh[:R], w, dy)
    err = (y[:R].double() - (xd + yd)).abs().max(dim=1).values
    assert torch.isfinite(y[:R].float()).all()
    assert (err < 2e-2 * (xd + yd).abs().max(dim=1).values.clamp(min=1.0)).all(), err.max().item()
    modes = ["split"] if sn else ["split", "one"]
    for mode in modes:
        t1 = torch.full((R + pad, 256), 7.0, dtype=torch.bfloat16, device="cuda")
        gb = torch.full((R + pad, 512), 7.0, dtype=torch.bfloat16, device="cuda")
        dub = torch.full((R + pad, 512), 7.0, dtype=torch.bfloat16, device="cuda")
        dx = torch.full((R + pad, 256), 7.0, dtype=torch.bfloat16, device="cuda")
        d = K.mlp_desc(R, w_up=w["Wp"], b_up=w["bp"], xhat=xh, rstd=rs, dy=dy, w_down_t=w["WdT"], w_up_t=w["WpTP"], t1=t1, g=gb, du=dub,
                       dx=None if mode == "split" else dx, scalenorm=sn, act=kind, act_beta=beta)
        K.mlp_bwd(d)
        if mode == "split":
            K.rowgemm(dub, w["WpT"], dx, R, 256, 512, residual=dy, ldr=256, ln_bwd=2 if sn else 1, bwd_xhat=xh, bwd_rstd=rs)
        torch.cuda.synchronize()
        assert (gb[R:] == 7.0).all() and (dub[R:] == 7.0).all() and (dx[R:] == 7.0).all()
        assert torch.equal(t1[:R], dy)
        assert torch.isfinite(gb[:R].float()).all() and torch.isfinite(dub[:R].float()).all()
        eg = (gb[:R].double() - g).abs().max(dim=1).values
        assert (eg < 2e-2 * g.abs().max(dim=1).values.clamp(min=1.0)).all(), (mode, eg.max().item())
        # du from the kernel's own bf16 u rounding: compare against fp64 with a row-relative bound
        edu = (dub[:R].double() - du).abs().max(dim=1).values
        assert (edu < 3e-2 * du.abs().max(dim=1).values.clamp(min=1e-3)).all(), (mode, edu.max().item())
        if kind == L.MLP_RELU:
            assert (dub[:R][u < -1e-2] == 0).all()
        # dx = dy + norm'(d x_hat)
        rsd = rs[:R].double().abs()[:, None]
        xhd = xh[:R].double()
        if sn:
            s = (dxh * xhd).sum(-1, keepdim=True)
            want_dx = dy.double() + rsd * (dxh - torch.where(rs[:R, None] < 0, 0.0, 1.0).double() * xhd * s)
        else:
            want_dx = dy.double() + rsd * (dxh - dxh.mean(-1, keepdim=True) - xhd * (dxh * xhd).mean(-1, keepdim=True))
        edx = (dx[:R].double() - want_dx).abs().max(dim=1).values
        assert (edx < 3e-2 * want_dx.abs().max(dim=1).values.clamp(min=1e-2)).all(), (mode, edx.max().item())


@pytest.mark.parametrize("name", ["relu", "silu", "gelu_new"])
def test_fused_mlp_dropout_mask_matches_between_forward_and_backward(name):
    """The forward's dropout decisions, read off y (a dropped element leaves y = x), are the ones the backward regenerates:
    t1 = dropout'(dy) is zero exactly there and 1 / (1 - p) elsewhere (as tests/test_rowchain_gpu.py checks for GELU)."""
    kind, beta = KINDS[name]
    R, p = 640, 0.4
    w = mlp_weights(False, seed=6)
    gen = torch.Generator().manual_seed(8)
    x = bf((torch.randn(R, 256, generator=gen) * 1.5).cuda())
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    K.rng_seed(state, 5)
    drop = K.dropout(state, 9, p)
    y, xh, rs = (torch.empty(R, 256, dtype=torch.bfloat16, device="cuda"), torch.empty(R, 256, dtype=torch.bfloat16, device="cuda"),
                 torch.empty(R, device="cuda"))
    K.mlp_fwd(K.mlp_desc(R, x=x, w_up=w["Wp"], b_up=w["bp"], w_down=w["WdP"], b_down=w["bd"], drop=drop, y=y, xhat=xh, rstd=rs,
                         act=kind, act_beta=beta))
    y0 = torch.empty_like(y)
    K.mlp_fwd(K.mlp_desc(R, x=x, w_up=w["Wp"], b_up=w["bp"], w_down=w["WdP"], b_down=w["bd"], y=y0, xhat=xh, rstd=rs, act=kind, act_beta=beta))
    torch.cuda.synchronize()
    kept = (y.float() - x.float()) != 0
    assert 0.57 < kept.float().mean().item() < 0.63
    ref = torch.where(kept, (y0.float() - x.float()) / (1 - p), torch.zeros((), device="cuda"))
    big = ref.abs() > 0.5
    torch.testing.assert_close((y.float() - x.float())[big], ref[big], rtol=0.05, atol=0.02)
    dy = torch.ones(R, 256, dtype=torch.bfloat16, device="cuda")
    t1, g, du = (torch.empty(R, 256, dtype=torch.bfloat16, device="cuda"), torch.empty(R, 512, dtype=torch.bfloat16, device="cuda"),
                 torch.empty(R, 512, dtype=torch.bfloat16, device="cuda"))
    K.mlp_bwd(K.mlp_desc(R, w_up=w["Wp"], b_up=w["bp"], drop=drop, xhat=xh, rstd=rs, dy=dy, w_down_t=w["WdT"], w_up_t=w["WpTP"], t1=t1,
                         g=g, du=du, act=kind, act_beta=beta))
    torch.cuda.synchronize()
    sure = (y0.float() - x.float()).abs() > 0.25
    assert sure.float().mean().item() > 0.2
    torch.testing.assert_close(t1.float()[sure], (kept.float() / (1 - p))[sure], rtol=1e-2, atol=1e-2)
    assert 0.57 < (t1 != 0).float().mean().item() < 0.63


# ---------------------------------------------------------------------------------------------- models, fp32 against the reference
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("mlp_act_fwd_bwd.npz")
    return _Z


@pytest.mark.parametrize("act", list(KINDS))
@pytest.mark.parametrize("objective", ["encoding", "decoding", "token_masking"])
def test_tiny_forward_backward_vs_reference_fixture(act, objective):
    z, meta = fixture()
    check_fixture_case(build_model(tiny_config(act=act), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"]), z, meta, act, objective)


@pytest.mark.parametrize("act", list(KINDS))
def test_loss_curve_tiny_50_steps_vs_reference_fixture(act):
    g = load_json("mlp_act_curve.json")["tiny"][act]
    model = build_model(tiny_config(act=act), g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    losses = run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


@pytest.mark.parametrize("act", ["relu", "silu"])
def test_default_config_scalars_vs_reference_fixture(act):
    g = load_json("mlp_act_curve.json")["default"][act]
    model = build_model(model_config(dropout=0.0, emb_dropout=0.0, act=act), 668, 2, seed=42).cuda().eval()
    batch = O.synth_batch(16, 100, 668, 2, seed=0)
    for obj in ("encoding", "decoding", "token_masking"):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(1)
        out = model(to_dev(O.make_mod_dict(batch, obj)))
        out.loss.backward()
        assert out.loss.item() == pytest.approx(g[obj]["loss"], rel=1e-5)
        for m in ("ap", "behavior"):
            assert int(out.mod_n_examples[m]) == g[obj]["n"][m]
            assert float(out.mod_preds[m].double().abs().sum()) == pytest.approx(g[obj]["pred_abssum"][m], rel=1e-4)
        for k, prm in model.named_parameters():
            assert float(prm.grad.double().norm()) == pytest.approx(g[obj]["grad_norm"][k], rel=5e-3, abs=1e-8), k


# ---------------------------------------------------------------------------------------------- bf16: fused against un-fused, drift
@pytest.mark.parametrize("act", list(KINDS))
def test_bf16_fused_path_matches_unfused_kernels(monkeypatch, act):
    kind, beta = KINDS[act]
    batch = O.synth_batch(16, 100, 668, 2, seed=0)
    seen = []
    mlp_fwd = K.mlp_fwd
    res = {}
    for mode in ("0", "15"):
        monkeypatch.setenv("MMFM_FUSED", mode)
        with monkeypatch.context() as mp:
            mp.setattr(K, "mlp_fwd", lambda d, plan=None: (seen.append((d.act, d.act_beta)), mlp_fwd(d, plan=plan))[1])
            model = build_model(model_config(dropout=0.0, emb_dropout=0.0, act=act), 668, 2, seed=42)
            model.compute_dtype = "bf16"
            model.cuda().train()
            model.zero_grad(set_to_none=True)
            torch.manual_seed(1)
            o = model(to_dev(O.make_mod_dict(batch, "token_masking")))
            o.loss.backward()
            res[mode] = (o.loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
        del model
        torch.cuda.empty_cache()
    assert seen and all(a == kind and b == pytest.approx(beta) for a, b in seen), seen
    l0, g0 = res["0"]
    l1, g1 = res["15"]
    assert np.isfinite(l0) and l1 == pytest.approx(l0, rel=3e-3)
    for k in g0:
        if g0[k].abs().max() == 0:
            assert g1[k].abs().max() == 0, k
            continue
        if k.endswith("key.bias"):
            continue
        c = cosine(g0[k], g1[k])
        assert c > (0.995 if g0[k].numel() >= 256 else 0.98), f"{k}: cosine {c}"


@pytest.mark.parametrize("act", ["relu", "silu"])
def test_bf16_drift_against_fp32_over_12_steps(monkeypatch, act):
    monkeypatch.setenv("MMFM_FUSED", "15")
    losses = {}
    for dtype in ("fp32", "bf16"):
        model = build_model(model_config(n_enc=2, n_dec=2, dropout=0.0, emb_dropout=0.0, act=act), 668, 2, seed=3)
        model.compute_dtype = dtype
        model.cuda().train()
        opt, sch = make_optimizer(model, 12, lr=5e-4)
        torch.manual_seed(5)
        ls = []
        for s in range(12):
            out = model(to_dev(O.make_mod_dict(O.synth_batch(8, 100, 668, 2, seed=s), "encoding")))
            out.loss.backward()
            opt.step(); sch.step(); opt.zero_grad()
            ls.append(out.loss.item())
        losses[dtype] = np.array(ls)
        del model
        torch.cuda.empty_cache()
    assert np.isfinite(losses["bf16"]).all()
    np.testing.assert_allclose(losses["bf16"], losses["fp32"], rtol=2e-2)


# ---------------------------------------------------------------------------------------------- resume
def test_silu_resume_from_train_state_is_bit_identical(tmp_path):
    """6 steps in one go == 3 steps, save_model + train state, fresh objects restored from the files, 3 more steps (bf16, dropout on)."""
    resume_roundtrip(tmp_path, tiny_config(n_enc=2, n_dec=2, dropout=0.4, emb_dropout=0.2, act="silu"), dtype="bf16")
