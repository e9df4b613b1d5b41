"""use_scalenorm: true on the MI355X: the stand-alone ScaleNorm kernels, the folded bf16 row-owner path (rowgemm ln = 2 /
ln_bwd = 2, the MLP prologue, scalar-gain weight preparation and linear gradients) against fp64 torch, and whole models against
the reference's own forward / backward (tests/golden/scalenorm_*, scripts/make_scalenorm_goldens.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_json, load_npz
from helpers import build_model, make_optimizer, model_config, tiny_config
from model_checks import check_fixture_case, cosine, resume_roundtrip, run_curve, to_dev
from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu
EPS = 1e-5


def sn_ref(x, g, dy, dres=None):
    """fp64 autograd of the reference formula (mm_utils.py:38-39)."""
    x = x.double().clone().requires_grad_(True)
    g = g.double().clone().requires_grad_(True)
    y = x * g / torch.norm(x, dim=-1, keepdim=True).clamp(min=EPS)
    y.backward(dy.double())
    dx = x.grad + (0 if dres is None else dres.double())
    return y.detach(), dx, g.grad


def sn_rows_input(R, H, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(R, H, generator=gen) * (1 + torch.rand(R, 1, generator=gen) * 3)
    x[3] = 0.0                                     # all-zero row
    x[7] = torch.randn(H, generator=gen) * 1e-8    # norm below eps: the clamp branch
    return x.to(dtype).cuda()


# ---------------------------------------------------------------------------------------------- stand-alone kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_dres", [False, True])
def test_standalone_scalenorm_fwd_bwd(dtype, with_dres):
    R, H = 1237, 256                                # not a multiple of any block's rows
    x = sn_rows_input(R, H, dtype, 0)
    dy = (torch.randn(R, H) * 0.1).to(dtype).cuda()
    dres = (torch.randn(R, H) * 0.1).to(dtype).cuda() if with_dres else None
    g = torch.tensor([14.5], device="cuda")
    pad = 5
    y = torch.full((R + pad, H), 3.0, dtype=dtype, device="cuda")
    rinv = torch.full((R + pad,), 3.0, device="cuda")
    K.scalenorm_fwd(x, g, y, rinv, R, H)
    yr, dxr, dgr = sn_ref(x.float(), g[0].cpu().double(), dy.float(), None if dres is None else dres.float())
    tol = dict(rtol=1e-5, atol=1e-5) if dtype == torch.float32 else dict(rtol=1.6e-2, atol=1e-2)
    torch.testing.assert_close(y[:R].double().cpu(), yr.cpu(), **tol)
    assert (y[R:] == 3.0).all() and (rinv[R:] == 3.0).all()                       # guard rows untouched
    n = x.double().norm(dim=-1).cpu()
    want_rinv = 1.0 / n.clamp(min=EPS)
    torch.testing.assert_close(rinv[:R].abs().double().cpu(), want_rinv, rtol=1e-5, atol=0)
    assert ((rinv[:R].cpu() < 0) == (n <= EPS)).all() and bool(rinv[3] < 0) and bool(rinv[7] < 0)
    ws = torch.zeros(K.scalenorm_bwd_workspace(R, H) // 4 + 1, device="cuda")
    dx = dres.clone() if dres is not None else torch.empty_like(x)     # dx aliases dres
    dg = torch.zeros(1, device="cuda")
    K.scalenorm_bwd(dy, x, rinv, g, dx if dres is not None else None, dx, dg, R, H, ws)
    scale = dxr.abs().max().item()
    torch.testing.assert_close(dx.double().cpu(), dxr.cpu(), rtol=tol["rtol"], atol=tol["atol"] * scale)
    assert dg.item() == pytest.approx(dgr.item(), rel=1e-4 if dtype == torch.float32 else 1e-2)
    # accumulate, and bit-identical on a second run
    dg2 = torch.full((1,), 0.5, device="cuda")
    dx2 = dres.clone() if dres is not None else torch.empty_like(x)
    K.scalenorm_bwd(dy, x, rinv, g, dx2 if dres is not None else None, dx2, dg2, R, H, ws, accumulate=True)
    assert dg2.item() == pytest.approx(0.5 + dg.item(), rel=1e-6)
    dg3 = torch.zeros(1, device="cuda")
    K.scalenorm_bwd(dy, x, rinv, g, None, torch.empty_like(x), dg3, R, H, ws)
    assert dg3.item() == dg.item()
    assert torch.equal(dx2, dx)


def test_scalenorm_module_forward_runs_the_kernel():
    from multi_modal.mm_utils import ScaleNorm, hip_layernorm
    m = ScaleNorm(16.0).cuda()
    x = torch.randn(3, 50, 256, device="cuda")
    want = x.double() * 16.0 / x.double().norm(dim=-1, keepdim=True).clamp(min=EPS)
    torch.testing.assert_close(m(x).double(), want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(hip_layernorm(x, m), m(x), rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------- folded bf16 kernels
def bf(t):
    return t.to(torch.bfloat16)


def prep_scalar_gain(W, g, bias):
    N, Kd = W.shape
    Wp = torch.zeros(N, Kd, dtype=torch.bfloat16, device="cuda")
    WpT = torch.zeros(Kd, N, dtype=torch.bfloat16, device="cuda")
    bp = torch.zeros(N, device="cuda")
    table, n, tiles = K.prep_table([dict(W=W, gamma=g, scalar_gain=True, bias=bias, Wp=Wp, WpT=WpT, bp=bp)], "cuda")
    K.prep_weights(table, n, tiles)
    torch.cuda.synchronize()
    return Wp, WpT, bp


def test_prep_weights_scalar_gain():
    W = torch.randn(768, 256, device="cuda") * 0.05
    g = torch.tensor([1.7], device="cuda")
    bias = torch.randn(768, device="cuda")
    Wp, WpT, bp = prep_scalar_gain(W, g, bias)
    assert torch.equal(Wp, bf(W * g))
    assert torch.equal(WpT, Wp.t())
    assert torch.equal(bp, bias)


@pytest.mark.parametrize("R,N", [(1000, 768), (1000, 256), (20000, 512)])
def test_rowgemm_scalenorm_prologue(R, N):
    """ln = 2: y = x_hat . Wp^T + bp with x_hat = x / max(||x||, eps); R = 1000 takes the N-split column blocks (few row passes),
    R = 20000 one block per row pass; every row checked, guard rows untouched."""
    x = bf(sn_rows_input(R, 256, torch.float32, 1))
    W = torch.randn(N, 256, device="cuda") * 0.06
    g = torch.tensor([15.0], device="cuda")
    bias = torch.randn(N, device="cuda") * 0.1
    Wp, _, bp = prep_scalar_gain(W, g, bias)
    pad = 64
    y = torch.full((R + pad, N), 5.0, dtype=torch.bfloat16, device="cuda")
    xh = torch.full((R + pad, 256), 5.0, dtype=torch.bfloat16, device="cuda")
    rs = torch.full((R + pad,), 5.0, device="cuda")
    K.rowgemm(x, Wp, y, R, N, 256, bias=bp, ln=2, xhat=xh, rstd=rs)
    torch.cuda.synchronize()
    xd = x.double()
    n = xd.norm(dim=-1)
    xhr = xd / n.clamp(min=EPS)[:, None]
    assert (y[R:] == 5.0).all() and (xh[R:] == 5.0).all() and (rs[R:] == 5.0).all()
    torch.testing.assert_close(rs[:R].abs().double(), 1.0 / n.clamp(min=EPS), rtol=1e-5, atol=0)
    assert ((rs[:R] < 0) == (n <= EPS)).all()
    torch.testing.assert_close(xh[:R].double(), xhr, rtol=1e-2, atol=1e-3)
    want = xh[:R].double() @ Wp.double().t() + bp.double()          # the kernel multiplies the rounded x_hat
    torch.testing.assert_close(y[:R].double(), want, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("Kd", [256, 512, 768])
def test_rowgemm_scalenorm_backward_epilogue(Kd):
    """ln_bwd = 2: y = res + |rs| (v - x_hat sum(v x_hat)), v = dY . w^T, the sum dropped where rs < 0 (clamped rows)."""
    R = 3000
    gen = torch.Generator().manual_seed(2)
    dY = bf(torch.randn(R, Kd, generator=gen) * 0.1).cuda()
    w = bf(torch.randn(256, Kd, generator=gen) * 0.05).cuda()
    xr = torch.randn(R, 256, generator=gen)
    xh = bf(xr / xr.norm(dim=-1, keepdim=True)).cuda()
    rs = (0.5 + torch.rand(R, generator=gen)).cuda()
    rs[::97] *= -1.0                                                 # clamped rows
    res = bf(torch.randn(R, 256, generator=gen) * 0.1).cuda()
    pad = 64
    y = torch.full((R + pad, 256), 5.0, dtype=torch.bfloat16, device="cuda")
    K.rowgemm(dY, w, y, R, 256, Kd, residual=res, ldr=256, ln_bwd=2, bwd_xhat=xh, bwd_rstd=rs)
    torch.cuda.synchronize()
    v = dY.double() @ w.double().t()
    xd = xh.double()
    s2 = (v * xd).sum(-1, keepdim=True)
    s2[rs < 0] = 0
    want = res.double() + rs.abs().double()[:, None] * (v - xd * s2)
    assert (y[R:] == 5.0).all()
    err = (y[:R].double() - want).abs().max().item()
    assert err < 2e-2 * want.abs().max().item(), err


def test_mlp_fwd_scalenorm_prologue():
    R = 2000
    x = bf(sn_rows_input(R, 256, torch.float32, 4))
    Wu, bu = torch.randn(512, 256, device="cuda") * 0.06, torch.randn(512, device="cuda") * 0.1
    Wd, bd = torch.randn(256, 512, device="cuda") * 0.04, torch.randn(256, device="cuda") * 0.1
    g = torch.tensor([16.0], device="cuda")
    Wp = torch.zeros(512, 256, dtype=torch.bfloat16, device="cuda")
    bp = torch.zeros(512, device="cuda")
    WdP = torch.zeros(256, 512, dtype=torch.bfloat16, device="cuda")
    table, n, tiles = K.prep_table([dict(W=Wu, gamma=g, scalar_gain=True, bias=bu, Wp=Wp, bp=bp), dict(W=Wd, WpP=WdP)], "cuda")
    K.prep_weights(table, n, tiles)
    pad = 128
    y = torch.full((R + pad, 256), 5.0, dtype=torch.bfloat16, device="cuda")
    xh = torch.full((R + pad, 256), 5.0, dtype=torch.bfloat16, device="cuda")
    rs = torch.full((R + pad,), 5.0, device="cuda")
    K.mlp_fwd(K.mlp_desc(R, x=x, w_up=Wp, b_up=bp, w_down=WdP, b_down=bd, y=y, xhat=xh, rstd=rs, scalenorm=True))
    torch.cuda.synchronize()
    xd = x.double()
    n = xd.norm(dim=-1)
    assert (y[R:] == 5.0).all() and (xh[R:] == 5.0).all() and (rs[R:] == 5.0).all()
    torch.testing.assert_close(rs[:R].abs().double(), 1.0 / n.clamp(min=EPS), rtol=1e-5, atol=0)
    assert ((rs[:R] < 0) == (n <= EPS)).all()
    u = xh[:R].double() @ Wp.double().t() + bp.double()
    want = xd + F.gelu(u) @ bf(Wd).double().t() + bd.double()
    err = (y[:R].double() - want).abs().max().item()
    assert err < 2e-2 * want.abs().max().item(), err
    # the one-launch backward refuses ScaleNorm (the engine always splits)
    d = K.mlp_desc(R, w_up=Wp, b_up=bp, xhat=xh, rstd=rs, dy=y, w_down_t=Wp, w_up_t=Wp, t1=y, g=y, du=y, dx=y, scalenorm=True)
    with pytest.raises(L.MmfmError):
        K.mlp_bwd(d)


@pytest.mark.parametrize("N", [256, 768])
def test_sn_linear_grad(N):
    Kd = 256
    gen = torch.Generator().manual_seed(5)
    Gdb = torch.randn(N * Kd + N, generator=gen).cuda()
    W = (torch.randn(N, Kd, generator=gen) * 0.05).cuda()
    g = torch.tensor([3.0], device="cuda")
    ws = K.ln_linear_grad_workspace(Kd, "cuda")
    dW, db, dg = torch.empty(N, Kd, device="cuda"), torch.empty(N, device="cuda"), torch.zeros(1, device="cuda")
    K.sn_linear_grad(Gdb, W, g, N, Kd, dW, db, dg, ws)
    G = Gdb[:N * Kd].view(N, Kd)
    assert torch.equal(dW, G * g) and torch.equal(db, Gdb[N * Kd:])
    assert dg.item() == pytest.approx(float((W.double() * G.double()).sum()), rel=1e-5, abs=1e-6)
    dg2 = torch.full((1,), 0.25, device="cuda")
    K.sn_linear_grad(Gdb, W, g, N, Kd, dW, db, dg2, ws, accumulate=True)
    assert dg2.item() == pytest.approx(0.25 + dg.item(), rel=1e-6)
    dg3 = torch.zeros(1, device="cuda")
    K.sn_linear_grad(Gdb, W, g, N, Kd, dW, db, dg3, ws)
    assert dg3.item() == dg.item()                                   # deterministic


# ---------------------------------------------------------------------------------------------- models, fp32 against the reference
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = load_npz("scalenorm_fwd_bwd.npz")
    return _Z


@pytest.mark.parametrize("variant", ["base", "pad", "sep", "deep"])
@pytest.mark.parametrize("objective", ["encoding", "decoding", "token_masking"])
def test_tiny_scalenorm_forward_backward_vs_reference_fixture(variant, objective):
    """The model is rebuilt from the fixture's seed (tests/test_scalenorm_cpu.py pins that rebuild to the reference's initial
    state dict bit for bit); every gradient tensor is compared where the fixture keeps it, each `.scale` gradient and every
    gradient norm everywhere."""
    z, meta = fixture()
    model = build_model(tiny_config(scalenorm=True, **meta["variants"][variant]), meta["n_ap"], meta["n_beh"], seed=meta["model_seed"])
    stored = check_fixture_case(model, z, meta, variant, objective, prefix=f"{variant}/batch/")
    assert sum(k.endswith(".scale") for k in stored) == (12 if variant == "deep" else 6)


def test_scalenorm_loss_curve_tiny_50_steps_vs_reference_fixture():
    g = load_json("scalenorm_curve.json")["tiny"]
    model = build_model(tiny_config(scalenorm=True), g["n_ap"], g["n_beh"], seed=g["model_seed"]).cuda()
    losses = run_curve(model, 50, g["B"], g["T"], g["n_ap"], g["n_beh"], g["total_steps"], g["objective"])
    np.testing.assert_allclose(losses, g["loss"], rtol=1e-4)


def test_scalenorm_default_config_scalars_vs_reference_fixture():
    g = load_json("scalenorm_curve.json")["default"]
    model = build_model(model_config(dropout=0.0, emb_dropout=0.0, scalenorm=True), 668, 2, seed=42).cuda().eval()
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


# ---------------------------------------------------------------------------------------------- bf16, default widths: fused against un-fused
@pytest.mark.parametrize("B", [16, 1024])
def test_bf16_scalenorm_fused_path_matches_unfused_kernels(monkeypatch, B):
    g = load_json("scalenorm_curve.json")["default"]
    batch = O.synth_batch(B, 100, 668, 2, seed=0)
    calls = {}

    def counting(name, fn):
        def wrapped(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        return wrapped
    res = {}
    for mode in ("0", "15"):
        monkeypatch.setenv("MMFM_FUSED", mode)
        calls.clear()
        with monkeypatch.context() as mp:        # count the plan's stand-alone ScaleNorm calls and the row-owner ScaleNorm launches
            mp.setattr(K, "scalenorm_fwd", counting("sn_fwd", K.scalenorm_fwd))
            mp.setattr(K, "scalenorm_bwd", counting("sn_bwd", K.scalenorm_bwd))
            mp.setattr(K, "sn_linear_grad", counting("sn_lin", K.sn_linear_grad))
            rowgemm = K.rowgemm
            mp.setattr(K, "rowgemm", lambda *a, **kw: (calls.__setitem__("rg_sn", calls.get("rg_sn", 0) + (kw.get("ln") == 2 or kw.get("ln_bwd") == 2)),
                                                       rowgemm(*a, **kw))[1])
            model = build_model(model_config(dropout=0.0, emb_dropout=0.0, scalenorm=True), 668, 2, seed=42)
            model.compute_dtype = "bf16"
            model.cuda().train()
            out = {}
            for obj in ("encoding", "token_masking"):
                model.zero_grad(set_to_none=True)
                torch.manual_seed(1)
                o = model(to_dev(O.make_mod_dict(batch, obj)))
                o.loss.backward()
                out[obj] = (o.loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
        assert model._engine._fused_mask(B * 200) == int(mode)
        if mode == "15":         # every ScaleNorm site folded into the row-owner kernels: no stand-alone ScaleNorm in the plan
            assert calls.get("sn_fwd", 0) == 0 and calls.get("sn_bwd", 0) == 0, calls
            assert calls.get("rg_sn", 0) > 0 and calls.get("sn_lin", 0) > 0, calls
        else:
            assert calls.get("sn_fwd", 0) > 0 and calls.get("sn_bwd", 0) > 0 and calls.get("rg_sn", 0) == 0, calls
        res[mode] = out
        del model
        torch.cuda.empty_cache()
    for obj in ("encoding", "token_masking"):
        l0, g0 = res["0"][obj]
        l1, g1 = res["15"][obj]
        assert l1 == pytest.approx(l0, rel=3e-3)
        if B == 16:
            assert l1 == pytest.approx(g[obj]["loss"], rel=2e-2)
        dg_max = max(g0[k].abs().item() for k in g0 if k.endswith(".scale"))
        for k in g0:
            if k.endswith(".scale"):
                assert abs(g1[k].item() - g0[k].item()) < 5e-2 * dg_max, f"{obj} {k}: {g1[k].item()} vs {g0[k].item()} (max |dg| {dg_max})"
                continue
            if g0[k].abs().max() == 0:
                assert g1[k].abs().max() == 0, k
                continue
            if k.endswith("key.bias"):
                continue
            c = cosine(g0[k], g1[k])
            assert c > (0.995 if g0[k].numel() >= 256 else 0.98), f"{obj} {k}: cosine {c}"
            n0, n1 = g0[k].double().norm().item(), g1[k].double().norm().item()
            assert n1 == pytest.approx(n0, rel=5e-2), f"{obj} {k}: norm {n1} vs {n0}"


# ---------------------------------------------------------------------------------------------- training
def test_bf16_scalenorm_trains_with_dropout(monkeypatch):
    monkeypatch.setenv("MMFM_FUSED", "15")
    model = build_model(model_config(n_enc=2, n_dec=2, scalenorm=True), 668, 2, seed=3)
    model.compute_dtype = "bf16"
    model.engine_seed = 11
    model.cuda().train()
    opt, sch = make_optimizer(model, 20, lr=5e-4)
    torch.manual_seed(5)
    losses = []
    for s in range(5):
        batch = O.synth_batch(5, 100, 668, 2, seed=s % 2, pad=[0, 10, 0, 37, 1])
        out = model(to_dev(O.make_mod_dict(batch, "encoding")))
        out.loss.backward()
        opt.step(); sch.step(); opt.zero_grad()
        losses.append(out.loss.item())
    assert np.isfinite(losses).all(), losses
    scales = [p.item() for k, p in model.named_parameters() if k.endswith(".scale")]
    assert len(scales) == 12 and np.isfinite(scales).all() and any(s != 16.0 for s in scales)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scalenorm_resume_from_train_state_is_bit_identical(tmp_path, dtype):
    """6 steps in one go == 3 steps, save_model (module pickle + train state), fresh objects restored from the files, 3 more steps;
    dropout on (engine RNG), sampled objectives (Python RNG), token masks (torch RNG)."""
    def after_restore(m2, opt2, sch2):
        assert any(k.endswith(".scale") for k in m2.state_dict())

    resume_roundtrip(tmp_path, tiny_config(n_enc=2, n_dec=2, dropout=0.4, emb_dropout=0.2, scalenorm=True), dtype=dtype, after_restore=after_restore)
