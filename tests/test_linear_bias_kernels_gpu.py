"""Bias-free linears (attention_bias / mlp_bias: false) through the C-ABI, kernel by kernel, against torch fp64: mmfm_rowgemm with
bias = None, mmfm_mlp_fwd / mmfm_mlp_bwd with b_down (and, behind a ScaleNorm, b_up) = None, mmfm_prep_weights with a NULL bias,
mmfm_ln_linear_grad / mmfm_sn_linear_grad with dbias = None.

Tolerances are the ones tests/test_rowchain_gpu.py states for the same kernel and dtype (relative L2 over the tensor: plain row GEMM
4e-3, norm-fed 6e-3, MLP forward / g 6e-3, du / dx 1.2e-2; fp32 gradient kernels rtol 1e-4).  The ScaleNorm prologue (ln = 2) has no
case there; it differs from ln = 1 only in the statistic (x_hat is rounded to bf16 once in both), so it takes the ln = 1 bound."""
import pytest
import torch
import torch.nn.functional as F

from multi_modal_foundation_model_amd import _lib as L
from multi_modal_foundation_model_amd import ops as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EPS = 1e-5


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def check(a, b, rel, msg):
    a, b = a.double().cpu(), b.double().cpu()
    r = float((a - b).norm() / (b.norm() + 1e-30))
    print(f"{msg}: relative L2 error {r:.3e} (bound {rel})")
    assert r < rel, f"{msg}: relative L2 error {r:.3e} >= {rel}"


def prep(entries):
    table, n, tiles = K.prep_table(entries, "cuda")
    K.prep_weights(table, n, tiles)
    torch.cuda.synchronize()


def norm_hat(xd, sn):
    if sn:
        return xd / xd.norm(dim=-1, keepdim=True).clamp(min=EPS)
    return F.layer_norm(xd, (xd.shape[-1],), None, None, EPS)


# ---------------------------------------------------------------------------------------------- mmfm_rowgemm
# R: 96 a ragged single pass (128 rows per pass), 160 more than one pass, 416 four passes.  At these sizes the K = 256 forward kernels
# split N into column blocks (fewer than 128 passes); N = 768 without a residual gives 512 / npass >= 12 = every pair its own block.
@pytest.mark.parametrize("R", [96, 160, 416])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("mode", ["plain", "ln1", "ln2", "residual"])
def test_rowgemm_without_bias(mode, N, R):
    x = (rnd(R, 256, seed=1) * 2 + rnd(R, 1, seed=5) * 3).to(BF)
    W = rnd(N, 256, seed=2, scale=1 / 16)
    res = rnd(R, N, seed=4).to(BF) if mode == "residual" else None
    ln = {"plain": 0, "residual": 0, "ln1": 1, "ln2": 2}[mode]
    Wp = torch.empty(N, 256, device="cuda", dtype=BF)
    if ln == 1:
        gamma = 1 + 0.3 * rnd(256, seed=3)
        prep([dict(W=W, gamma=gamma, Wp=Wp)])
        Wref = W.double() * gamma.double()
    elif ln == 2:
        gain = torch.tensor([15.0], device="cuda")
        prep([dict(W=W, gamma=gain, scalar_gain=True, Wp=Wp)])          # bias-free behind a ScaleNorm: no bp at all
        Wref = W.double() * 15.0
    else:
        prep([dict(W=W, Wp=Wp)])
        Wref = Wp.double()
    pad = 3
    y = torch.full((R + pad, N), 7.0, device="cuda", dtype=BF)
    xh = torch.full((R + pad, 256), 7.0, device="cuda", dtype=BF) if ln else None
    rs = torch.full((R + pad,), 7.0, device="cuda") if ln else None
    kw = dict(ln=ln, xhat=xh, rstd=rs, residual=res, ldr=N if res is not None else 0)
    K.rowgemm(x, Wp, y, R, N, 256, bias=None, **kw)
    torch.cuda.synchronize()
    xd = x.double()
    ref = (norm_hat(xd, ln == 2) if ln else xd) @ Wref.T + (res.double() if res is not None else 0.0)
    check(y[:R], ref, 6e-3 if ln else 4e-3, f"rowgemm bias=None {mode} {R}x{N}")
    assert torch.all(y[R:] == 7.0)
    if ln:
        assert torch.all(xh[R:] == 7.0) and torch.all(rs[R:] == 7.0)
        check(xh[:R], norm_hat(xd, ln == 2), 3e-3, "x_hat")
    # "adds nothing": bit-identical to an explicit zero bias
    y0 = torch.empty(R, N, device="cuda", dtype=BF)
    kw0 = dict(kw, xhat=torch.empty(R, 256, device="cuda", dtype=BF) if ln else None, rstd=torch.empty(R, device="cuda") if ln else None)
    K.rowgemm(x, Wp, y0, R, N, 256, bias=torch.zeros(N, device="cuda"), **kw0)
    torch.cuda.synchronize()
    assert torch.equal(y0, y[:R])


# ---------------------------------------------------------------------------------------------- mmfm_prep_weights
def test_prep_weights_null_bias_folds_beta_only():
    W, gamma, beta = rnd(96, 256, seed=1), rnd(256, seed=2), rnd(256, seed=3)
    Wp, bp = torch.empty(96, 256, device="cuda", dtype=BF), torch.full((96 + 8,), 7.0, device="cuda")
    prep([dict(W=W, gamma=gamma, beta=beta, bias=None, Wp=Wp, bp=bp[:96])])
    assert torch.equal(Wp, (W * gamma).to(BF))
    torch.testing.assert_close(bp[:96].double(), W.double() @ beta.double(), rtol=1e-5, atol=1e-5)
    assert torch.all(bp[96:] == 7.0)
    # scalar gain, no bias: bp = NULL is accepted and nothing is written; a bp that is given comes out as zeros
    gain = torch.tensor([1.7], device="cuda")
    bp2 = torch.full((96,), 7.0, device="cuda")
    Wp2 = torch.empty(96, 256, device="cuda", dtype=BF)
    prep([dict(W=W, gamma=gain, scalar_gain=True, Wp=Wp), dict(W=W, gamma=gain, scalar_gain=True, Wp=Wp2, bp=bp2)])
    assert torch.equal(Wp, (W * gain).to(BF)) and torch.equal(Wp2, Wp)
    assert torch.all(bp2 == 0.0)


# ---------------------------------------------------------------------------------------------- mmfm_mlp_fwd / mmfm_mlp_bwd
def mlp_setup(R, sn, seed):
    x = (rnd(R, 256, seed=seed + 1) * 1.5 + rnd(R, 1, seed=seed + 2)).to(BF)
    Wu, Wd = rnd(512, 256, seed=seed + 3, scale=1 / 16), rnd(256, 512, seed=seed + 5, scale=1 / 22)
    mk = lambda *s: torch.empty(*s, device="cuda", dtype=BF)
    up = dict(W=Wu, Wp=mk(512, 256), WpT=mk(256, 512), WpTP=mk(256, 512))
    if sn:
        up.update(gamma=torch.tensor([16.0], device="cuda"), scalar_gain=True, bp=None)
        w = dict(gain=16.0)
    else:
        gamma, beta = 1 + 0.3 * rnd(256, seed=seed + 7), 0.2 * rnd(256, seed=seed + 8)
        up.update(gamma=gamma, beta=beta, bias=None, bp=torch.empty(512, device="cuda"))      # bp = W_up . beta
        w = dict(gamma=gamma.double(), beta=beta.double())
    dn = dict(W=Wd, WpP=mk(256, 512), WpT=mk(512, 256))
    prep([up, dn])
    w.update(Wu=Wu.double(), Wd=Wd.double())
    return x, up, dn, w


def mlp_ref(x, w, sn, mask, dy):
    """fp64 autograd of y = x + mask * (gelu(up(norm(x))) . W_down^T), no bias anywhere but the folded beta."""
    xd = x.double().requires_grad_(True)
    if sn:
        h = w["gain"] * norm_hat(xd, True)
    else:
        h = F.layer_norm(xd, (256,), w["gamma"], w["beta"], EPS)
    u = h @ w["Wu"].T
    g = F.gelu(u)
    out = xd + (g @ w["Wd"].T) * mask
    u.retain_grad()
    out.backward(dy.double())
    return out.detach(), g.detach(), u.grad, xd.grad


@pytest.mark.parametrize("R", [96, 416])
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("norm", ["layernorm", "scalenorm"])
def test_mlp_without_bias(norm, p, R):
    """LayerNorm: b_down = None, b_up = the prepared W_up . beta.  ScaleNorm: b_up = b_down = None.  Forward, the one-launch backward
    (LayerNorm only: it has no ScaleNorm epilogue) and the front half + mmfm_rowgemm(ln_bwd).  Under dropout the reference takes the
    keep decisions from the backward's t1 = dropout'(dy); that the forward used the same ones is what its check against that reference
    shows (a dropped element leaves y = x exactly)."""
    sn = norm == "scalenorm"
    x, up, dn, w = mlp_setup(R, sn, seed=40)
    drop = None
    if p > 0:
        state = torch.zeros(2, dtype=torch.int32, device="cuda")
        K.rng_seed(state, 5)
        drop = K.dropout(state, 9, p)
    pad = 2
    y = torch.full((R + pad, 256), 3.0, device="cuda", dtype=BF)
    xhat, rstd = torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    K.mlp_fwd(K.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=None, y=y, xhat=xhat, rstd=rstd, drop=drop,
                         scalenorm=sn))
    dy = rnd(R, 256, seed=77).to(BF)
    assert not (dy == 0).any()
    modes = ["split"] if sn else ["one", "split"]
    outs = {}
    for mode in modes:
        mk = lambda n: torch.full((R + 1, n), 5.0, device="cuda", dtype=BF)
        t1, gg, du, dx = mk(256), mk(512), mk(512), mk(256)
        K.mlp_bwd(K.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], drop=drop, xhat=xhat, rstd=rstd, dy=dy, w_down_t=dn["WpT"], w_up_t=up["WpTP"],
                             t1=t1, g=gg, du=du, dx=dx if mode == "one" else None, scalenorm=sn))
        if mode == "split":
            K.rowgemm(du, up["WpT"], dx, R, 256, 512, ldw=512, residual=dy, ldr=256, ln_bwd=2 if sn else 1, bwd_xhat=xhat, bwd_rstd=rstd)
        torch.cuda.synchronize()
        for b in (t1, gg, du, dx):
            assert torch.all(b[R:] == 5.0)
        outs[mode] = (t1[:R], gg[:R], du[:R], dx[:R])
    t1 = outs["split"][0]
    if p == 0:
        assert torch.equal(t1, dy)
        mask = torch.ones(R, 256, device="cuda", dtype=torch.float64)
    else:
        kept = t1 != 0
        assert 0.57 < kept.float().mean().item() < 0.63
        torch.testing.assert_close(t1.float()[kept], (dy.float() / (1 - p))[kept], rtol=1e-2, atol=1e-3)
        mask = kept.double() / (1 - p)
        assert torch.equal(y[:R][~kept], x[~kept])                       # the forward dropped exactly these
    out, g_ref, du_ref, dx_ref = mlp_ref(x, w, sn, mask, dy)
    assert torch.all(y[R:] == 3.0)
    check(y[:R], out, 6e-3, f"mlp fwd {norm} p={p} R={R}")
    for mode, (t1m, gg, du, dx) in outs.items():
        assert torch.equal(t1m, t1)
        check(gg, g_ref, 6e-3, f"g ({mode})")
        check(du, du_ref, 1.2e-2, f"du ({mode})")
        check(dx, dx_ref, 1.2e-2, f"dx ({mode})")
    if len(outs) == 2:            # same operands, same MFMA order: the front half is the one-launch kernel's bit for bit
        assert torch.equal(outs["one"][1], outs["split"][1]) and torch.equal(outs["one"][2], outs["split"][2])


def test_mlp_null_b_up_needs_scalenorm():
    x, up, dn, w = mlp_setup(96, False, seed=3)
    y, xhat, rstd = torch.empty(96, 256, device="cuda", dtype=BF), torch.empty(96, 256, device="cuda", dtype=BF), torch.empty(96, device="cuda")
    with pytest.raises(L.MmfmError):
        K.mlp_fwd(K.mlp_desc(96, x=x, w_up=up["Wp"], b_up=None, w_down=dn["WpP"], b_down=None, y=y, xhat=xhat, rstd=rstd))


# ---------------------------------------------------------------------------------------------- norm-fed linear gradients
def test_ln_linear_grad_without_dbias():
    """y = LayerNorm(x) W^T (no bias): dW, dgamma, dbeta from Gdb = [dY^T x_hat | colsum dY] - db stays in Gdb, beta being folded into
    the linear - and nothing is written where a bias gradient would sit behind dW."""
    R, N, Kd = 700, 96, 256
    x = (rnd(R, Kd, seed=1) * 1.3 + 0.4).double()
    W, g, bt = (rnd(N, Kd, seed=2, scale=1 / 16).double().requires_grad_(True), (1 + 0.3 * rnd(Kd, seed=4)).double().requires_grad_(True),
                (0.2 * rnd(Kd, seed=5)).double().requires_grad_(True))
    dY = rnd(R, N, seed=6).double()
    (F.layer_norm(x, (Kd,), g, bt, EPS) @ W.T).backward(dY)
    xhat = F.layer_norm(x, (Kd,), None, None, EPS)
    Gdb = torch.cat([(dY.T @ xhat).flatten(), dY.sum(0)]).float().contiguous()
    flat = torch.full((N * Kd + N,), -77.0, device="cuda")
    dW = flat[:N * Kd].view(N, Kd)
    dg, dbt = torch.ones(Kd, device="cuda"), torch.ones(Kd, device="cuda")
    ws = K.ln_linear_grad_workspace(Kd, "cuda")
    f32 = lambda t: t.detach().float().contiguous()
    K.ln_linear_grad(Gdb, f32(W), f32(g), f32(bt), N, Kd, dW, None, dg, dbt, ws)
    torch.cuda.synchronize()
    torch.testing.assert_close(dW.double(), W.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dg.double(), g.grad, rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(dbt.double(), bt.grad, rtol=1e-4, atol=2e-4)
    assert torch.all(flat[N * Kd:] == -77.0)
    # with a dbias the same launch is unchanged
    dW2, db2 = torch.empty(N, Kd, device="cuda"), torch.empty(N, device="cuda")
    dg2, dbt2 = torch.ones(Kd, device="cuda"), torch.ones(Kd, device="cuda")
    K.ln_linear_grad(Gdb, f32(W), f32(g), f32(bt), N, Kd, dW2, db2, dg2, dbt2, ws)
    torch.cuda.synchronize()
    assert torch.equal(dW2, dW) and torch.equal(dg2, dg) and torch.equal(dbt2, dbt) and torch.equal(db2, Gdb[N * Kd:])


@pytest.mark.parametrize("N", [256, 768])
def test_sn_linear_grad_without_dbias_reads_no_db_block(N):
    """y = (g x_hat) W^T: dW = g G, dg = sum W * G against autograd, from a Gdb that holds G alone (N * K floats)."""
    R, Kd = 300, 256
    x = (rnd(R, Kd, seed=1) * 1.3 + 0.4).double()
    W = rnd(N, Kd, seed=2, scale=1 / 16).double().requires_grad_(True)
    g = torch.tensor([3.0], device="cuda", dtype=torch.float64, requires_grad=True)
    dY = rnd(R, N, seed=6).double()
    xhat = norm_hat(x, True)
    ((g * xhat) @ W.T).backward(dY)
    G = (dY.T @ xhat).float().contiguous()
    assert G.numel() == N * Kd
    flat = torch.full((N * Kd + N,), -77.0, device="cuda")
    dW, dg = flat[:N * Kd].view(N, Kd), torch.zeros(1, device="cuda")
    ws = K.ln_linear_grad_workspace(Kd, "cuda")
    K.sn_linear_grad(G, W.detach().float().contiguous(), g.detach().float(), N, Kd, dW, None, dg, ws)
    torch.cuda.synchronize()
    torch.testing.assert_close(dW.double(), W.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dg.double(), g.grad, rtol=1e-4, atol=2e-4)
    assert torch.all(flat[N * Kd:] == -77.0)
