"""Row-owner fused kernels (mmfm_prep_weights, mmfm_rowgemm, mmfm_mlp_fwd/bwd, mmfm_ln_linear_grad) against a torch
fp64 reference of the same ops on the same bf16-rounded inputs.  bf16 storage: outputs carry one bf16 rounding
(2^-9 relative) plus the rounding of in-kernel bf16 intermediates (x_hat, gelu output, du); tolerances are stated per check."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30)), float((a - b).abs().max()), float(b.abs().max())


def check(a, b, rel, msg):
    r, mx, ref = relerr(a, b)
    assert r < rel, f"{msg}: relative L2 error {r:.3e} (max abs {mx:.3e}, ref max {ref:.3e}) >= {rel}"


def prep(ops, W, gamma=None, beta=None, bias=None, want_T=True):
    N, K = W.shape
    e = dict(W=W, gamma=gamma, beta=beta, bias=bias, Wp=torch.empty(N, K, device="cuda", dtype=BF),
             WpT=torch.empty(K, N, device="cuda", dtype=BF) if want_T else None, bp=torch.empty(N, device="cuda"),
             WpP=torch.empty(N, K, device="cuda", dtype=BF), WpTP=torch.empty(K, N, device="cuda", dtype=BF))
    table, n, tiles = ops.prep_table([e], "cuda")
    ops.prep_weights(table, n, tiles)
    torch.cuda.synchronize()
    return e


def test_prep_weights_folds_layernorm_affine(ops):
    W, g, b, bias = rnd(96, 256, seed=1), rnd(256, seed=2), rnd(256, seed=3), rnd(96, seed=4)
    e = prep(ops, W, g, b, bias)
    ref = (W * g).to(BF)
    assert torch.equal(e["Wp"], ref) and torch.equal(e["WpT"], ref.T.contiguous())
    torch.testing.assert_close(e["bp"], bias + W @ b, rtol=1e-5, atol=1e-5)
    # unit-permuted copies (the order an accumulator tile holds its k index in): 4-element units 1 and 2 of every 16 swap places
    def unit_perm(t):
        return t.reshape(t.shape[0], -1, 4, 4)[:, :, [0, 2, 1, 3], :].reshape(t.shape)
    assert torch.equal(e["WpP"], unit_perm(ref)) and torch.equal(e["WpTP"], unit_perm(ref.T.contiguous()))
    # several entries in one launch, ragged N
    es = [dict(W=rnd(n, k, seed=9 + i), Wp=torch.empty(n, k, device="cuda", dtype=BF), WpT=torch.empty(k, n, device="cuda", dtype=BF))
          for i, (n, k) in enumerate([(256, 512), (40, 256), (768, 256)])]
    table, n, tiles = ops.prep_table(es, "cuda")
    ops.prep_weights(table, n, tiles)
    for e in es:
        assert torch.equal(e["Wp"], e["W"].to(BF)) and torch.equal(e["WpT"], e["W"].to(BF).T.contiguous())


@pytest.mark.parametrize("R,N,K", [(128, 256, 256), (1000, 768, 256), (4096 + 40, 512, 256), (300, 256, 512), (517, 256, 768), (33, 64, 256)])
def test_rowgemm_plain(ops, R, N, K):
    x, W, b = rnd(R, K, seed=1).to(BF), rnd(N, K, seed=2, scale=K ** -0.5).to(BF), rnd(N, seed=3)
    res = rnd(R, N, seed=4).to(BF)
    y = torch.full((R + 3, N), 7.0, device="cuda", dtype=BF)          # guard rows must stay untouched
    ops.rowgemm(x, W, y, R, N, K, bias=b, residual=res, ldr=N)
    ref = x.double() @ W.double().T + b.double() + res.double()
    check(y[:R], ref, 4e-3, f"rowgemm {R}x{N}x{K}")
    assert torch.all(y[R:] == 7.0)
    ops.rowgemm(x, W, y, R, N, K, stream_out=True)
    check(y[:R], x.double() @ W.double().T, 4e-3, f"rowgemm no-epilogue {R}x{N}x{K}")


@pytest.mark.parametrize("R,N", [(256, 768), (1000, 256), (77, 512)])
def test_rowgemm_layernorm_prologue(ops, R, N):
    x = (rnd(R, 256, seed=1) * 2 + rnd(R, 1, seed=5) * 3).to(BF)       # non-zero row means
    W, g, bt, bias = rnd(N, 256, seed=2, scale=1 / 16), 1 + 0.3 * rnd(256, seed=3), 0.2 * rnd(256, seed=4), rnd(N, seed=6)
    e = prep(ops, W, g, bt, bias)
    y, xhat, rstd = (torch.empty(R, N, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda"))
    res = rnd(R, N, seed=7).to(BF)
    ops.rowgemm(x, e["Wp"], y, R, N, 256, bias=e["bp"], ln=True, xhat=xhat, rstd=rstd, residual=res, ldr=N)
    xd = x.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    xh_ref = (xd - mu) / torch.sqrt(var + 1e-5)
    check(xhat, xh_ref, 3e-3, "x_hat")
    torch.testing.assert_close(rstd.double(), (1 / torch.sqrt(var + 1e-5)).squeeze(1), rtol=1e-5, atol=1e-6)
    ref = F.layer_norm(xd, (256,), g.double(), bt.double(), 1e-5) @ W.double().T + bias.double() + res.double()
    check(y, ref, 6e-3, f"ln+linear {R}x{N}")
    # without a residual the launch takes the LDS-DMA ring kernel, which at these sizes splits N into column blocks: x_hat / rstd are
    # written by column block 0 only and must still be complete, every block's columns must land, nothing beyond R may be touched
    y2, xhat2, rstd2 = (torch.full((R + 2, N), 9.0, device="cuda", dtype=BF), torch.full((R + 2, 256), 9.0, device="cuda", dtype=BF),
                        torch.full((R + 2,), 9.0, device="cuda"))
    ops.rowgemm(x, e["Wp"], y2, R, N, 256, bias=e["bp"], ln=True, xhat=xhat2, rstd=rstd2)
    check(y2[:R], ref - res.double(), 6e-3, f"ln+linear (column blocks) {R}x{N}")
    assert torch.equal(xhat2[:R], xhat) and torch.equal(rstd2[:R], rstd)
    assert torch.all(y2[R:] == 9.0) and torch.all(xhat2[R:] == 9.0) and torch.all(rstd2[R:] == 9.0)


@pytest.mark.parametrize("R,K", [(300, 256), (1000, 768), (129, 512)])
def test_rowgemm_layernorm_backward_epilogue(ops, R, K):
    """dx = dres + LayerNorm'(dy . Wp) for a linear [K out-features] fed by a LayerNorm over 256."""
    dy = rnd(R, K, seed=1).to(BF)
    W, g = rnd(K, 256, seed=2, scale=K ** -0.5), 1 + 0.3 * rnd(256, seed=3)
    x = rnd(R, 256, seed=4) * 1.7 + 0.5
    dres = rnd(R, 256, seed=5).to(BF)
    e = prep(ops, W, g, None, None)
    mu, var = x.double().mean(1, keepdim=True), x.double().var(1, unbiased=False, keepdim=True)
    rstd = (1 / torch.sqrt(var + 1e-5)).squeeze(1).float().contiguous()
    xhat = ((x.double() - mu) * rstd.double()[:, None]).to(BF).contiguous()
    dx = torch.empty(R, 256, device="cuda", dtype=BF)
    ops.rowgemm(dy, e["WpT"], dx, R, 256, K, ldw=K, residual=dres, ldr=256, ln_bwd=True, bwd_xhat=xhat, bwd_rstd=rstd)
    v = dy.double() @ e["Wp"].double()                                 # d x_hat
    xh = xhat.double()
    ref = dres.double() + rstd.double()[:, None] * (v - v.mean(1, keepdim=True) - xh * (v * xh).mean(1, keepdim=True))
    check(dx, ref, 5e-3, f"ln-bwd epilogue {R}x{K}")


def mlp_setup(ops, R, seed=0):
    x = (rnd(R, 256, seed=seed + 1) * 1.5 + rnd(R, 1, seed=seed + 2)).to(BF)
    Wu, bu = rnd(512, 256, seed=seed + 3, scale=1 / 16), 0.1 * rnd(512, seed=seed + 4)
    Wd, bd = rnd(256, 512, seed=seed + 5, scale=1 / 22), 0.1 * rnd(256, seed=seed + 6)
    g, bt = 1 + 0.3 * rnd(256, seed=seed + 7), 0.2 * rnd(256, seed=seed + 8)
    up = prep(ops, Wu, g, bt, bu)
    dn = prep(ops, Wd, None, None, bd)
    return x, Wu, bu, Wd, bd, g, bt, up, dn


@pytest.mark.parametrize("R", [128, 1000, 5000])
def test_mlp_forward(ops, R):
    x, Wu, bu, Wd, bd, g, bt, up, dn = mlp_setup(ops, R)
    y, xhat, rstd = torch.full((R + 2, 256), 3.0, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    d = ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y, xhat=xhat, rstd=rstd)
    ops.mlp_fwd(d)
    xd = x.double()
    h = F.layer_norm(xd, (256,), g.double(), bt.double(), 1e-5)
    ref = xd + F.gelu(h @ Wu.double().T + bu.double()) @ Wd.double().T + bd.double()
    check(y[:R], ref, 6e-3, f"mlp fwd R={R}")
    assert torch.all(y[R:] == 3.0)


def test_mlp_forward_dropout_matches_backward_mask(ops):
    """The forward's dropout mask (counter row*256 + col) is the one the backward regenerates: t1 = dropout'(dy) must be
    zero exactly where y - x is zero, and scaled by 1/(1-p) elsewhere."""
    R, p = 640, 0.4
    x, Wu, bu, Wd, bd, g, bt, up, dn = mlp_setup(ops, R, seed=20)
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 5)
    drop = ops.dropout(state, 9, p)
    y, xhat, rstd = torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    ops.mlp_fwd(ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y, xhat=xhat, rstd=rstd, drop=drop))
    y0 = torch.empty_like(y)
    ops.mlp_fwd(ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y0, xhat=xhat, rstd=rstd))
    kept = (y.float() - x.float()) != 0
    assert 0.57 < kept.float().mean().item() < 0.63
    ref = torch.where(kept, (y0.float() - x.float()) / (1 - p), torch.zeros((), device="cuda"))
    big = ref.abs() > 0.5                                              # away from bf16 cancellation noise of y - x
    torch.testing.assert_close((y.float() - x.float())[big], ref[big], rtol=0.05, atol=0.02)
    dy = torch.ones(R, 256, device="cuda", dtype=BF)
    t1, gg, du, dx = (torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, 512, device="cuda", dtype=BF),
                      torch.empty(R, 512, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF))
    ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], drop=drop, xhat=xhat, rstd=rstd, dy=dy, w_down_t=dn["WpT"], w_up_t=up["WpTP"],
                             t1=t1, g=gg, du=du, dx=dx))
    sure = (y0.float() - x.float()).abs() > 0.25                      # where "y == x" can only mean "dropped", not "rounded away"
    assert sure.float().mean().item() > 0.3
    torch.testing.assert_close(t1.float()[sure], (kept.float() / (1 - p))[sure], rtol=1e-2, atol=1e-2)
    assert 0.57 < (t1 != 0).float().mean().item() < 0.63


@pytest.mark.parametrize("R", [128, 1000])
def test_mlp_backward(ops, R):
    x, Wu, bu, Wd, bd, g, bt, up, dn = mlp_setup(ops, R, seed=40)
    y, xhat, rstd = torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    ops.mlp_fwd(ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y, xhat=xhat, rstd=rstd))
    dy = rnd(R, 256, seed=77).to(BF)
    t1, gg, du, dx = (torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, 512, device="cuda", dtype=BF),
                      torch.empty(R, 512, device="cuda", dtype=BF), torch.full((R + 1, 256), 5.0, device="cuda", dtype=BF))
    ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], xhat=xhat, rstd=rstd, dy=dy, w_down_t=dn["WpT"], w_up_t=up["WpTP"],
                             t1=t1, g=gg, du=du, dx=dx))
    assert torch.equal(t1, dy) and torch.all(dx[R:] == 5.0)
    xd = x.double().requires_grad_(True)
    h = F.layer_norm(xd, (256,), g.double(), bt.double(), 1e-5)
    u = h @ Wu.double().T + bu.double()
    gl = F.gelu(u)
    out = xd + gl @ Wd.double().T + bd.double()
    u.retain_grad(); gl.retain_grad()
    out.backward(dy.double())
    check(gg, gl.detach(), 6e-3, "g")
    check(du, u.grad, 1.2e-2, "du")
    check(dx[:R], xd.grad, 1.2e-2, "dx")


@pytest.mark.parametrize("R,p", [(128, 0.0), (1000, 0.0), (2333, 0.4)])
def test_mlp_backward_front_half_plus_rowgemm(ops, R, p):
    """mmfm_mlp_bwd with dx == NULL stops after t1 / g / du (eight-wave kernel); mmfm_rowgemm(ln_bwd) on du finishes dx.  t1, g, du must
    be the fused kernel's bit for bit (same operands, same MFMA order, same dropout decisions) and dx must match it to bf16 rounding."""
    x, Wu, bu, Wd, bd, g, bt, up, dn = mlp_setup(ops, R, seed=60)
    drop = None
    if p > 0:
        state = torch.zeros(2, dtype=torch.int32, device="cuda")
        ops.rng_seed(state, 11)
        drop = ops.dropout(state, 3, p)
    y, xhat, rstd = torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    ops.mlp_fwd(ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y, xhat=xhat, rstd=rstd, drop=drop))
    dy = rnd(R, 256, seed=78).to(BF)
    mk = lambda n: torch.full((R + 1, n), 5.0, device="cuda", dtype=BF)
    t1, gg, du, dx = mk(256), mk(512), mk(512), mk(256)
    ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], drop=drop, xhat=xhat, rstd=rstd, dy=dy, w_down_t=dn["WpT"], w_up_t=up["WpTP"],
                             t1=t1, g=gg, du=du, dx=dx))
    t1h, ggh, duh, dxh = mk(256), mk(512), mk(512), mk(256)
    ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], drop=drop, xhat=xhat, dy=dy, w_down_t=dn["WpT"], t1=t1h, g=ggh, du=duh, dx=None))
    ops.rowgemm(duh, up["WpT"], dxh, R, 256, 512, ldw=512, residual=dy, ldr=256, ln_bwd=True, bwd_xhat=xhat, bwd_rstd=rstd)
    assert torch.equal(t1h, t1) and torch.equal(ggh, gg) and torch.equal(duh, du)
    for b in (t1h, ggh, duh, dxh):
        assert torch.all(b[R:] == 5.0)
    check(dxh[:R], dx[:R].double(), 1.2e-2, "dx (front half + rowgemm) vs fused")
    if p == 0:
        xd = x.double().requires_grad_(True)
        h = F.layer_norm(xd, (256,), g.double(), bt.double(), 1e-5)
        out = xd + F.gelu(h @ Wu.double().T + bu.double()) @ Wd.double().T + bd.double()
        out.backward(dy.double())
        check(dxh[:R], xd.grad, 1.2e-2, "dx (front half + rowgemm) vs autograd")


@pytest.mark.parametrize("R", [70_000, 84_736 - 5, 204_800, 131_072 - 17])
def test_mlp_large_ragged_sizes_every_row(ops, R):
    """Launches of more than one round of passes with a ragged last round (workgroups with one pass more than others, a last pass
    with idle waves, a partial last tile).  Every row must come out exactly as a launch over just its neighbourhood produces it (rows
    are independent; rotate = 0 so that the order in which a workgroup walks the intermediate tiles - and with it the fp32 summation
    order - does not depend on which workgroup owns a row), nothing may be written past R, and no row may be skipped."""
    x, Wu, bu, Wd, bd, g, bt, up, dn = mlp_setup(ops, R, seed=90)
    y, xhat, rstd = torch.full((R + 2, 256), 3.0, device="cuda", dtype=BF), torch.full((R, 256), 7.0, device="cuda", dtype=BF), torch.full((R,), -1.0, device="cuda")
    ops.mlp_fwd(ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y, xhat=xhat, rstd=rstd, rotate=0))
    assert torch.all(y[R:] == 3.0) and torch.all(rstd > 0)
    dy = rnd(R, 256, seed=91).to(BF)
    mk = lambda n: torch.full((R + 1, n), 5.0, device="cuda", dtype=BF)
    t1, gg, du = mk(256), mk(512), mk(512)
    ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], xhat=xhat, dy=dy, w_down_t=dn["WpT"], t1=t1, g=gg, du=du, dx=None, rotate=0))
    assert torch.equal(t1[:R], dy)
    for b in (t1, gg, du):
        assert torch.all(b[R:] == 5.0)
    for r0 in (0, 65_536 - 96, R - 1000):                                 # first round, the round boundary, the tail
        n = min(1000, R - r0)
        ys, xs, rs_ = torch.empty(n, 256, device="cuda", dtype=BF), torch.empty(n, 256, device="cuda", dtype=BF), torch.empty(n, device="cuda")
        ops.mlp_fwd(ops.mlp_desc(n, x=x[r0:r0 + n], w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=ys, xhat=xs, rstd=rs_, rotate=0))
        assert torch.equal(ys, y[r0:r0 + n]) and torch.equal(xs, xhat[r0:r0 + n]) and torch.equal(rs_, rstd[r0:r0 + n])
        g2, d2, t2 = torch.empty(n, 512, device="cuda", dtype=BF), torch.empty(n, 512, device="cuda", dtype=BF), torch.empty(n, 256, device="cuda", dtype=BF)
        ops.mlp_bwd(ops.mlp_desc(n, w_up=up["Wp"], b_up=up["bp"], xhat=xs, dy=dy[r0:r0 + n], w_down_t=dn["WpT"], t1=t2, g=g2, du=d2, dx=None, rotate=0))
        assert torch.equal(g2, gg[r0:r0 + n]) and torch.equal(d2, du[r0:r0 + n])
    # no row skipped anywhere: g = gelu(u) of a random row is never exactly the fill value in all 512 columns
    assert not torch.any(torch.all(gg[:R] == 5.0, dim=1)) and not torch.any(torch.all(xhat == 7.0, dim=1))


def test_ln_linear_grad_matches_autograd(ops):
    """dW, db of the linear and dgamma, dbeta of the LayerNorm in front of it from G = dY^T x_hat and db = colsum dY."""
    R, N, K = 700, 96, 256
    x = (rnd(R, K, seed=1) * 1.3 + 0.4).double().requires_grad_(False)
    W, bias, g, bt = (rnd(N, K, seed=2, scale=1 / 16).double().requires_grad_(True), rnd(N, seed=3).double().requires_grad_(True),
                      (1 + 0.3 * rnd(K, seed=4)).double().requires_grad_(True), (0.2 * rnd(K, seed=5)).double().requires_grad_(True))
    dY = rnd(R, N, seed=6).double()
    y = F.layer_norm(x, (K,), g, bt, 1e-5) @ W.T + bias
    y.backward(dY)
    xhat = F.layer_norm(x, (K,), None, None, 1e-5)
    Gdb = torch.cat([(dY.T @ xhat).flatten(), dY.sum(0)]).float().contiguous()
    dW, db, dg, dbt = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda"), torch.ones(K, device="cuda"), torch.ones(K, device="cuda")
    ws = ops.ln_linear_grad_workspace(K, "cuda")
    ops.ln_linear_grad(Gdb, W.detach().float().contiguous(), g.detach().float().contiguous(), bt.detach().float().contiguous(), N, K, dW, db, dg, dbt, ws)
    torch.testing.assert_close(dW.double(), W.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(db.double(), bias.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dg.double(), g.grad, rtol=1e-4, atol=2e-4)
    torch.testing.assert_close(dbt.double(), bt.grad, rtol=1e-4, atol=2e-4)
    ops.ln_linear_grad(Gdb, W.detach().float().contiguous(), g.detach().float().contiguous(), bt.detach().float().contiguous(), N, K, dW, db, dg, dbt,
                       ws, accumulate_ln=True)                                      # same workspace: the tickets re-armed themselves
    torch.testing.assert_close(dg.double(), 2 * g.grad, rtol=1e-4, atol=4e-4)


# ------------------------------------------------------------------------------------ BASELINE configs[1] row count
# R = 1024 x 200 (+ a ragged tail): every workgroup walks several 128-row passes (the weight ring runs across pass boundaries,
# chunk rotation, tail masking), which the small cases above never reach.  Checked on a sample of rows against torch fp64 and,
# row-local ops being position independent, bit for bit against a small launch over the first rows.
R_FULL = 1024 * 200 + 37


def sample_rows(R, n=1536, seed=0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.cat([torch.arange(0, 200), torch.randint(0, R, (n,), generator=g), torch.arange(R - 300, R)]).unique()
    return idx.cuda()


def test_full_size_rowgemm_variants(ops):
    R = R_FULL
    idx = sample_rows(R)
    x = (rnd(R, 256, seed=1) * 2 + rnd(R, 1, seed=5)).to(BF)
    res = rnd(R, 256, seed=4).to(BF)
    # out_proj-type: plain product + bias + residual
    W, b = rnd(256, 256, seed=2, scale=1 / 16).to(BF), rnd(256, seed=3)
    y = torch.full((R + 3, 256), 7.0, device="cuda", dtype=BF)
    ops.rowgemm(x, W, y, R, 256, 256, bias=b, residual=res, ldr=256)
    check(y[idx], x[idx].double() @ W.double().T + b.double() + res[idx].double(), 4e-3, "full-size rowgemm")
    assert torch.all(y[R:] == 7.0)
    y_small = torch.empty(1000, 256, device="cuda", dtype=BF)
    ops.rowgemm(x[:1000], W, y_small, 1000, 256, 256, bias=b, residual=res[:1000], ldr=256)
    assert torch.equal(y_small, y[:1000])
    # LayerNorm-fed qkv
    Wq, g, bt, bq = rnd(768, 256, seed=6, scale=1 / 16), 1 + 0.3 * rnd(256, seed=7), 0.2 * rnd(256, seed=8), rnd(768, seed=9)
    e = prep(ops, Wq, g, bt, bq)
    yq, xhat, rstd = torch.empty(R, 768, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    ops.rowgemm(x, e["Wp"], yq, R, 768, 256, bias=e["bp"], ln=True, xhat=xhat, rstd=rstd, stream_out=True)
    xd = x[idx].double()
    check(yq[idx], F.layer_norm(xd, (256,), g.double(), bt.double(), 1e-5) @ Wq.double().T + bq.double(), 6e-3, "full-size LN+qkv")
    check(xhat[idx], F.layer_norm(xd, (256,), None, None, 1e-5), 3e-3, "full-size x_hat")
    # its backward: dx = dres + LayerNorm'(dqkv . Wp)
    dy = rnd(R, 768, seed=10, scale=0.5).to(BF)
    dx = torch.empty(R, 256, device="cuda", dtype=BF)
    ops.rowgemm(dy, e["WpT"], dx, R, 256, 768, ldw=768, residual=res, ldr=256, ln_bwd=True, bwd_xhat=xhat, bwd_rstd=rstd)
    v, xh, rs = dy[idx].double() @ e["Wp"].double(), xhat[idx].double(), rstd[idx].double()[:, None]
    check(dx[idx], res[idx].double() + rs * (v - v.mean(1, keepdim=True) - xh * (v * xh).mean(1, keepdim=True)), 5e-3, "full-size dX + LN backward")


def test_full_size_mlp_forward_backward(ops):
    R = R_FULL
    idx = sample_rows(R, seed=1)
    x, Wu, bu, Wd, bd, g, bt, up, dn = mlp_setup(ops, R, seed=60)
    y, xhat, rstd = torch.full((R + 2, 256), 3.0, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    ops.mlp_fwd(ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y, xhat=xhat, rstd=rstd, rotate=1))
    assert torch.all(y[R:] == 3.0)
    xd = x[idx].double().requires_grad_(True)
    h = F.layer_norm(xd, (256,), g.double(), bt.double(), 1e-5)
    u = h @ Wu.double().T + bu.double()
    gl = F.gelu(u)
    out = xd + gl @ Wd.double().T + bd.double()
    check(y[idx], out.detach(), 6e-3, "full-size mlp fwd")
    ys = torch.empty(1000, 256, device="cuda", dtype=BF)
    ops.mlp_fwd(ops.mlp_desc(1000, x=x[:1000], w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=ys, xhat=torch.empty(1000, 256, device="cuda", dtype=BF),
                             rstd=torch.empty(1000, device="cuda")))
    assert torch.equal(ys, y[:1000])
    dy = rnd(R, 256, seed=77).to(BF)
    t1, gg, du, dx = (torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, 512, device="cuda", dtype=BF),
                      torch.empty(R, 512, device="cuda", dtype=BF), torch.full((R + 1, 256), 5.0, device="cuda", dtype=BF))
    ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], xhat=xhat, rstd=rstd, dy=dy, w_down_t=dn["WpT"], w_up_t=up["WpTP"], t1=t1, g=gg, du=du, dx=dx, rotate=1))
    assert torch.equal(t1, dy) and torch.all(dx[R:] == 5.0)
    u.retain_grad(); gl.retain_grad()
    out.backward(dy[idx].double())
    check(gg[idx], gl.detach(), 6e-3, "full-size g")
    check(du[idx], u.grad, 1.2e-2, "full-size du")
    check(dx[idx], xd.grad, 1.2e-2, "full-size dx")


# ------------------------------------------------------------------------------------ the fused MLP with dropout on
def mlp_setup_norm(ops, R, scalenorm, seed):
    """mlp_setup, or its ScaleNorm twin: the up projection prepared with the scalar gain g = sqrt(256) (mmfm_prep_entry.scalar_gain)."""
    if not scalenorm:
        return mlp_setup(ops, R, seed=seed)
    x = (rnd(R, 256, seed=seed + 1) * 1.5 + rnd(R, 1, seed=seed + 2)).to(BF)
    Wu, bu = rnd(512, 256, seed=seed + 3, scale=1 / 16), 0.1 * rnd(512, seed=seed + 4)
    Wd, bd = rnd(256, 512, seed=seed + 5, scale=1 / 22), 0.1 * rnd(256, seed=seed + 6)
    g = torch.tensor([16.0], device="cuda")
    up = dict(W=Wu, gamma=g, scalar_gain=True, bias=bu, Wp=torch.empty(512, 256, device="cuda", dtype=BF),
              WpT=torch.empty(256, 512, device="cuda", dtype=BF), bp=torch.empty(512, device="cuda"))
    table, n, tiles = ops.prep_table([up], "cuda")
    ops.prep_weights(table, n, tiles)
    torch.cuda.synchronize()
    return x, Wu, bu, Wd, bd, g, None, up, prep(ops, Wd, None, None, bd)


@pytest.mark.parametrize("R", [1000, 2333])                      # neither a multiple of the 128-row pass
@pytest.mark.parametrize("norm,act", [("layernorm", "gelu"), ("scalenorm", "silu")])
def test_mlp_dropout_forward_backward_vs_autograd(ops, R, norm, act):
    """p = 0.4: y, g, du, dx and t1 of the real forward / backward (random dy) against fp64 autograd of x + mask * down(act(up(norm(x)))),
    the mask (RowDrop, csrc/rowchain.h) read off t1 of a dy = 1 launch, at the bounds test_mlp_forward / test_mlp_backward use at p = 0
    (6e-3 / 1.2e-2: dropout adds one multiply).  Both dx routes: the one-launch backward (LayerNorm only: it refuses ScaleNorm) and the
    front half + mmfm_rowgemm(ln_bwd).  A wrong row or feature in either direction's hash, a missing or doubled 1 / (1 - p), or a
    forward / backward pair that draws different masks all move y or the gradients by O(1)."""
    import dropout_refs as DR
    sn, p = norm == "scalenorm", 0.4
    kind, beta = ops.mlp_act(act)
    x, Wu, bu, Wd, bd, g, bt, up, dn = mlp_setup_norm(ops, R, sn, seed=120)
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 31)
    drop = ops.dropout(state, 4, p)
    mult = DR.rowdrop_multiplier(ops, state, 4, p, R).double()
    rate = (mult != 0).double().mean().item()
    assert abs(rate - (1 - p)) < 5 * math.sqrt(p * (1 - p) / mult.numel()) + 1e-4, f"keep rate {rate}"
    mk = lambda n, dt=BF: torch.full((R + 1, n), 5.0, device="cuda", dtype=dt)
    y, xhat, rstd = mk(256), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
    ops.mlp_fwd(ops.mlp_desc(R, x=x, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"], y=y, xhat=xhat, rstd=rstd, drop=drop,
                             scalenorm=sn, act=kind, act_beta=beta))
    dy = rnd(R, 256, seed=79).to(BF)
    t1, gg, du, dx = mk(256), mk(512), mk(512), mk(256)
    ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], drop=drop, xhat=xhat, dy=dy, w_down_t=dn["WpT"], t1=t1, g=gg, du=du, dx=None,
                             scalenorm=sn, act=kind, act_beta=beta))
    ops.rowgemm(du, up["WpT"], dx, R, 256, 512, ldw=512, residual=dy, ldr=256, ln_bwd=2 if sn else True, bwd_xhat=xhat, bwd_rstd=rstd)
    for b in (y, t1, gg, du, dx):
        assert torch.all(b[R:] == 5.0)
    xd = x.double().requires_grad_(True)
    if sn:
        h = xd * g.double() / xd.norm(dim=-1, keepdim=True).clamp(min=1e-5)
    else:
        h = F.layer_norm(xd, (256,), g.double(), bt.double(), 1e-5)
    u = h @ Wu.double().T + bu.double()
    gl = F.silu(u) if act == "silu" else F.gelu(u)
    out = xd + mult * (gl @ Wd.double().T + bd.double())
    u.retain_grad()
    out.backward(dy.double())
    check(y[:R], out.detach(), 6e-3, f"{norm}/{act} y with dropout")
    check(t1[:R], dy.double() * mult, 6e-3, "t1 = dropout'(dy)")           # one bf16 rounding of dy / (1 - p)
    assert torch.equal(t1[:R] != 0, (mult != 0) & (dy != 0))
    check(gg[:R], gl.detach(), 6e-3, "g")
    check(du[:R], u.grad, 1.2e-2, "du")
    check(dx[:R], xd.grad, 1.2e-2, "dx (front half + rowgemm)")
    if not sn:
        t1f, ggf, duf, dxf = mk(256), mk(512), mk(512), mk(256)
        ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], drop=drop, xhat=xhat, rstd=rstd, dy=dy, w_down_t=dn["WpT"], w_up_t=up["WpTP"],
                                 t1=t1f, g=ggf, du=duf, dx=dxf, act=kind, act_beta=beta))
        assert torch.equal(t1f, t1) and torch.equal(ggf, gg) and torch.equal(duf, du) and torch.all(dxf[R:] == 5.0)
        check(dxf[:R], xd.grad, 1.2e-2, "dx (one-launch backward)")


def test_rowdrop_hash_statistics(ops):
    """The fused MLP's row-keyed hash (RowDrop, csrc/rowchain.h: a key per row, a short mix per feature pair) under the statistics and
    bounds test_dropout_pair_hash_statistics applies to the flat hash, on 16,384 rows of 256 (4 M decisions, noise 5e-4): keep rate within
    4 sigma, |corr| < 0.01 between the halves of a pair, along columns, along rows - the lags 127, 128, 129 straddle the 128-row pass
    of a workgroup -, against another site and against the next step; same state and site give the same mask."""
    import dropout_refs as DR
    R, N, p = 16384, 256, 0.4
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 1234)
    mask = lambda site: (DR.rowdrop_multiplier(ops, state, site, p, R) != 0).float()
    k = mask(3)
    assert abs(k.mean().item() - (1 - p)) < 4 * math.sqrt(p * (1 - p) / (R * N))
    c = k - (1 - p)
    var = p * (1 - p)
    corr = lambda a, b: (a * b).mean().item() / var
    assert abs(corr(c[:, 0::2], c[:, 1::2])) < 0.01                      # the two halves of one hash
    for lag in (1, 2, 3, 4, 8, 16, 32, 64):
        assert abs(corr(c[:, :-lag], c[:, lag:])) < 0.01, f"column lag {lag}"
    for lag in (1, 2, 8, 127, 128, 129):
        assert abs(corr(c[:-lag], c[lag:])) < 0.01, f"row lag {lag}"
    assert abs(corr(c, mask(4) - (1 - p))) < 0.01                        # another site
    assert torch.equal(k, mask(3))                                       # same state, same site: same mask
    ops.rng_advance(state)
    assert abs(corr(c, mask(3) - (1 - p))) < 0.01                        # next step
