"""tests/rowowner_refs.py proved before it is used.  No GPU:
  * every reference agrees with torch fp64 autograd of the plain formulation;
  * every exact-integer generator meets its <= 256 condition at every shape tests/test_rowowner_elementwise_gpu.py uses;
  * a plain emulation of the kernels (bf16 inputs cast up, fp32 matmul, bf16 rounding where the kernel rounds) passes every check;
  * the same emulation with a fault injected is rejected: the exact cases reject (a) one product dropped from one element, (b) one
    output element replaced by its neighbour in the next row, (c) one 8-element store left at the fill value, (d) the bias missing on one
    column, (e) the residual missing on one row, (f) one row of x_hat stale; the derived-bound cases reject (b) to (f);
  * the relative-L2 check() of tests/test_rowchain_gpu.py, at its thresholds, accepts (b) and (c) at 1000 x 768: the gap this closes."""
import pytest
import torch
import torch.nn.functional as F

import rowowner_refs as RR
from test_rowchain_gpu import check as l2_check

D, BF = torch.float64, torch.bfloat16
FILL = 1e30                      # the sentinel of the GPU tests' output buffers


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype) * scale


def same(a, b, what, rtol=1e-11, atol=1e-12):
    assert a.dtype == D, f"{what}: the reference must return fp64, got {a.dtype}"
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {(a - b).abs().max().item():.3e}"


def rejected(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ------------------------------------------------------------------------------------------------- references against autograd
def plain_norm(x, norm, eps=1e-5):
    if norm == 1:
        return F.layer_norm(x, (x.shape[1],), None, None, eps)
    return x / x.norm(dim=1, keepdim=True).clamp(min=eps)


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("groups", [1, 3])
def test_norm_linear_refs_match_autograd(norm, groups):
    """norm_fwd + product = norm + linear; norm_bwd = its autograd with respect to x (the grouped dX sum for several linears)."""
    R, N = 37, 64
    x = rnd(R, 256, seed=1, dtype=D) * 1.5 + 0.3
    if norm == 2:
        x[5] = 0.0                                                      # a clamped row
    x.requires_grad_(True)
    Ws = [rnd(N, 256, seed=10 + g, scale=1 / 16, dtype=D) for g in range(groups)]
    bs = [rnd(N, seed=20 + g, dtype=D) for g in range(groups)]
    dys = [rnd(R, N, seed=30 + g, dtype=D) for g in range(groups)]
    dres = rnd(R, 256, seed=40, dtype=D)
    xh_plain = plain_norm(x, norm)
    ys = [xh_plain @ W.T + b for W, b in zip(Ws, bs)]
    (sum((y * dy).sum() for y, dy in zip(ys, dys)) + (x * dres).sum()).backward()
    xh, rstd, e32 = RR.norm_fwd(x.detach(), norm)
    same(xh, xh_plain.detach(), "x_hat")
    assert (e32 >= 0).all() and (rstd[5] < 0 if norm == 2 else (rstd > 0).all())
    for g in range(groups):
        ref, e = RR.product(xh, Ws[g], bs[g])
        same(ref, ys[g].detach(), f"y[{g}]")
        assert (e > 0).all()
    ref, e = RR.norm_bwd(dys, [W.T for W in Ws], xh, rstd, dres, norm)
    same(ref, x.grad, "dx", atol=1e-9 if norm == 2 else 1e-12)          # the clamped row's 1 / eps scales its rounding
    assert (e >= 0).all()
    same(RR.norm_bwd(dys, [W.T for W in Ws], xh, rstd, None, norm)[0], x.grad - dres, "dx without residual", atol=1e-9 if norm == 2 else 1e-12)


@pytest.mark.parametrize("kind,beta,act", [(RR.ACT_GELU, 1.0, F.gelu), (RR.ACT_RELU, 1.0, F.relu), (RR.ACT_SIGMOID, 1.0, F.silu),
                                           (RR.ACT_SIGMOID, 1.702, lambda u: u * torch.sigmoid(1.702 * u))])
def test_mlp_refs_match_autograd(kind, beta, act):
    R = 29
    x = (rnd(R, 256, seed=1, dtype=D) * 1.5 + 0.2).requires_grad_(True)
    Wu, bu = rnd(512, 256, seed=2, scale=1 / 16, dtype=D), rnd(512, seed=3, scale=0.1, dtype=D)
    Wd, bd = rnd(256, 512, seed=4, scale=1 / 22, dtype=D), rnd(256, seed=5, scale=0.1, dtype=D)
    dy = rnd(R, 256, seed=6, dtype=D)
    xh_plain = plain_norm(x, 1)
    u = xh_plain @ Wu.T + bu
    g = act(u)
    y = x + g @ Wd.T + bd
    u.retain_grad(), g.retain_grad()
    y.backward(dy)
    xh, rstd, _ = RR.norm_fwd(x.detach(), 1)
    ref, e = RR.mlp_fwd_ref(x.detach(), xh, Wu, bu, Wd, bd, kind, beta)
    same(ref, y.detach(), "y")
    assert (e > 0).all()
    same(RR.mlp_fwd_ref(x.detach(), xh, Wu, bu, Wd, None, kind, beta)[0], (y - bd).detach(), "y without b_down")
    r = RR.mlp_bwd_refs(xh, Wu, bu, dy, Wd.T, kind, beta)
    same(r["g"], g.detach(), "g")
    same(r["du"], u.grad, "du")
    same(RR.norm_bwd([r["du"]], [Wu.T], xh, rstd, dy, 1)[0], x.grad, "dx")
    # the derivatives the bounds propagate errors with
    uu = torch.linspace(-6, 6, 241, dtype=D).requires_grad_(True)
    d1, = torch.autograd.grad(act(uu).sum(), uu, create_graph=True)
    same(RR.act_d1(kind, uu.detach(), beta), d1.detach(), "act'")
    if kind != RR.ACT_RELU:
        d2, = torch.autograd.grad(d1.sum(), uu)
        same(RR.act_d2(kind, uu.detach(), beta), d2, "act''")


# ------------------------------------------------------------------------------------------------- the exact cases hold their condition
ROWS = RR.ROWS                   # the row counts tests/test_rowowner_elementwise_gpu.py uses


def test_exact_generators_hold_their_condition_small():
    """Every generator asserts its own condition (|value| <= 256, integer valued) while it builds the case; run each at every shape
    below the multi-pass row count and hold the result well inside it (the constructions put 256 at 8 sigma or more)."""
    for R in ROWS[:3]:
        for K in (256, 512, 768):
            for N in (64, 256, 768):
                assert float(RR.exact_rowgemm(R, N, K, "cpu")["ref"].abs().max()) <= 200
        for norm in (1, 2):
            for N, G in ((64, 1), (256, 1), (768, 1), (256, 2), (512, 5)):
                c = RR.exact_norm_rowgemm(R, N, norm, "cpu", residual=G == 1, groups=G)
                assert max(float(r.abs().max()) for r in c["refs"]) <= 160
        c = RR.exact_mlp(R, "cpu")
        assert max(float(c[k].abs().max()) for k in ("y", "g", "du")) <= 200


@pytest.mark.parametrize("R", ROWS[3:])
def test_exact_generators_hold_their_condition_large(R):
    """The two large row counts, once each on the CPU, at the widest shape of each kernel (the larger K and N are, the nearer the sums
    come to 256)."""
    for K in (256, 768):
        assert float(RR.exact_rowgemm(R, 768, K, "cpu")["ref"].abs().max()) <= 200
    for norm in (1, 2):
        assert float(RR.exact_norm_rowgemm(R, 768, norm, "cpu", residual=True)["refs"][0].abs().max()) <= 160
    c = RR.exact_mlp(R, "cpu")
    assert max(float(c[k].abs().max()) for k in ("y", "g", "du")) <= 200


def test_exact_layernorm_rows_round_to_unit_xhat():
    """balanced_rows: mean 0 and variance 1 exactly, so fp32 LayerNorm gives +-0.999995 in any order and bf16 rounds it to +-1."""
    x = RR.balanced_rows(200, torch.Generator().manual_seed(0))
    assert (x.sum(1) == 0).all() and (x.abs() == 1).all()
    xh, rs = emu_norm(x.to(BF), 1)
    assert torch.equal(xh, x.to(BF))
    RR.check_norm(xh, rs, x.to(BF), 1, "balanced rows")
    xs = torch.where(torch.rand(50, 256, generator=torch.Generator().manual_seed(1)) < 0.5, 1.0, -1.0).to(BF)
    xh, rs = emu_norm(xs, 2)
    assert torch.equal(xh, (xs.double() / 16).to(BF)) and torch.equal(rs, torch.full((50,), 1 / 16))


# ------------------------------------------------------------------------------------------------- the emulation
def emu_rowgemm(x, W, bias=None, res=None, skip=None):
    """fp32 product of the bf16 operands + bias + residual, one bf16 rounding.  skip = (row, col, k): that product is left out."""
    acc = x.float() @ W.float().T
    if skip is not None:
        r, c, k = skip
        acc[r, c] -= x[r, k].float() * W[c, k].float()
    if bias is not None:
        acc = acc + bias.float()
    if res is not None:
        acc = acc + res.float()
    return acc.to(BF)


def emu_norm(x, norm, eps=1e-5):
    xf = x.float()
    if norm == 1:
        mu = xf.mean(1, keepdim=True)
        rs = torch.rsqrt(((xf - mu) ** 2).mean(1, keepdim=True) + eps)
        return ((xf - mu) * rs).to(BF), rs[:, 0]
    n = xf.norm(dim=1, keepdim=True)
    rs = 1.0 / n.clamp_min(eps)
    return (xf * rs).to(BF), torch.where(n > eps, rs, -rs)[:, 0]


def emu_norm_bwd(xs, ws, xhat, rstd, res, norm):
    v = sum(x.float() @ w.float().T for x, w in zip(xs, ws))
    xh, rs = xhat.float(), rstd.float()[:, None]
    if norm == 1:
        t = v - v.mean(1, keepdim=True) - xh * (v * xh).mean(1, keepdim=True)
    else:
        t = v - xh * (v * xh).sum(1, keepdim=True) * (rs > 0)
    out = rs.abs() * t
    return (out + res.float() if res is not None else out).to(BF)


ACTS32 = {RR.ACT_GELU: F.gelu, RR.ACT_RELU: F.relu, RR.ACT_SIGMOID: F.silu}


def emu_mlp_fwd(x, Wu, bu, Wd, bd, kind, norm=1):
    xh, rs = emu_norm(x, norm)
    g = ACTS32[kind](xh.float() @ Wu.float().T + bu).to(BF)
    return emu_rowgemm(g, Wd, bd, x), xh, rs


def emu_mlp_bwd(xh, rs, Wu, bu, Wd, dy, kind, norm=1):
    u = (xh.float() @ Wu.float().T + bu).requires_grad_(True)
    a = ACTS32[kind](u)
    d1, = torch.autograd.grad(a.sum(), u)
    du = ((dy.float() @ Wd.float()) * d1).to(BF)
    return a.detach().to(BF), du, emu_norm_bwd([du], [Wu.T], xh, rs, dy, norm)


def bounds_rowgemm_case(R=1000, N=768, K=256):
    """test_rowgemm_plain's inputs at 1000 x 768 x 256."""
    x, W, b = rnd(R, K, seed=1).to(BF), rnd(N, K, seed=2, scale=K ** -0.5).to(BF), rnd(N, seed=3)
    return x, W, b, rnd(R, N, seed=4).to(BF)


def differing(y, r0, c0):
    """The first position at or after (r0, c0) in row r0 at which the next row holds another value."""
    c = c0 + int(torch.nonzero(y[r0, c0:] != y[r0 + 1, c0:])[0])
    return r0, c


# ------------------------------------------------------------------------------------------------- rowgemm: honest passes, faults fail
@pytest.mark.parametrize("K", [256, 768])
def test_rowgemm_exact_case_rejects_every_fault(K):
    R, N = 1000, 768
    c = RR.exact_rowgemm(R, N, K, "cpu")
    y = emu_rowgemm(c["x"], c["W"], c["bias"], c["res"])
    RR.check_exact(y, c["ref"], "honest")
    RR.assert_written(y, FILL, "honest")
    rejected(RR.check_exact, emu_rowgemm(c["x"], c["W"], c["bias"], c["res"], skip=(517, 300, K - 3)), c["ref"], "(a)")
    r, col = differing(y, 640, 100)
    f = y.clone(); f[r, col] = y[r + 1, col]
    rejected(RR.check_exact, f, c["ref"], "(b)")
    f = y.clone(); f[911, 256:264] = FILL
    rejected(RR.check_exact, f, c["ref"], "(c)")
    rejected(RR.assert_written, f, FILL, "(c)")
    col = int(torch.nonzero(c["bias"])[0])
    f = y.clone(); f[:, col] = emu_rowgemm(c["x"], c["W"], None, c["res"])[:, col]
    rejected(RR.check_exact, f, c["ref"], "(d)")
    r = 77
    assert c["res"][r].abs().max() > 0
    f = y.clone(); f[r] = emu_rowgemm(c["x"], c["W"], c["bias"], None)[r]
    rejected(RR.check_exact, f, c["ref"], "(e)")


def test_rowgemm_bounds_case_rejects_faults_the_l2_measure_accepts():
    x, W, b, res = bounds_rowgemm_case()
    R, N = res.shape
    y = emu_rowgemm(x, W, b, res)
    ratio = RR.check_product(y, x, W, b, res, "honest")
    assert 0.3 < ratio <= 1.0                                          # bf16 rounding uses at most the half ulp: the bound is tight, not slack
    ref = x.double() @ W.double().T + b.double() + res.double()
    l2_check(y, ref, 4e-3, "honest")
    # (b) one element replaced by its neighbour in the next row
    f = y.clone(); f[640, 100] = y[641, 100]
    assert (f[640, 100].double() - ref[640, 100]).abs() > 0.1
    rejected(RR.check_product, f, x, W, b, res, "(b)")
    l2_check(f, ref, 4e-3, "(b) under the old measure")             # accepted: the gap
    # (c) one 8-element store dropped: the buffer keeps what it held (the GPU tests fill with a sentinel, which assert_written also
    # catches; the old tests launch into torch.empty or a buffer a previous launch wrote - zeros here).  Whether the old measure accepts
    # it depends on the eight values lost (honest rounding alone is 1.65e-3 of the 4e-3): it accepts most stores, the new check none
    stores = [(r, c) for r in range(0, R, 143) for c in range(0, N, 200)]
    accepted = 0
    for r, c in stores:
        f = y.clone(); f[r, c:c + 8] = 0.0
        rejected(RR.check_product, f, x, W, b, res, "(c)")
        try:
            l2_check(f, ref, 4e-3, "(c) under the old measure")
            accepted += 1
        except AssertionError:
            pass
    assert accepted >= 2 * len(stores) // 3, f"the old measure accepted {accepted} of {len(stores)} dropped stores"
    f = y.clone(); f[500, 96:104] = 0.0
    l2_check(f, ref, 4e-3, "(c) under the old measure")             # accepted: the gap
    f[911, 256:264] = FILL
    rejected(RR.check_product, f, x, W, b, res, "(c) sentinel")
    rejected(RR.assert_written, f, FILL, "(c) sentinel")
    # (d) bias missing on one column, (e) residual missing on one row
    col = int(b.abs().argmax())
    f = y.clone(); f[:, col] = emu_rowgemm(x, W, None, res)[:, col]
    rejected(RR.check_product, f, x, W, b, res, "(d)")
    f = y.clone(); f[77] = emu_rowgemm(x, W, b, None)[77]
    rejected(RR.check_product, f, x, W, b, res, "(e)")


# ------------------------------------------------------------------------------------------------- norm prologue and backward epilogue
@pytest.mark.parametrize("norm", [1, 2])
def test_norm_rowgemm_exact_case_rejects_every_fault(norm):
    R, N = 1000, 768
    c = RR.exact_norm_rowgemm(R, N, norm, "cpu", residual=True)
    Wp, bp = c["Wp"][0], c["biases"][0]
    xh, rs = emu_norm(c["x"], norm)
    y = emu_rowgemm(xh, Wp, bp, c["res"])
    RR.check_exact(y, c["refs"][0], "honest y")
    RR.check_exact(xh, c["xhat"], "honest x_hat")
    RR.check_close(rs, c["rstd"], RR.TOL_LN_RSTD, "honest rstd")
    rejected(RR.check_exact, emu_rowgemm(xh, Wp, bp, c["res"], skip=(3, 700, 11)), c["refs"][0], "(a)")
    r, col = differing(y, 128, 64)
    f = y.clone(); f[r, col] = y[r + 1, col]
    rejected(RR.check_exact, f, c["refs"][0], "(b)")
    f = y.clone(); f[999, 760:768] = FILL
    rejected(RR.check_exact, f, c["refs"][0], "(c)")
    col = int(torch.nonzero(bp)[0])
    f = y.clone(); f[:, col] = emu_rowgemm(xh, Wp, None, c["res"])[:, col]
    rejected(RR.check_exact, f, c["refs"][0], "(d)")
    f = y.clone(); f[500] = emu_rowgemm(xh, Wp, bp, None)[500]
    rejected(RR.check_exact, f, c["refs"][0], "(e)")
    f = xh.clone(); f[130] = xh[129]                                   # (f) a stale row of x_hat
    rejected(RR.check_exact, f, c["xhat"], "(f)")


@pytest.mark.parametrize("norm", [1, 2])
def test_norm_rowgemm_bounds_case_rejects_faults(norm):
    R, N = 1000, 768
    x = (rnd(R, 256, seed=1) * 2 + rnd(R, 1, seed=5) * 3).to(BF)
    if norm == 2:
        x[17] = 0.0
    Wp, bp, res = rnd(N, 256, seed=2, scale=1 / 16).to(BF), rnd(N, seed=6), rnd(R, N, seed=7).to(BF)
    xh, rs = emu_norm(x, norm)
    y = emu_rowgemm(xh, Wp, bp, res)
    RR.check_norm(xh, rs, x, norm, "honest")
    RR.check_product(y, xh, Wp, bp, res, "honest y")
    f = y.clone(); f[640, 100] = y[641, 100]
    rejected(RR.check_product, f, xh, Wp, bp, res, "(b)")
    f = y.clone(); f[911, 256:264] = FILL
    rejected(RR.check_product, f, xh, Wp, bp, res, "(c)")
    col = int(bp.abs().argmax())
    f = y.clone(); f[:, col] = emu_rowgemm(xh, Wp, None, res)[:, col]
    rejected(RR.check_product, f, xh, Wp, bp, res, "(d)")
    f = y.clone(); f[77] = emu_rowgemm(xh, Wp, bp, None)[77]
    rejected(RR.check_product, f, xh, Wp, bp, res, "(e)")
    f = xh.clone(); f[130] = xh[129]                                   # (f): against x, and y (computed from the right row) against it
    rejected(RR.check_norm, f, rs, x, norm, "(f)")
    rejected(RR.check_product, y, f, Wp, bp, res, "(f) y")
    f = rs.clone(); f[130] = rs[129] * 1.001                           # a wrong rstd, and for ScaleNorm a lost clamp sign
    rejected(RR.check_norm, xh, f, x, norm, "rstd")
    if norm == 2:
        f = rs.clone(); f[17] = -rs[17]
        rejected(RR.check_norm, xh, f, x, norm, "clamp sign")


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("K,groups", [(256, 1), (768, 1), (512, 5)])
def test_norm_bwd_bounds_case_rejects_faults(norm, K, groups):
    R = 300
    dys = [rnd(R, K, seed=1 + g).to(BF) for g in range(groups)]
    WpTs = [rnd(256, K, seed=20 + g, scale=K ** -0.5).to(BF) for g in range(groups)]
    x = (rnd(R, 256, seed=4) * 1.7 + 0.5).to(BF)
    if norm == 2:
        x[9] = 0.0
    xh, rs = emu_norm(x, norm)
    res = rnd(R, 256, seed=5).to(BF)
    for r_ in (res, None):
        dx = emu_norm_bwd(dys, WpTs, xh, rs, r_, norm)
        RR.check_norm_bwd(dx, dys, WpTs, xh, rs, r_, norm, "honest")
    dx = emu_norm_bwd(dys, WpTs, xh, rs, res, norm)
    f = dx.clone(); f[100, 30] = dx[101, 30]
    rejected(RR.check_norm_bwd, f, dys, WpTs, xh, rs, res, norm, "(b)")
    f = dx.clone(); f[299, 248:256] = FILL
    rejected(RR.check_norm_bwd, f, dys, WpTs, xh, rs, res, norm, "(c)")
    f = dx.clone(); f[77] = emu_norm_bwd(dys, WpTs, xh, rs, None, norm)[77]
    rejected(RR.check_norm_bwd, f, dys, WpTs, xh, rs, res, norm, "(e)")
    f = xh.clone(); f[130] = xh[129]                                   # (f): the epilogue read a stale x_hat row
    rejected(RR.check_norm_bwd, emu_norm_bwd(dys, WpTs, f, rs, res, norm), dys, WpTs, xh, rs, res, norm, "(f)")
    if groups > 1:                                                     # a group left out of the sum
        rejected(RR.check_norm_bwd, emu_norm_bwd(dys[1:], WpTs[1:], xh, rs, res, norm), dys, WpTs, xh, rs, res, norm, "group dropped")
    if norm == 1:                                                      # the mean term forgotten
        v = sum(d.float() @ w.float().T for d, w in zip(dys, WpTs))
        f = (res.float() + rs[:, None] * (v - xh.float() * (v * xh.float()).mean(1, keepdim=True))).to(BF)
        rejected(RR.check_norm_bwd, f, dys, WpTs, xh, rs, res, norm, "mean dropped")


# ------------------------------------------------------------------------------------------------- the fused MLP
def test_mlp_exact_case_rejects_every_fault():
    R = 1000
    c = RR.exact_mlp(R, "cpu")
    Wu, Wd = c["Wu"].to(BF), c["Wd"].to(BF)
    y, xh, rs = emu_mlp_fwd(c["x"], Wu, c["bu"], Wd, c["bd"], RR.ACT_RELU)
    g, du, dx = emu_mlp_bwd(xh, rs, Wu, c["bu"], Wd, c["dy"], RR.ACT_RELU)
    for out, key in ((y, "y"), (xh, "xhat"), (g, "g"), (du, "du")):
        RR.check_exact(out, c[key], f"honest {key}")
    RR.check_close(rs, c["rstd"], RR.TOL_LN_RSTD, "honest rstd")
    RR.check_norm_bwd(dx, [du], [Wu.T], xh, rs, c["dy"], 1, "honest dx")
    # (a) one product dropped: in the up projection (seen through g and y) and in the down projection
    r, j = 400, int(torch.nonzero(c["g"][400])[0])
    k = int(torch.nonzero(Wu[j])[0])
    u_bad = xh.float() @ Wu.float().T + c["bu"]
    u_bad[r, j] -= xh[r, k].float() * Wu[j, k].float()
    g_bad = F.relu(u_bad).to(BF)
    rejected(RR.check_exact, g_bad, c["g"], "(a) g")
    n = int(torch.nonzero(Wd[:, j])[0])
    rejected(RR.check_exact, emu_rowgemm(g_bad, Wd, c["bd"], c["x"]), c["y"], "(a) y through g")
    rejected(RR.check_exact, emu_rowgemm(g, Wd, c["bd"], c["x"], skip=(r, n, j)), c["y"], "(a) y")
    for out, key in ((y, "y"), (g, "g"), (du, "du")):
        r, col = differing(out, 640, 100)
        f = out.clone(); f[r, col] = out[r + 1, col]
        rejected(RR.check_exact, f, c[key], f"(b) {key}")
        f = out.clone(); f[911, 248:256] = FILL
        rejected(RR.check_exact, f, c[key], f"(c) {key}")
    col = int(torch.nonzero(c["bd"])[0])
    f = y.clone(); f[:, col] = emu_rowgemm(g, Wd, None, c["x"])[:, col]
    rejected(RR.check_exact, f, c["y"], "(d) b_down")
    col = int(torch.nonzero(c["bu"])[0])
    u_bad = xh.float() @ Wu.float().T + c["bu"]
    u_bad[:, col] -= c["bu"][col]
    rejected(RR.check_exact, F.relu(u_bad).to(BF), c["g"], "(d) b_up")
    f = y.clone(); f[77] = emu_rowgemm(g, Wd, c["bd"], None)[77]
    rejected(RR.check_exact, f, c["y"], "(e)")
    f = xh.clone(); f[130] = xh[129]
    rejected(RR.check_exact, f, c["xhat"], "(f)")
    g2, du2, dx2 = emu_mlp_bwd(f, rs, Wu, c["bu"], Wd, c["dy"], RR.ACT_RELU)       # the backward recomputing u from a stale row
    rejected(RR.check_exact, g2, c["g"], "(f) g")
    rejected(RR.check_norm_bwd, dx2, [du], [Wu.T], xh, rs, c["dy"], 1, "(f) dx")
    f = dx.clone(); f[640, 100] = dx[641, 100]
    rejected(RR.check_norm_bwd, f, [du], [Wu.T], xh, rs, c["dy"], 1, "(b) dx")


@pytest.mark.parametrize("kind,norm", [(RR.ACT_GELU, 1), (RR.ACT_SIGMOID, 2)])
def test_mlp_bounds_case_rejects_faults(kind, norm):
    R = 1000
    x = (rnd(R, 256, seed=1) * 1.5 + rnd(R, 1, seed=2)).to(BF)
    Wu, bu = rnd(512, 256, seed=3, scale=(1 if norm == 1 else 16) / 16).to(BF), 0.1 * rnd(512, seed=4)
    Wd, bd = rnd(256, 512, seed=5, scale=1 / 22).to(BF), 0.1 * rnd(256, seed=6)
    dy = rnd(R, 256, seed=77).to(BF)
    y, xh, rs = emu_mlp_fwd(x, Wu, bu, Wd, bd, kind, norm)
    g, du, dx = emu_mlp_bwd(xh, rs, Wu, bu, Wd, dy, kind, norm)
    WdT = Wd.T.contiguous()

    def fwd(out, what, xh_=xh):
        ref, e32 = RR.mlp_fwd_ref(x, xh_, Wu, bu, Wd, bd, kind)
        return RR.check_bf16(out, ref, e32, what)

    def bwd(g_, du_, what, xh_=xh):
        return RR.check_mlp_bwd(g_, du_, xh_, Wu, bu, dy, WdT, kind, what)

    RR.check_norm(xh, rs, x, norm, "honest")
    assert fwd(y, "honest y") <= 1.0
    bwd(g, du, "honest")
    RR.check_norm_bwd(dx, [du], [Wu.T], xh, rs, dy, norm, "honest dx")
    f = y.clone(); f[640, 100] = y[641, 100]
    rejected(fwd, f, "(b) y")
    f = y.clone(); f[911, 248:256] = FILL
    rejected(fwd, f, "(c) y")
    col = int(bd.abs().argmax())
    f = y.clone(); f[:, col] = (y[:, col].float() - bd[col]).to(BF)
    rejected(fwd, f, "(d) y")
    f = y.clone(); f[77] = (y[77].float() - x[77].float()).to(BF)
    rejected(fwd, f, "(e) y")
    f = xh.clone(); f[130] = xh[129]
    rejected(RR.check_norm, f, rs, x, norm, "(f)")
    rejected(fwd, y, "(f) y", f)
    rejected(bwd, g, du, "(f) g / du", f)
    for out, name, args in ((g, "g", lambda t: (t, du)), (du, "du", lambda t: (g, t))):
        f = out.clone(); f[640, 100] = out[641, 100]
        rejected(bwd, *args(f), f"(b) {name}")
        f = out.clone(); f[911, 504:512] = FILL
        rejected(bwd, *args(f), f"(c) {name}")
    f = dx.clone(); f[640, 100] = dx[641, 100]
    rejected(RR.check_norm_bwd, f, [du], [Wu.T], xh, rs, dy, norm, "(b) dx")
    f = dx.clone(); f[77] = (dx[77].float() - dy[77].float()).to(BF)
    rejected(RR.check_norm_bwd, f, [du], [Wu.T], xh, rs, dy, norm, "(e) dx")


def test_sentinel_helpers():
    t = torch.full((4, 8), FILL, dtype=BF)
    RR.assert_untouched(t, FILL, "guard")
    RR.assert_untouched(torch.full((3,), float("nan")), float("nan"), "NaN pad")
    rejected(RR.assert_written, t, FILL, "unwritten")
    t[2, 3] = 1.0
    rejected(RR.assert_untouched, t, FILL, "guard hit")
    RR.assert_written(torch.zeros(3, dtype=BF), FILL, "written")
