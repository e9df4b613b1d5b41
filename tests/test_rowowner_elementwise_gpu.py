"""The row-owner kernels (mmfm_rowgemm, mmfm_rowgemm_groups, mmfm_mlp_fwd, mmfm_mlp_bwd) element by element, on every row, through
every launch shape their dispatchers can pick: the exact-integer cases of tests/rowowner_refs.py bit for bit, the randn cases against
fp64 references at derived bounds (tests/test_rowowner_refs_cpu.py proves both).  Row counts: rowowner_refs.ROWS, the smallest that
reach each launch shape; the workload's 204,837 rows stay with the full-size tests of test_rowchain_gpu.py.

Every output buffer carries guard rows and is filled with a sentinel no result can take: no element of the rows a launch owns may still
hold it afterwards, and the guard rows (and, in the strided cases, the pad columns) must still hold it.  The report lines give the worst
|err| / bound of every derived-bound check (pytest -s)."""
import pytest
import torch

import rowowner_refs as RR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FILL = 1e30                # the sentinel: finite in bf16 and fp32, beyond anything these inputs produce
GUARD = 3                  # rows beyond R in every output buffer
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda") * scale


def obuf(R, N=None, ld=None, dtype=BF):
    """An output buffer of R + GUARD rows (of ld >= N elements), every element the sentinel."""
    return torch.full((R + GUARD,) if N is None else (R + GUARD, ld or N), FILL, device="cuda", dtype=dtype)


def done(buf, R, N, what):
    """The rows < R of a buffer a launch has written: all written, guard rows and pad columns untouched.  Returns the [R, N] view."""
    out = buf[:R] if buf.dim() == 1 else buf[:R, :N]
    RR.assert_written(out, FILL, what)
    RR.assert_untouched(buf[R:], FILL, f"{what}: guard rows")
    if buf.dim() == 2 and buf.shape[1] > N:
        RR.assert_untouched(buf[:R, N:], FILL, f"{what}: pad columns")
    return out


def padded(t, ld):
    """t [R, K] inside a [R, ld] buffer whose pad columns hold NaN: a kernel that reads a pad poisons its row."""
    buf = torch.full((t.shape[0], ld), NAN, device="cuda", dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf


def prep(ops, entries):
    table, n, tiles = ops.prep_table(entries, "cuda")
    ops.prep_weights(table, n, tiles)
    torch.cuda.synchronize()


def prep_linear(ops, W, gamma=None, beta=None, bias=None, scalar_gain=False, want_bp=True):
    """mmfm_prep_weights for one linear: Wp, WpT, bp and the unit-permuted copies."""
    N, K = W.shape
    e = dict(W=W, gamma=gamma, beta=beta, bias=bias, scalar_gain=scalar_gain, Wp=torch.empty(N, K, device="cuda", dtype=BF),
             WpT=torch.empty(K, N, device="cuda", dtype=BF), bp=torch.empty(N, device="cuda") if want_bp else None,
             WpP=torch.empty(N, K, device="cuda", dtype=BF), WpTP=torch.empty(K, N, device="cuda", dtype=BF))
    prep(ops, [e])
    return e


def prep_groups(ops, Ws, gammas, betas, biases, scalar_gain=False):
    """The prepared weights of all groups as slices of one tensor each: the grouped launch addresses them through one buffer."""
    G, (N, K) = len(Ws), Ws[0].shape
    Wp, WpT, bp = torch.empty(G, N, K, device="cuda", dtype=BF), torch.empty(G, K, N, device="cuda", dtype=BF), torch.empty(G, N, device="cuda")
    prep(ops, [dict(W=Ws[g], gamma=gammas[g] if gammas is not None else None, beta=betas[g] if betas is not None else None,
                    bias=biases[g] if biases is not None else None, Wp=Wp[g], WpT=WpT[g], bp=bp[g], scalar_gain=scalar_gain) for g in range(G)])
    return Wp, WpT, bp


ROWS = RR.ROWS


# ------------------------------------------------------------------------------------------------- mmfm_rowgemm, plain
@pytest.mark.parametrize("K", [256, 512, 768])
@pytest.mark.parametrize("R", ROWS)
def test_rowgemm_plain(ops, R, K):
    """K = 256: the LDS-DMA ring (no residual, or N = 256 with one: four column pairs in one block or, below 128 passes, one in each of
    four), the register-staged ring (residual at N != 256); K = 512 / 768: the staged ring at one workgroup per CU.  Each with temporal
    and non-temporal stores; bias = NULL on one combination per N."""
    for N in (64, 256, 768):
        for residual in (True, False):
            for stream_out in (False, True):
                bias = residual or not stream_out
                what = f"rowgemm R={R} K={K} N={N} res={residual} nt={stream_out} bias={bias}"
                c = RR.exact_rowgemm(R, N, K, "cuda", seed=N + K, bias=bias, residual=residual)
                y = obuf(R, N)
                ops.rowgemm(c["x"], c["W"], y, R, N, K, bias=c["bias"], residual=c["res"], ldr=N if residual else 0, stream_out=stream_out)
                RR.check_exact(done(y, R, N, what), c["ref"], f"{what} exact")
                x, W = rnd(R, K, seed=1).to(BF), rnd(N, K, seed=2, scale=K ** -0.5).to(BF)
                b, res = rnd(N, seed=3) if bias else None, rnd(R, N, seed=4).to(BF) if residual else None
                y = obuf(R, N)
                ops.rowgemm(x, W, y, R, N, K, bias=b, residual=res, ldr=N if residual else 0, stream_out=stream_out)
                RR.check_product(done(y, R, N, what), x, W, b, res, what)


# ------------------------------------------------------------------------------------------------- mmfm_rowgemm, norm prologue
def norm_weights(ops, N, norm, bias, seed=0, groups=1):
    """randn master weights with a non-trivial norm affine, prepared: (Wp [G, N, 256], bp [G, N] or None)."""
    Ws = [rnd(N, 256, seed=seed + 10 + g, scale=1 / 16) for g in range(groups)]
    bs = [rnd(N, seed=seed + 30 + g) for g in range(groups)] if bias else None
    if norm == 1:
        gam, bet = [1 + 0.3 * rnd(256, seed=seed + 50 + g) for g in range(groups)], [0.2 * rnd(256, seed=seed + 70 + g) for g in range(groups)]
    else:
        gam, bet = [16 * (1 + 0.3 * rnd(1, seed=seed + 50 + g).abs()) for g in range(groups)], None
    Wp, WpT, bp = prep_groups(ops, Ws, gam, bet, bs, scalar_gain=norm == 2)
    return Wp, WpT, (bp if bias or norm == 1 else None)          # under a LayerNorm the prepared bias W . beta exists either way


def norm_input(R, norm, seed=1):
    x = (rnd(R, 256, seed=seed) * 2 + rnd(R, 1, seed=seed + 4) * 3).to(BF)       # non-zero row means
    if norm == 2:
        x[R // 2] = 0.0                                                           # a clamped row: rstd saved negated
    return x


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("R", ROWS)
def test_rowgemm_norm_prologue(ops, R, norm):
    """ln = 1 / 2 without a residual: the LDS-DMA ring, x_hat / rstd written by column block 0 when N is split; with one: the staged ring."""
    for N in (64, 256, 768):
        for residual, stream_out in ((False, False), (False, True), (True, False)):
            bias = norm == 1 or N != 256 or residual                     # ScaleNorm, N = 256, no residual: bias = NULL
            what = f"rowgemm ln={norm} R={R} N={N} res={residual} nt={stream_out} bias={bias}"
            c = RR.exact_norm_rowgemm(R, N, norm, "cuda", seed=N, bias=bias, residual=residual)
            e = prep_linear(ops, c["Ws"][0], gamma=c["gamma"], bias=c["biases"][0], scalar_gain=norm == 2, want_bp=bias)
            RR.check_exact(e["Wp"], c["Wp"][0], f"{what} prepared weights")
            if bias:
                RR.check_exact(e["bp"], c["biases"][0], f"{what} prepared bias")
            y, xhat, rstd = obuf(R, N), obuf(R, 256), obuf(R, dtype=torch.float32)
            ops.rowgemm(c["x"], e["Wp"], y, R, N, 256, bias=e["bp"], ln=norm, xhat=xhat, rstd=rstd, residual=c["res"], ldr=N if residual else 0,
                        stream_out=stream_out)
            RR.check_exact(done(y, R, N, what), c["refs"][0], f"{what} exact y")
            RR.check_exact(done(xhat, R, 256, what), c["xhat"], f"{what} exact x_hat")
            RR.check_close(done(rstd, R, 0, what), c["rstd"], RR.TOL_LN_RSTD, f"{what} exact-case rstd")
            x = norm_input(R, norm)
            Wp, _, bp = norm_weights(ops, N, norm, bias)
            res = rnd(R, N, seed=7).to(BF) if residual else None
            y, xhat, rstd = obuf(R, N), obuf(R, 256), obuf(R, dtype=torch.float32)
            ops.rowgemm(x, Wp[0], y, R, N, 256, bias=None if bp is None else bp[0], ln=norm, xhat=xhat, rstd=rstd, residual=res,
                        ldr=N if residual else 0, stream_out=stream_out)
            xh = done(xhat, R, 256, what)
            RR.check_norm(xh, done(rstd, R, 0, what), x, norm, what)
            RR.check_product(done(y, R, N, what), xh, Wp[0], None if bp is None else bp[0], res, f"{what} y")
            if norm == 2:
                assert rstd[R // 2] < 0 and torch.all(rstd[:R // 2] > 0), f"{what}: the clamped row's rstd must be saved negated, no other"


# ------------------------------------------------------------------------------------------------- mmfm_rowgemm, norm backward epilogue
def bwd_operands(R, K, norm, groups=1):
    dys = [rnd(R, K, seed=1 + g).to(BF) for g in range(groups)]
    x = norm_input(R, norm, seed=4)
    xh64, rs64, _ = RR.norm_fwd(x, norm)
    return dys, xh64.to(BF).contiguous(), rs64.float().contiguous(), rnd(R, 256, seed=5).to(BF)


@pytest.mark.parametrize("K", [256, 512, 768])
@pytest.mark.parametrize("R", ROWS)
def test_rowgemm_norm_backward(ops, R, K):
    """ln_bwd = 1 / 2: the wave-pair kernel (K = 256) and the two ring kernels (K = 512, 768), with and without residual; the ScaleNorm
    case carries a clamped row (rstd < 0: the projection term is dropped)."""
    for norm in (1, 2):
        dys, xhat, rstd, dres = bwd_operands(R, K, norm)
        gam = [1 + 0.3 * rnd(256, seed=3)] if norm == 1 else [16 * (1 + 0.3 * rnd(1, seed=3).abs())]
        _, WpT, _ = prep_groups(ops, [rnd(K, 256, seed=2, scale=K ** -0.5)], gam, None, None, scalar_gain=norm == 2)
        for res in (dres, None):
            what = f"rowgemm ln_bwd={norm} R={R} K={K} res={res is not None}"
            dx = obuf(R, 256)
            ops.rowgemm(dys[0], WpT[0], dx, R, 256, K, ldw=K, residual=res, ldr=256 if res is not None else 0, ln_bwd=norm, bwd_xhat=xhat, bwd_rstd=rstd)
            RR.check_norm_bwd(done(dx, R, 256, what), dys, [WpT[0]], xhat, rstd, res, norm, what)


# ------------------------------------------------------------------------------------------------- mmfm_rowgemm_groups
@pytest.mark.parametrize("G,N", [(2, 256), (5, 512)])
@pytest.mark.parametrize("R", ROWS)
def test_rowgemm_groups_forward(ops, R, G, N):
    for norm in (1, 2):
        what = f"groups fwd ln={norm} R={R} G={G} N={N}"
        c = RR.exact_norm_rowgemm(R, N, norm, "cuda", seed=G, groups=G)
        Wp, _, bp = prep_groups(ops, c["Ws"], None if norm == 1 else [c["gamma"]] * G, None, c["biases"], scalar_gain=norm == 2)
        ys, xhat, rstd = [obuf(R, N) for _ in range(G)], obuf(R, 256), obuf(R, dtype=torch.float32)
        ops.rowgemm_groups([c["x"]], [Wp[g] for g in range(G)], ys, R, N, 256, biases=[bp[g] for g in range(G)], ln=norm, xhat=xhat, rstd=rstd,
                           stream_out=True)
        for g in range(G):
            RR.check_exact(Wp[g], c["Wp"][g], f"{what} prepared weights {g}")
            RR.check_exact(done(ys[g], R, N, what), c["refs"][g], f"{what} exact y[{g}]")
        RR.check_exact(done(xhat, R, 256, what), c["xhat"], f"{what} exact x_hat")
        RR.check_close(done(rstd, R, 0, what), c["rstd"], RR.TOL_LN_RSTD, f"{what} exact-case rstd")
        x = norm_input(R, norm)
        Wp, _, bp = norm_weights(ops, N, norm, True, groups=G)
        ys, xhat, rstd = [obuf(R, N) for _ in range(G)], obuf(R, 256), obuf(R, dtype=torch.float32)
        ops.rowgemm_groups([x], [Wp[g] for g in range(G)], ys, R, N, 256, biases=[bp[g] for g in range(G)], ln=norm, xhat=xhat, rstd=rstd)
        xh = done(xhat, R, 256, what)
        RR.check_norm(xh, done(rstd, R, 0, what), x, norm, what)
        for g in range(G):
            RR.check_product(done(ys[g], R, N, what), xh, Wp[g], bp[g], None, f"{what} y[{g}]")


@pytest.mark.parametrize("G,K", [(2, 256), (5, 256), (2, 512), (5, 512)])
@pytest.mark.parametrize("R", ROWS)
def test_rowgemm_groups_backward(ops, R, G, K):
    for norm in (1, 2):
        dys, xhat, rstd, dres = bwd_operands(R, K, norm, groups=G)
        gam = [1 + 0.3 * rnd(256 if norm == 1 else 1, seed=40 + g).abs() for g in range(G)]
        _, WpT, _ = prep_groups(ops, [rnd(K, 256, seed=20 + g, scale=K ** -0.5) for g in range(G)], gam, None, None, scalar_gain=norm == 2)
        for res in (dres, None):
            what = f"groups bwd ln_bwd={norm} R={R} G={G} K={K} res={res is not None}"
            dx = obuf(R, 256)
            ops.rowgemm_groups(dys, [WpT[g] for g in range(G)], [dx], R, 256, K, ldw=K, residual=res, ldr=256 if res is not None else 0, ln_bwd=norm,
                               bwd_xhat=xhat, bwd_rstd=rstd)
            RR.check_norm_bwd(done(dx, R, 256, what), dys, [WpT[g] for g in range(G)], xhat, rstd, res, norm, what)


# ------------------------------------------------------------------------------------------------- the fused MLP
def mlp_weights(ops, scalenorm, seed=0):
    """randn MLP weights as tests/test_rowchain_gpu.py's mlp_setup / mlp_setup_norm, prepared."""
    Wu, bu = rnd(512, 256, seed=seed + 3, scale=1 / 16), 0.1 * rnd(512, seed=seed + 4)
    Wd, bd = rnd(256, 512, seed=seed + 5, scale=1 / 22), 0.1 * rnd(256, seed=seed + 6)
    if scalenorm:
        up = prep_linear(ops, Wu, gamma=torch.tensor([16.0], device="cuda"), bias=bu, scalar_gain=True)
    else:
        up = prep_linear(ops, Wu, gamma=1 + 0.3 * rnd(256, seed=seed + 7), beta=0.2 * rnd(256, seed=seed + 8), bias=bu)
    return up, prep_linear(ops, Wd, bias=bd)


def run_mlp(ops, R, x, up, dn, dy, kind, rotate, scalenorm=False, b_down=True, one_launch=True, ld=None):
    """Forward, front half + mmfm_rowgemm(ln_bwd) and (LayerNorm only) the one-launch backward.  ld = (ldx, ldy, lddy, lddx) runs the
    strided variant.  Returns the [R, .] views of y, xhat, rstd, (t1, g, du, dx) of the split route and of the one-launch route."""
    what = f"mlp R={R} act={kind} rotate={rotate} scalenorm={scalenorm} b_down={b_down} ld={ld}"
    ldx, ldy, lddy, lddx = ld or (256, 256, 256, 256)
    xs, dys = (padded(x, ldx), padded(dy, lddy)) if ld else (x, dy)
    norm = 2 if scalenorm else 1
    kw = dict(scalenorm=scalenorm, act=kind, rotate=rotate)
    y, xhat, rstd = obuf(R, 256, ldy), obuf(R, 256), obuf(R, dtype=torch.float32)
    ops.mlp_fwd(ops.mlp_desc(R, x=xs, ldx=ldx, w_up=up["Wp"], b_up=up["bp"], w_down=dn["WpP"], b_down=dn["bp"] if b_down else None, y=y, ldy=ldy,
                             xhat=xhat, rstd=rstd, **kw))
    xh, rs = done(xhat, R, 256, what), done(rstd, R, 0, what)
    routes = []
    for one in ((False, True) if one_launch else (False,)):
        t1, g, du, dx = obuf(R, 256), obuf(R, 512), obuf(R, 512), obuf(R, 256, lddx)
        if one:
            ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], xhat=xh, rstd=rs, dy=dys, lddy=lddy, w_down_t=dn["WpT"], w_up_t=up["WpTP"],
                                     t1=t1, g=g, du=du, dx=dx, lddx=lddx, **kw))
        else:
            ops.mlp_bwd(ops.mlp_desc(R, w_up=up["Wp"], b_up=up["bp"], xhat=xh, dy=dys, lddy=lddy, w_down_t=dn["WpT"], t1=t1, g=g, du=du, dx=None, **kw))
            ops.rowgemm(done(du, R, 512, what), up["WpT"], dx, R, 256, 512, ldw=512, ldy=lddx, residual=dys, ldr=lddy, ln_bwd=norm, bwd_xhat=xh,
                        bwd_rstd=rs, rotate=rotate)
        w = f"{what} {'one launch' if one else 'front half + rowgemm'}"
        routes.append((done(t1, R, 256, w), done(g, R, 512, w), done(du, R, 512, w), done(dx, R, 256, w)))
    return done(y, R, 256, what), xh, rs, routes


@pytest.mark.parametrize("rotate", [0, 1])
@pytest.mark.parametrize("R", ROWS)
def test_mlp_relu_exact(ops, R, rotate):
    """LayerNorm + ReLU on the exact-integer case: y, x_hat, t1, g and du bit for bit in both backward routes, dx (through the LayerNorm
    backward, not exact) at norm_bwd's bound from each route's own du; b_down = NULL on the second pass."""
    for b_down in (True, False):
        c = RR.exact_mlp(R, "cuda", seed=R, b_down=b_down)
        up, dn = prep_linear(ops, c["Wu"], bias=c["bu"]), prep_linear(ops, c["Wd"], bias=c["bd"])
        RR.check_exact(up["bp"], c["bu"], "prepared b_up")
        y, xh, rs, routes = run_mlp(ops, R, c["x"], up, dn, c["dy"], RR.ACT_RELU, rotate, b_down=b_down)
        what = f"mlp relu R={R} rotate={rotate} b_down={b_down}"
        RR.check_exact(y, c["y"], f"{what} y")
        RR.check_exact(xh, c["xhat"], f"{what} x_hat")
        RR.check_close(rs, c["rstd"], RR.TOL_LN_RSTD, f"{what} rstd")
        for (t1, g, du, dx), route in zip(routes, ("front half + rowgemm", "one launch")):
            RR.check_exact(t1, c["dy"], f"{what} {route} t1")
            RR.check_exact(g, c["g"], f"{what} {route} g")
            RR.check_exact(du, c["du"], f"{what} {route} du")
            RR.check_norm_bwd(dx, [du], [up["WpT"]], xh, rs, c["dy"], 1, f"{what} {route} dx")


@pytest.mark.parametrize("rotate", [0, 1])
@pytest.mark.parametrize("norm,kind", [(1, RR.ACT_GELU), (2, RR.ACT_SIGMOID)])
@pytest.mark.parametrize("R", ROWS)
def test_mlp_bounds(ops, R, norm, kind, rotate):
    """LayerNorm + GELU (both backward routes) and ScaleNorm + SiLU (front half + rowgemm: the one-launch backward has no ScaleNorm
    epilogue) on randn inputs, every stage from the bf16 tensors the kernels stored."""
    sn = norm == 2
    x = (rnd(R, 256, seed=1) * 1.5 + rnd(R, 1, seed=2)).to(BF)
    dy = rnd(R, 256, seed=77).to(BF)
    up, dn = mlp_weights(ops, sn)
    y, xh, rs, routes = run_mlp(ops, R, x, up, dn, dy, kind, rotate, scalenorm=sn, one_launch=not sn)
    what = f"mlp {'scalenorm' if sn else 'layernorm'} act={kind} R={R} rotate={rotate}"
    RR.check_norm(xh, rs, x, norm, what)
    ref, e32 = RR.mlp_fwd_ref(x, xh, up["Wp"], up["bp"], dn["Wp"], dn["bp"], kind)
    RR.check_bf16(y, ref, e32, f"{what} y")
    for (t1, g, du, dx), route in zip(routes, ("front half + rowgemm", "one launch")):
        RR.check_exact(t1, dy, f"{what} {route} t1")
        RR.check_mlp_bwd(g, du, xh, up["Wp"], up["bp"], dy, dn["WpT"], kind, f"{what} {route}")
        RR.check_norm_bwd(dx, [du], [up["WpT"]], xh, rs, dy, norm, f"{what} {route} dx")
    if not sn:
        assert all(torch.equal(a, b) for a, b in zip(routes[0][:3], routes[1][:3])), f"{what}: t1 / g / du differ between the two backward routes"


# ------------------------------------------------------------------------------------------------- strided views
R_LD = 1000


def test_rowgemm_strided(ops):
    """ldx = K + 8, ldy = N + 8, ldr = N + 16: the results of the packed launch, pads (NaN on inputs, the sentinel on outputs) and guard
    rows untouched.  Plain (ring and staged ring), norm prologue, norm backward (lddx = 264)."""
    R = R_LD
    for K, N in ((256, 256), (256, 768), (512, 256)):
        c = RR.exact_rowgemm(R, N, K, "cuda", seed=5)
        y = obuf(R, N, N + 8)
        ops.rowgemm(padded(c["x"], K + 8), c["W"], y, R, N, K, ldx=K + 8, ldy=N + 8, bias=c["bias"], residual=padded(c["res"], N + 16), ldr=N + 16)
        RR.check_exact(done(y, R, N, f"strided rowgemm K={K} N={N}").contiguous(), c["ref"], f"strided rowgemm K={K} N={N}")
    for norm in (1, 2):
        for residual in (False, True):
            N = 256
            c = RR.exact_norm_rowgemm(R, N, norm, "cuda", seed=6, residual=residual)
            e = prep_linear(ops, c["Ws"][0], gamma=c["gamma"], bias=c["biases"][0], scalar_gain=norm == 2)
            y, xhat, rstd = obuf(R, N, N + 8), obuf(R, 256), obuf(R, dtype=torch.float32)
            ops.rowgemm(padded(c["x"], 264), e["Wp"], y, R, N, 256, ldx=264, ldy=N + 8, bias=e["bp"], ln=norm, xhat=xhat, rstd=rstd,
                        residual=padded(c["res"], N + 16) if residual else None, ldr=N + 16 if residual else 0)
            what = f"strided rowgemm ln={norm} res={residual}"
            RR.check_exact(done(y, R, N, what).contiguous(), c["refs"][0], what)
            RR.check_exact(done(xhat, R, 256, what), c["xhat"], f"{what} x_hat")
            done(rstd, R, 0, what)
        for K in (256, 512):
            dys, xhat, rstd, dres = bwd_operands(R, K, norm)
            _, WpT, _ = prep_groups(ops, [rnd(K, 256, seed=2, scale=K ** -0.5)], [1 + 0.3 * rnd(256 if norm == 1 else 1, seed=3).abs()], None, None,
                                    scalar_gain=norm == 2)
            packed, strided = obuf(R, 256), obuf(R, 256, 264)
            ops.rowgemm(dys[0], WpT[0], packed, R, 256, K, ldw=K, residual=dres, ldr=256, ln_bwd=norm, bwd_xhat=xhat, bwd_rstd=rstd)
            ops.rowgemm(padded(dys[0], K + 8), WpT[0], strided, R, 256, K, ldx=K + 8, ldw=K, ldy=264, residual=padded(dres, 272), ldr=272, ln_bwd=norm,
                        bwd_xhat=xhat, bwd_rstd=rstd)
            what = f"strided rowgemm ln_bwd={norm} K={K}"
            RR.check_exact(done(strided, R, 256, what).contiguous(), done(packed, R, 256, what).contiguous(), what)


def test_rowgemm_groups_strided(ops):
    R, G = R_LD, 2
    for norm in (1, 2):
        N = 256
        c = RR.exact_norm_rowgemm(R, N, norm, "cuda", seed=8, groups=G)
        Wp, _, bp = prep_groups(ops, c["Ws"], None if norm == 1 else [c["gamma"]] * G, None, c["biases"], scalar_gain=norm == 2)
        ys, xhat, rstd = [obuf(R, N, N + 8) for _ in range(G)], obuf(R, 256), obuf(R, dtype=torch.float32)
        ops.rowgemm_groups([padded(c["x"], 264)], [Wp[g] for g in range(G)], ys, R, N, 256, ldx=264, ldy=N + 8, biases=[bp[g] for g in range(G)], ln=norm,
                           xhat=xhat, rstd=rstd)
        what = f"strided groups fwd ln={norm}"
        for g in range(G):
            RR.check_exact(done(ys[g], R, N, what).contiguous(), c["refs"][g], f"{what} y[{g}]")
        RR.check_exact(done(xhat, R, 256, what), c["xhat"], f"{what} x_hat")
        K = 512
        dys, xhat, rstd, dres = bwd_operands(R, K, norm, groups=G)
        gam = [1 + 0.3 * rnd(256 if norm == 1 else 1, seed=40 + g).abs() for g in range(G)]
        _, WpT, _ = prep_groups(ops, [rnd(K, 256, seed=20 + g, scale=K ** -0.5) for g in range(G)], gam, None, None, scalar_gain=norm == 2)
        packed, strided = obuf(R, 256), obuf(R, 256, 264)
        ops.rowgemm_groups(dys, [WpT[g] for g in range(G)], [packed], R, 256, K, ldw=K, residual=dres, ldr=256, ln_bwd=norm, bwd_xhat=xhat, bwd_rstd=rstd)
        ops.rowgemm_groups([padded(d, K + 8) for d in dys], [WpT[g] for g in range(G)], [strided], R, 256, K, ldx=K + 8, ldw=K, ldy=264,
                           residual=padded(dres, 272), ldr=272, ln_bwd=norm, bwd_xhat=xhat, bwd_rstd=rstd)
        what = f"strided groups bwd ln_bwd={norm}"
        RR.check_exact(done(strided, R, 256, what).contiguous(), done(packed, R, 256, what).contiguous(), what)


def test_mlp_strided(ops):
    """ldx = ldy = lddy = lddx = 264 on the exact ReLU case (y, x_hat, t1, g, du bit for bit against the reference, dx against the
    packed launch) and on LayerNorm + GELU against the packed launch."""
    R = R_LD
    c = RR.exact_mlp(R, "cuda", seed=9)
    up, dn = prep_linear(ops, c["Wu"], bias=c["bu"]), prep_linear(ops, c["Wd"], bias=c["bd"])
    cases = [(c["x"], c["dy"], up, dn, RR.ACT_RELU)]
    up, dn = mlp_weights(ops, False)
    cases.append(((rnd(R, 256, seed=1) * 1.5 + rnd(R, 1, seed=2)).to(BF), rnd(R, 256, seed=77).to(BF), up, dn, RR.ACT_GELU))
    for x, dy, up, dn, kind in cases:
        y0, xh0, rs0, routes0 = run_mlp(ops, R, x, up, dn, dy, kind, 1)
        y1, xh1, rs1, routes1 = run_mlp(ops, R, x, up, dn, dy, kind, 1, ld=(264, 264, 264, 264))
        what = f"strided mlp act={kind}"
        RR.check_exact(y1.contiguous(), y0.contiguous(), f"{what} y")
        RR.check_exact(xh1, xh0, f"{what} x_hat")
        RR.check_exact(rs1, rs0, f"{what} rstd")
        for r0, r1 in zip(routes0, routes1):
            for a, b, name in zip(r0, r1, ("t1", "g", "du", "dx")):
                RR.check_exact(b.contiguous(), a.contiguous(), f"{what} {name}")
        if kind == RR.ACT_RELU:
            RR.check_exact(y1.contiguous(), c["y"], f"{what} y against the reference")
            RR.check_exact(routes1[1][2], c["du"], f"{what} du against the reference")
