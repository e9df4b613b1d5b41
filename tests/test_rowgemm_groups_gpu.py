"""mmfm_rowgemm_groups: the row-owner linear over several weight sets in one launch (the context side of cross-attention).

Forward: every group's output, x_hat and rstd must be the bits the per-group mmfm_rowgemm(ln) launches write.  Backward: the summed
product behind one norm-backward epilogue, against the fp64 formula and against today's chain of per-group launches (each adding into the
previous one's bf16 output), whose error it may not exceed: the grouped launch rounds to bf16 once, the chain once per group."""
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
    return float((a - b).norm() / (b.norm() + 1e-30))


def prep_groups(ops, Ws, gammas, betas, biases, scalar_gain=False):
    """The prepared weights of all groups as slices of one tensor each (Wp [G][N][K], WpT [G][K][N], bp [G][N]): the grouped launch
    addresses every group's weights through one buffer."""
    G, (N, K) = len(Ws), Ws[0].shape
    Wp, WpT, bp = torch.empty(G, N, K, device="cuda", dtype=BF), torch.empty(G, K, N, device="cuda", dtype=BF), torch.empty(G, N, device="cuda")
    es = [dict(W=Ws[g], gamma=gammas[g], beta=None if betas is None else betas[g], bias=None if biases is None else biases[g],
               Wp=Wp[g], WpT=WpT[g], bp=bp[g], scalar_gain=scalar_gain) for g in range(G)]
    table, n, tiles = ops.prep_table(es, "cuda")
    ops.prep_weights(table, n, tiles)
    torch.cuda.synchronize()
    return Wp, WpT, bp


def norm_ref(xd, norm):
    """fp64 x_hat and rstd of the LayerNorm (1) / ScaleNorm (2) prologue."""
    if norm == 1:
        mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
        rs = 1 / torch.sqrt(var + 1e-5)
        return (xd - mu) * rs, rs.squeeze(1)
    rs = 1 / xd.norm(dim=1, keepdim=True).clamp_min(1e-5)
    return xd * rs, rs.squeeze(1)


FWD_CASES = [(77, 2, 512, 1), (300, 5, 512, 1), (1000, 3, 256, 1), (129, 1, 512, 1), (300, 5, 512, 2)]


@pytest.mark.parametrize("R,G,N,norm", FWD_CASES)
def test_groups_forward(ops, R, G, N, norm):
    """R = 77 / 129: a ragged last pass; every R here is small enough for the column-block split (fewer than 128 row passes), whose
    blocks straddle the groups; G = 1 is the plain launch."""
    x = (rnd(R, 256, seed=1) * 2 + rnd(R, 1, seed=5) * 3).to(BF)       # non-zero row means
    Ws = [rnd(N, 256, seed=10 + g, scale=1 / 16) for g in range(G)]
    biases = [rnd(N, seed=30 + g) for g in range(G)]
    if norm == 1:
        gam, bet = [1 + 0.3 * rnd(256, seed=50 + g) for g in range(G)], [0.2 * rnd(256, seed=70 + g) for g in range(G)]
    else:
        gam, bet = [1 + 0.3 * rnd(1, seed=50 + g).abs() for g in range(G)], None
    Wp, _, bp = prep_groups(ops, Ws, gam, bet, biases, scalar_gain=norm == 2)
    ys = [torch.full((R + 2, N), 9.0, device="cuda", dtype=BF) for _ in range(G)]
    xhat, rstd = torch.full((R + 2, 256), 9.0, device="cuda", dtype=BF), torch.full((R + 2,), 9.0, device="cuda")
    ops.rowgemm_groups([x], [Wp[g] for g in range(G)], ys, R, N, 256, biases=[bp[g] for g in range(G)], ln=norm, xhat=xhat, rstd=rstd,
                       stream_out=True)
    xd = x.double()
    xh_ref, rs_ref = norm_ref(xd, norm)
    for g in range(G):
        y1, xh1, rs1 = torch.empty(R, N, device="cuda", dtype=BF), torch.empty(R, 256, device="cuda", dtype=BF), torch.empty(R, device="cuda")
        ops.rowgemm(x, Wp[g], y1, R, N, 256, bias=bp[g], ln=norm, xhat=xh1, rstd=rs1, stream_out=True)
        assert torch.equal(ys[g][:R], y1), f"group {g}: y differs from the per-group launch"
        assert torch.equal(xhat[:R], xh1) and torch.equal(rstd[:R], rs1), f"group {g}: x_hat / rstd differ from the per-group launch"
        if norm == 1:
            ref = F.layer_norm(xd, (256,), gam[g].double(), bet[g].double(), 1e-5) @ Ws[g].double().T + biases[g].double()
        else:
            ref = (xh_ref * gam[g].double()) @ Ws[g].double().T + biases[g].double()
        err = relerr(ys[g][:R], ref)
        print(f"forward R={R} G={G} N={N} norm={norm} group {g}: relative L2 error {err:.3e}")
        assert err < 6e-3
        assert torch.all(ys[g][R:] == 9.0)
    assert torch.all(xhat[R:] == 9.0) and torch.all(rstd[R:] == 9.0)
    torch.testing.assert_close(rstd[:R].double(), rs_ref, rtol=1e-5, atol=1e-6)
    # without the side outputs (the forward-only plan): the same y
    ys2 = [torch.empty(R, N, device="cuda", dtype=BF) for _ in range(G)]
    ops.rowgemm_groups([x], [Wp[g] for g in range(G)], ys2, R, N, 256, biases=[bp[g] for g in range(G)], ln=norm)
    assert all(torch.equal(ys2[g], ys[g][:R]) for g in range(G))


BWD_CASES = [(129, 2, 512, 1), (300, 5, 512, 1), (1000, 3, 256, 1), (33, 1, 512, 1), (300, 5, 512, 2)]


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("R,G,K,norm", BWD_CASES)
def test_groups_backward(ops, R, G, K, norm, with_res):
    dys = [rnd(R, K, seed=1 + g).to(BF) for g in range(G)]
    Ws = [rnd(K, 256, seed=20 + g, scale=K ** -0.5) for g in range(G)]
    gam = [1 + 0.3 * rnd(256 if norm == 1 else 1, seed=40 + g).abs() for g in range(G)]
    Wp, WpT, _ = prep_groups(ops, Ws, gam, None, None, scalar_gain=norm == 2)
    x = rnd(R, 256, seed=4) * 1.7 + 0.5
    xh64, rs64 = norm_ref(x.double(), norm)
    rstd, xhat = rs64.float().contiguous(), xh64.to(BF).contiguous()
    dres = rnd(R, 256, seed=5).to(BF) if with_res else None
    dx = torch.full((R + 2, 256), 5.0, device="cuda", dtype=BF)
    ops.rowgemm_groups(dys, [WpT[g] for g in range(G)], [dx], R, 256, K, ldw=K, residual=dres, ldr=256 if with_res else 0, ln_bwd=norm,
                       bwd_xhat=xhat, bwd_rstd=rstd)
    # today's chain: one launch per group, each adding into the previous one's bf16 output
    chain = torch.empty(R, 256, device="cuda", dtype=BF)
    for g in range(G):
        res = dres if g == 0 else chain
        ops.rowgemm(dys[g], WpT[g], chain, R, 256, K, ldw=K, residual=res, ldr=256 if res is not None else 0, ln_bwd=norm, bwd_xhat=xhat,
                    bwd_rstd=rstd)
    v = sum(dys[g].double() @ Wp[g].double() for g in range(G))        # d x_hat
    xh = xhat.double()
    if norm == 1:
        ref = rstd.double()[:, None] * (v - v.mean(1, keepdim=True) - xh * (v * xh).mean(1, keepdim=True))
    else:
        ref = rstd.double()[:, None] * (v - xh * (v * xh).sum(1, keepdim=True))
    if with_res:
        ref = ref + dres.double()
    e_grp, e_chain = relerr(dx[:R], ref), relerr(chain, ref)
    print(f"backward R={R} G={G} K={K} norm={norm} res={with_res}: grouped {e_grp:.3e}, chain of per-group launches {e_chain:.3e}")
    assert e_grp < 5e-3
    assert e_grp <= e_chain
    assert torch.all(dx[R:] == 5.0)


def test_groups_refuses_bad_arguments(ops):
    from multi_modal_foundation_model_amd._lib import MmfmError
    x, W, y = torch.zeros(64, 256, device="cuda", dtype=BF), torch.zeros(9, 512, 256, device="cuda", dtype=BF), torch.zeros(64, 512, device="cuda", dtype=BF)
    with pytest.raises(MmfmError):          # neither a norm prologue nor a norm backward
        ops.rowgemm_groups([x], [W[0]], [y], 64, 512, 256)
    with pytest.raises(MmfmError):          # the biases of 6 x 512 outputs do not fit
        ops.rowgemm_groups([x], [W[g] for g in range(6)], [y] * 6, 64, 512, 256, ln=1)
    with pytest.raises(ValueError):         # more than 8 groups
        ops.rowgemm_groups([x], [W[g] for g in range(9)], [y] * 9, 64, 512, 256, ln=1)
