"""Per-kernel fp64 parity of the edge kernels: stitch / destitch, mask preparation, the masked loss, LayerNorm, AdamW, the
bf16 cast and the fp32 reductions, at bf16 and fp32, at the default B = 1024 sizes and at odd shapes.  The references and
every bound are in tests/edge_refs.py (proved on the CPU by tests/test_edge_refs_cpu.py); the references run on the device
in fp64 so that the full-size cases stay quick.  Runs on the MI355X only."""
import pytest
import torch

import edge_refs as E
from oracle import mm_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
GUARD = 4096                 # bytes of sentinel behind every exactly-sized workspace
SENT = 0xA5


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def lib():
    from multi_modal_foundation_model_amd import _lib as L
    return L


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0, dtype=F32):
    return (torch.randn(*shape, generator=gen(seed), device="cuda") * scale).to(dtype)


def guarded(nbytes):
    """(whole buffer, the exactly-sized workspace view in front of its sentinel tail)."""
    buf = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[:nbytes]


def guard_intact(buf, nbytes, what):
    assert bool((buf[nbytes:] == SENT).all()), f"{what}: wrote behind its {nbytes}-byte workspace"


# ------------------------------------------------------------------------------------------------- stitch forward
@pytest.mark.parametrize("with_emb", [True, False], ids=["emb", "noemb"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,M,H,max_F", [(1024, 100, 2, 256, 100),      # the default step: 25600 blocks' worth on a 4096-block grid
                                           (256, 300, 2, 512, 300),       # config 5
                                           (3, 7, 3, 36, 9),              # M = 3, H % 8 != 0
                                           (2, 5, 2, 4, 1)])
def test_stitch_fwd(ops, B, T, M, H, max_F, dtype, with_emb):
    L, n = M * T, B * T
    ts = torch.randint(0, max_F, (B, T), generator=gen(3), device="cuda")
    ts.view(-1)[[0, n // 2]] = -3                                          # outside [0, max_F): the clamped gather
    ts.view(-1)[[1 % n, n - 1]] = max_F + 5
    keep0 = (torch.rand(L, generator=gen(4), device="cuda") > 0.3).to(torch.uint8)
    x = torch.full((B, L, H), float("nan"), dtype=dtype, device="cuda")
    emb = torch.full((B, L, H), float("nan"), dtype=dtype, device="cuda") if with_emb else None
    refs = []
    for m in range(M):
        tok, mod, pos = rnd(n, H, seed=10 + m, dtype=dtype), rnd(H, seed=20 + m), rnd(max_F, H, seed=30 + m)
        ops.stitch_fwd(tok, mod, pos, ts, keep0, x, emb, B, T, L, m, H, max_F)
        xr, er, mag = E.stitch_fwd(tok, mod, pos, ts, keep0, m, max_F)
        refs.append((xr, er, mag))
        for name, out in (("x", x), ("emb", emb)):
            if out is None:
                continue
            assert bool(torch.isfinite(out[:, :(m + 1) * T]).all()), f"{name}: modality {m} left positions unwritten"
            assert bool(torch.isnan(out[:, (m + 1) * T:]).all()), f"{name}: modality {m} wrote outside its slice"
    for m, (xr, er, mag) in enumerate(refs):                               # after all M calls: nothing was overwritten either
        for name, out, ref in (("x", x, xr), ("emb", emb, er)):
            if out is None:
                continue
            sl, what = out[:, m * T:(m + 1) * T], f"stitch_fwd {name} m={m}"
            if dtype == BF16:
                E.check_bf16(sl, ref, E.stitch_fwd_e32(mag), what)
            else:
                E.check_close(sl, ref, E.TOL_STITCH, what)


# ------------------------------------------------------------------------------------------------- stitch backward
# B = 300 gives more than one batch per chunk and empty trailing chunks in the fp32 scatter kernel.  With
# stitch_chunks(B, H, cw) = max(1, min(B, 512 / (H / cw))) and pick_cw's largest cw with H % cw == 0, max_F * cw * 4 <= 60 KB:
#   H = 256, max_F = 100: cw = 128, nch = min(300, 256) = 256, bper = 2 (chunks 150.. are empty)
#   H = 512, max_F = 100: cw = 128, nch = 128, bper = 3      H = 36, max_F = 9: cw = 4, nch = 56, bper = 6
#   H = 260, max_F = 200: cw = 4, nch = 512 / 65 = 7, bper = 43
# bf16 takes the one-hot GEMM at H = 256 / 512 and falls back to the scatter kernel at H = 36 / 260 (H % 8 != 0).
#           dextra  d_tok  drop   acc_mod acc_pos
VARIANTS = [(True,  True,  False, False, False),
            (True,  True,  True,  True,  False),
            (False, True,  False, False, True),
            (True,  False, False, True,  True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,max_F", [(300, 20, 256, 100), (300, 20, 512, 100), (300, 20, 36, 9), (300, 20, 260, 200),
                                         (1024, 100, 256, 100)])          # the default step: one variant, with dropout
def test_stitch_bwd(ops, B, T, H, max_F, dtype):
    Lb = lib()
    M, p, site = 2, 0.2, 5
    L, n = M * T, B * T
    ts = torch.randint(0, max_F, (B, T), generator=gen(3), device="cuda")
    ts.view(-1)[[0, n - 1]] = torch.tensor([-3, max_F + 5], device="cuda")
    keep0 = (torch.rand(L, generator=gen(4), device="cuda") > 0.3).to(torch.uint8)
    dx, dextra = rnd(B, L, H, seed=40, dtype=dtype), rnd(B, L, H, seed=41, dtype=dtype)
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 11)
    drop = ops.dropout(state, site, p)
    pattern = torch.empty(n, H, dtype=dtype, device="cuda")               # what dropout_apply keeps for (state, site) over [B*T, H]
    ops.dropout_apply(torch.ones(n, H, dtype=dtype, device="cuda"), pattern, n, H, drop)
    keep = pattern != 0
    assert 0.75 < keep.float().mean().item() < 0.85
    nbytes = Lb.lib().mmfm_stitch_bwd_workspace(ops.dt(dx), B, T, L, H, max_F)
    assert nbytes > 0
    variants = VARIANTS[1:2] if B == 1024 else VARIANTS
    for m in range(M):
        for with_extra, with_tok, with_drop, acc_mod, acc_pos in variants:
            what = f"stitch_bwd m={m} dextra={with_extra} d_tok={with_tok} drop={with_drop} acc=({acc_mod},{acc_pos})"
            extra = dextra if with_extra else None
            d_tok = torch.full((n, H), float("nan"), dtype=dtype, device="cuda") if with_tok else None
            prior_mod, prior_pos = rnd(H, seed=50), rnd(max_F, H, seed=51)
            d_mod, d_pos = prior_mod.clone(), prior_pos.clone()
            buf, ws = guarded(nbytes)
            ops.stitch_bwd(dx, extra, ts, keep0, drop if with_drop else None, d_tok, d_mod, d_pos, acc_mod, acc_pos, B, T, L, m, H, max_F, ws)
            guard_intact(buf, nbytes, what)
            r = E.stitch_bwd(dx, extra, ts, keep0, keep if with_drop else None, p, m, max_F)
            # e = dx + dextra is one fp32 addition per term in the scatter kernel (none in the one-hot GEMM): 2^-24 |term|
            for name, out, prior, acc, ref, cnt, sabs in (("d_mod", d_mod, prior_mod, acc_mod, r["d_mod"], r["n_mod"], r["abs_mod"]),
                                                          ("d_pos", d_pos, prior_pos, acc_pos, r["d_pos"], r["n_pos"], r["abs_pos"])):
                terr = E.U32 * sabs if with_extra else 0.0
                if acc:
                    ref, cnt, sabs = ref + E.f64(prior), cnt + 1, sabs + E.f64(prior).abs()
                E.check_sum(out, ref, cnt, sabs, f"{what} {name}", term_err=terr)
            if not with_tok:
                continue
            if with_drop:
                g = dx[:, m * T:(m + 1) * T].reshape(n, H)
                expect = keep & (keep0[m * T:(m + 1) * T].repeat(B)[:, None] != 0) & (g != 0)
                assert torch.equal(d_tok != 0, expect), f"{what}: d_tok's non-zero pattern is not dropout_apply's"
                if dtype == BF16:
                    E.check_bf16(d_tok, r["d_tok"], E.DROP_SCALE_REL * r["d_tok"].abs(), f"{what} d_tok")
                else:
                    E.check_close(d_tok, r["d_tok"], E.TOL_STITCH, f"{what} d_tok")
            else:
                E.check_exact(d_tok, r["d_tok"].to(dtype), f"{what} d_tok")      # a copy or a zero: no rounding at all


# ------------------------------------------------------------------------------------------------- mask preparation
@pytest.mark.parametrize("attn_hi", [1, 3])       # 3: valid steps carry attn = 1 or 3, so v = mask & attn reaches 2 and 3
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("B,T,M", [(1024, 100, 2),    # 204800 elements on a 256 x 256 grid: the grid-stride loop, counts from every wave
                                   (64, 600, 2), (7, 5, 8), (1, 1, 1)])
def test_mask_prep(ops, B, T, M, stride, attn_hi):
    L = M * T
    g = gen(5)
    lens = torch.randint(1, T + 1, (B,), generator=g, device="cuda")                    # a ragged tail of padding per sample
    valid = torch.arange(T, device="cuda")[None, :] < lens[:, None]
    hi = torch.randint(0, 2, (B, T), generator=g, device="cuda") * (attn_hi - 1) + 1     # 1, or 1 / attn_hi
    attn = (valid * hi).to(torch.int64)
    masks = [torch.randint(0, 4, (B, T, stride), generator=g, device="cuda") for _ in range(M)]
    channels = [668, 2, 5, 1, 7, 3, 11, 13][:M]
    tok, kpd = torch.full((B, L), 9, dtype=torch.uint8, device="cuda"), torch.full((B, L), 9, dtype=torch.uint8, device="cuda")
    keep0, mod = torch.full((L,), 9, dtype=torch.uint8, device="cuda"), torch.full((L,), 9, dtype=torch.uint8, device="cuda")
    cnt = torch.full((M,), 123456789, dtype=torch.int64, device="cuda")                 # the call zeroes its counters itself
    ops.mask_prep(B, T, masks, [stride] * M, attn, channels, tok, kpd, keep0, mod, cnt)
    refs = E.mask_prep(masks, [stride] * M, attn, channels)
    for name, out, ref in zip(("tokmask", "keypad", "keep0", "mod_id", "count"), (tok, kpd, keep0, mod, cnt), refs):
        E.check_exact(out, ref, f"mask_prep {name}")
    ops.mask_prep(B, T, masks, [stride] * M, attn, channels, tok, kpd, keep0, mod, cnt)  # into the same, now non-zero, counters
    E.check_exact(cnt, refs[4], "mask_prep count, second call")


# ------------------------------------------------------------------------------------------------- masked loss
def _row_masks(B, T, M):
    """[B, M*T] token masks; the loss reads modality 1's slice (mask_ld = M*T)."""
    R = B * T
    bern = (torch.rand(B, M * T, generator=gen(6), device="cuda") < 0.3).to(torch.uint8)
    ones = torch.ones(B, M * T, dtype=torch.uint8, device="cuda")
    other_only = ones.clone()
    other_only[:, T:] = 0                                                  # nothing of this modality, the other has rows
    edges = torch.zeros(R, dtype=torch.uint8, device="cuda")             # single rows at the ends of the grid-stride ranges: a
    edges[[r for r in (0, 4095, 4096, R - 2, R - 1) if 0 <= r < R]] = 1    # dropped row is the whole sum here, far outside n u sum|t|
    e2 = torch.zeros(B, M * T, dtype=torch.uint8, device="cuda")
    e2[:, T:] = edges.view(B, T)
    return [("bernoulli", bern), ("all", ones), ("none of this modality", other_only), ("edge rows", e2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,R,N,T", [(0, 102400, 668, 100),            # the default step's spike head (Poisson only at this size)
                                        (0, 102400, 2, 100), (1, 102400, 2, 100), (0, 4100, 12, 100), (1, 4100, 12, 100),
                                        (0, 60, 668, 10), (1, 60, 668, 10)])
def test_masked_loss(ops, kind, R, N, T, dtype):
    Lb = lib()
    B, M = R // T, 2
    pred = (rnd(R, N, seed=1, scale=2.5).clamp_(-8.0, 8.0)).to(dtype)      # |pred| reaches 8: exp(p) up to 2981 dominates the sum
    assert pred.abs().max().item() >= 7.0 or R * N < 10000
    tgt = torch.poisson(torch.full((R, N), 0.3, device="cuda"), generator=gen(2)) if kind == 0 else rnd(R, N, seed=2)
    nbytes = Lb.lib().mmfm_masked_loss_workspace(R, N)
    gout = torch.tensor([0.5], device="cuda")
    other_sum, other_n = 3.0, 7
    for name, tokmask in _row_masks(B, T, M):
        what = f"masked_loss kind={kind} [{R}x{N}] {name}"
        rowmask = tokmask[:, T:]
        out = torch.full((1,), float("nan"), device="cuda")
        buf, ws = guarded(nbytes)
        ops.masked_loss_fwd(kind, pred, tgt, rowmask, M * T, T, R, N, out, ws)
        guard_intact(buf, nbytes, what)
        s, n, sabs, terr = E.masked_loss_sum(kind, pred, tgt, rowmask)
        E.check_sum(out, s.reshape(1), n, sabs, f"{what} sum", term_err=terr)
        if n == 0:
            assert out.item() == 0.0
        sums = torch.stack([torch.tensor(other_sum, device="cuda"), out[0]])
        cnt = torch.tensor([other_n, int(rowmask.sum().item()) * N], dtype=torch.int64, device="cuda")
        loss, inv_n = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        ops.loss_finalize(sums, cnt, 2, loss, inv_n)
        lr, ir = E.loss_finalize(sums, cnt)
        E.check_close(loss, lr.reshape(1), E.TOL_LOSS, f"{what} loss")
        E.check_close(inv_n, ir.reshape(1), (3 * E.U32, 0.0), f"{what} inv_n")   # (float)n, then 1 / it: two roundings (3 with slack)
        dpred = torch.full((R, N), 7.0, dtype=dtype, device="cuda")
        ops.masked_loss_bwd(kind, pred, tgt, rowmask, M * T, T, R, N, gout, inv_n, dpred)
        ref = E.masked_loss_bwd(kind, pred, tgt, rowmask, gout, inv_n)
        E.check_elem(dpred, ref, E.TOL_DPRED, f"{what} dpred")
        off = (rowmask == 0).reshape(R)
        assert bool((dpred[off] == 0).all()), f"{what}: dpred must be exactly zero on un-masked rows"
    # nothing masked in any modality: 0 / 0 = NaN, inv_n = inf, and every gradient NaN
    none = torch.zeros(B, M * T, dtype=torch.uint8, device="cuda")
    loss, inv_n = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    ops.loss_finalize(torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), 2, loss, inv_n)
    lr, ir = E.loss_finalize(torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"))
    assert bool(torch.isnan(loss[0])) and bool(torch.isnan(lr)) and bool(torch.isinf(inv_n[0])) and bool(torch.isinf(ir))
    dpred = torch.full((R, N), 7.0, dtype=dtype, device="cuda")
    ops.masked_loss_bwd(kind, pred, tgt, none[:, T:], M * T, T, R, N, gout, inv_n, dpred)
    assert bool(torch.isnan(E.masked_loss_bwd(kind, pred, tgt, none[:, T:], gout, inv_n)).all())
    assert bool(torch.isnan(dpred).all()), "nothing masked: dpred must be NaN everywhere"


# ------------------------------------------------------------------------------------------------- LayerNorm
def _ln_inputs(R, H, dtype):
    x = rnd(R, H, seed=1, scale=2.0)
    x[0] = 2.0                                                             # variance 0: eps alone sets rstd = 1e5 ** 0.5
    if R > 1:
        x[1] = (x[1] + 6.0) * 1e4                                          # magnitude 1e4 (mean 6e4, deviation 2e4)
    return x.to(dtype), rnd(H, seed=2), rnd(H, seed=3), rnd(R, H, seed=4, dtype=dtype), rnd(R, H, seed=5, dtype=dtype)


def _ln_fwd_bwd(ops, R, H, dtype, variants, dsL=0, dsT=0):
    Lb = lib()
    x, g, b, dy, dres = _ln_inputs(R, H, dtype)
    tag = f"layernorm [{R}x{H}]" + (f" destitch L={dsL} T={dsT}" if dsT else "")
    y = torch.full((R, H), float("nan"), dtype=dtype, device="cuda")
    mean, rstd = torch.full((R,), float("nan"), device="cuda"), torch.full((R,), float("nan"), device="cuda")
    ops.layernorm_fwd(x, g, b, y, mean, rstd, R, H, ds_L=dsL, ds_T=dsT)
    yr, mr, rr = E.layernorm_fwd(x, g, b, 1e-5, dsL, dsT)
    E.check_elem(y, yr, E.TOL_LN_Y, f"{tag} y")
    E.check_close(mean, mr, E.TOL_LN_Y, f"{tag} mean")
    E.check_close(rstd, rr, E.TOL_LN_RSTD, f"{tag} rstd")
    nbytes = Lb.lib().mmfm_layernorm_bwd_workspace(R, H)
    for with_dres, acc, packed in variants:
        what = f"{tag} bwd dres={with_dres} accumulate={acc} packed={packed}"
        prior = rnd(2 * H, seed=7)
        if packed:                                                         # dbeta == dgamma + H: the single [2H] reduction
            flat = prior.clone()
            dg, db = flat[:H], flat[H:]
        else:                                                              # two tensors, H floats apart: never dgamma + H
            flat = torch.cat([prior[:H], torch.zeros(H, device="cuda"), prior[H:]])
            dg, db = flat[:H], flat[2 * H:]
        dx = torch.full((R, H), float("nan"), dtype=dtype, device="cuda")
        buf, ws = guarded(nbytes)
        ops.layernorm_bwd(dy, x, mean, rstd, g, dres if with_dres else None, dx, dg, db, R, H, ws, accumulate=acc, ds_L=dsL, ds_T=dsT)
        guard_intact(buf, nbytes, what)
        r = E.layernorm_bwd(dy, x, g, dres if with_dres else None, 1e-5, dsL, dsT)
        E.check_elem(dx, r["dx"], E.TOL_LN_DX, f"{what} dx")
        for name, out, pr, ref, sabs, terr in (("dgamma", dg, prior[:H], r["dgamma"], r["abs_gamma"], r["err_gamma"]),
                                               ("dbeta", db, prior[H:], r["dbeta"], r["abs_beta"], 0.0)):
            cnt = r["n"]
            if acc:
                ref, cnt, sabs = ref + E.f64(pr), cnt + 1, sabs + E.f64(pr).abs()
            E.check_sum(out, ref, cnt, sabs, f"{what} {name}", term_err=terr)


#               dres   accumulate  dgamma / dbeta in one [2H] buffer
LN_VARIANTS = [(True, False, False), (False, True, True), (True, True, False), (False, False, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,H", [(204800, 256),                            # the default step's [B*L, H]
                                 (20000, 512),                             # 1250 row groups of 16: above the backward's 1024-block cap
                                 (77, 260), (33, 516), (9, 772),           # the last 256-column chunk part-filled
                                 (5, 1024), (1, 4)])
def test_layernorm(ops, R, H, dtype):
    _ln_fwd_bwd(ops, R, H, dtype, LN_VARIANTS[:2] if R >= 20000 else LN_VARIANTS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,M,T,H", [(1024, 2, 100, 256), (3, 3, 5, 36)])
def test_layernorm_destitch(ops, B, M, T, H, dtype):
    _ln_fwd_bwd(ops, B * M * T, H, dtype, [(False, False, True), (True, True, False)], dsL=M * T, dsT=T)


# ------------------------------------------------------------------------------------------------- AdamW and the bf16 cast
@pytest.mark.parametrize("with_bf16", [True, False], ids=["pbf16", "nopbf16"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
@pytest.mark.parametrize("n", [10007, 4096 * 256 * 2 + 13])               # the second: two trips of the 4096 x 256 grid and a tail
def test_adamw(ops, n, grad_scale, with_bf16):
    p0 = rnd(n, seed=1)
    starts = [(1, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")),                     # a fresh optimiser
              (4, rnd(n, seed=2, scale=0.01), torch.rand(n, generator=gen(3), device="cuda") * 1e-3)]  # moments coming in
    for first, m0, v0 in starts:
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        pr, mr, vr = E.f64(p0), E.f64(m0), E.f64(v0)
        pb = torch.full((n,), float("nan"), dtype=BF16, device="cuda") if with_bf16 else None
        for step in range(first, first + 5):
            g = rnd(n, seed=100 + step, scale=0.1)
            lr, b1 = O.onecycle(step - 1, 100)
            hyper = torch.tensor(E.adamw_hyper(step, lr, b1, grad_scale=grad_scale), dtype=F32, device="cuda")
            ops.adamw_step(p, g, m, v, pb, n, hyper)
            E.adamw_step(pr, g, mr, vr, hyper)                             # the reference sees g * grad_scale through hyper[7]
            E.check_close(p, pr, E.TOL_ADAMW, f"adamw n={n} scale={grad_scale} start={first} step {step}")
            if with_bf16:
                E.check_exact(E.bits(pb), E.bits(p.to(BF16)), f"adamw p_bf16, step {step}")   # a rounding of the same value


def _cast(ops, x):
    out = torch.full(x.shape, float("nan"), dtype=BF16, device="cuda")
    ops.cast_bf16(x, out, x.numel())
    return out


@pytest.mark.parametrize("n", [1, 7, 3 * 2 ** 20 + 5])
def test_cast_f32_to_bf16_random(ops, n):
    x = rnd(n, seed=n, scale=3.0)
    E.check_exact(E.bits(_cast(ops, x)), E.bits(x.to(BF16)), f"cast n={n}")


def test_cast_f32_to_bf16_special_values(ops):
    u = 2.0 ** -8                                                          # half a bf16 ulp at 1.0
    vals = [1.0 + u, 1.0 + 3 * u, -(1.0 + u), -(1.0 + 3 * u),              # exact ties: to even, down (1.0) and up (1 + 4u)
            1.0 + u + 2.0 ** -23, 1.0 + u - 2.0 ** -23,                    # one fp32 ulp off a tie
            3.4028234663852886e38, -3.4028234663852886e38,                 # the largest finite float rounds to inf
            3.3895313892515355e38,                                         # the largest finite bf16 stays
            float("inf"), float("-inf"), 0.0, -0.0,
            2.0 ** -126, 2.0 ** -127, 2.0 ** -130, -(2.0 ** -133), 2.0 ** -134, 2.0 ** -149, 1.5 * 2.0 ** -133]   # fp32 / bf16 subnormals
    x = torch.tensor(vals, dtype=F32, device="cuda")
    assert torch.equal(x.cpu(), torch.tensor(vals, dtype=F32)), "the inputs must reach the device unflushed"
    out = _cast(ops, x)
    # x.to(torch.bfloat16) taken on the host: IEEE round to nearest even with subnormals kept, whatever mode a device build flushes in
    E.check_exact(E.bits(out).cpu(), E.bits(torch.tensor(vals, dtype=F32).to(BF16)), "cast, special values")
    nan = torch.tensor([float("nan"), -float("nan"), 1.0], device="cuda")
    assert _cast(ops, nan).isnan().tolist() == [True, True, False]


# ------------------------------------------------------------------------------------------------- colsum / slab reductions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,N", [(3200, 256), (1001, 668), (64, 2), (51200, 768), (333, 1336), (204800, 256), (102400, 668), (1000, 7)])
def test_colsum(ops, R, N, dtype):
    Lb = lib()
    ld = N if R > 50000 else N + 4                                         # a row stride larger than N on the small shapes
    xs = rnd(R, ld, seed=10, dtype=dtype)
    x = xs[:, :N]
    nbytes = Lb.lib().mmfm_colsum_workspace(R, N)
    prior = rnd(N, seed=11)
    out = prior.clone()
    buf, ws = guarded(nbytes)
    ops.colsum(xs, R, N, ld, out, ws)
    guard_intact(buf, nbytes, "colsum")
    s, n, a = E.colsum(x)
    E.check_sum(out, s, n, a, f"colsum [{R}x{N}] ld={ld}")               # stored values: no per-term error
    out = prior.clone()
    ops.colsum(xs, R, N, ld, out, ws, accumulate=True)
    s, n, a = E.colsum(x, prior)
    E.check_sum(out, s, n, a, f"colsum [{R}x{N}] accumulate")


@pytest.mark.parametrize("n,nslabs,stride", [(1000, 7, 1000), (1001, 5, 1027),      # n % 4 != 0: the scalar kernel, stride > n
                                             (25700, 100, 25856),                   # tall-skinny: the two-stage path (groups of slabs)
                                             (512, 1024, 512), (2 * 256, 1024, 2 * 256 + 64),    # LayerNorm's [nblk][2H] partials
                                             (196608, 3, 196608), (4, 1, 4), (4, 16, 8)])
def test_reduce_slabs(ops, n, nslabs, stride):
    src = rnd(nslabs * stride, seed=12)
    prior = rnd(n, seed=13)
    for acc in (False, True):
        what = f"reduce_slabs n={n} nslabs={nslabs} stride={stride} accumulate={acc}"
        s, cnt, a = E.reduce_slabs(src, n, nslabs, stride, prior if acc else None)
        scratch, out = src.clone(), prior.clone()                          # the call may clobber its source
        ops.reduce_slabs(out, scratch, n, nslabs, stride, accumulate=acc)
        E.check_sum(out, s, cnt, a, what)


def test_reduce_slabs_multi(ops):
    shapes = [(1000, 7, 1000), (1001, 5, 1027), (3, 2, 300), (256, 64, 512), (70000, 3, 70016)]      # strides larger than n included
    items, refs = [], []
    for i, (n, nslabs, stride) in enumerate(shapes):
        src, prior, acc = rnd(nslabs * stride, seed=20 + i), rnd(n, seed=30 + i), bool(i % 2)
        refs.append(E.reduce_slabs(src, n, nslabs, stride, prior if acc else None))
        items.append((prior.clone(), src, n, nslabs, stride, acc))
    ops.reduce_slabs_multi(items, "cuda")
    for (out, *_), (s, cnt, a), shape in zip(items, refs, shapes):
        E.check_sum(out, s, cnt, a, f"reduce_slabs_multi entry {shape}")
