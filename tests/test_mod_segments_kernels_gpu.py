"""The modality-segment kernels (MMFM_MOD_SEGMENTS in include/mmfm.h) on the MI355X.

At equal lengths, shared stamps and a shared attention mask every segment entry point must give the bits of its uniform counterpart.
For mask preparation and the stitch the two entry points run the same kernels (csrc/stitch.hip: one kernel set, the slot given by its
offset), so there these tests guard the entry points' offset arithmetic - m * T against the segment's own offset, the slot table of
mmfm_mask_prep against the one built from seg_T - not two kernels; for the LayerNorm it is the optional segment pack.  The independent
evidence is on ragged slots - lengths (8, 5, 1) and (1, 7), stamps with repeats and distinct per slot, per-slot padding - where the
segment entry points are compared with the fp64 references of tests/mod_segments_refs.py at the bounds tests/test_edge_kernels_gpu.py
holds the uniform ones to."""
import pytest
import torch

import edge_refs as E
import mod_segments_refs as S

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
GUARD, SENT = 4096, 0xA5
B, MAX_F = 3, 8
RAGGED = [(8, 5, 1), (1, 7)]


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def lib():
    from multi_modal_foundation_model_amd import _lib as L
    return L.lib()


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def rnd(*shape, seed=0, dtype=F32):
    return torch.randn(*shape, generator=gen(seed), device="cuda").to(dtype)


def nan(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def guarded(nbytes):
    buf = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[:nbytes]


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32 if a.dtype == F32 else a.dtype),
                       b.view(torch.int16 if b.dtype == BF16 else torch.int32 if b.dtype == F32 else b.dtype)), f"{what}: bits differ"


def mask_inputs(Ts, chans, seed=0):
    """Per slot an eval mask [B, T, channels] (the kernel reads [:, :, 0]: stride = channels) and an attention mask with right padding."""
    evals = [(torch.rand(B, T, c, generator=gen(seed + j), device="cuda") > 0.5).long() for j, (T, c) in enumerate(zip(Ts, chans))]
    attns = []
    for j, T in enumerate(Ts):
        a = torch.ones(B, T, dtype=torch.int64, device="cuda")
        if T > 2:
            a[j % B, T - 2:] = 0                        # two padded bins on sample j of slot j (sample 0 included)
        attns.append(a)
    return evals, attns


def run_mask_prep_seg(ops, Ts, evals, attns, chans):
    L, M = sum(Ts), len(Ts)
    out = [torch.full(s, 0xEE, dtype=torch.uint8, device="cuda") for s in ((B, L), (B, L), (L,), (L,))]
    count = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    ops.mask_prep_seg(B, Ts, evals, chans, attns, chans, *out, count)
    return out + [count]


# ------------------------------------------------------------------------------------------------- bit-identity at equal lengths
# (mask prep and stitch: both entry points launch the same kernels, these guard the offsets and tables they hand them)
def test_mask_prep_equal_lengths_is_uniform(ops):
    T, M, chans = 8, 2, [12, 2]
    evals, attns = mask_inputs((T,) * M, chans)
    attn = attns[1]
    uni = [torch.full(s, 0xEE, dtype=torch.uint8, device="cuda") for s in ((B, M * T), (B, M * T), (M * T,), (M * T,))]
    count = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    ops.mask_prep(B, T, evals, chans, attn, chans, *uni, count)
    for name, a, b in zip(("tokmask", "keypad", "keep0", "mod_id", "count"), run_mask_prep_seg(ops, (T,) * M, evals, [attn] * M, chans), uni + [count]):
        E.check_exact(a, b, f"mask_prep_seg at equal lengths: {name}")


def stitch_inputs(Ts, H, dtype, seed=0):
    L = sum(Ts)
    toks = [rnd(B * T, H, seed=seed + 10 + j, dtype=dtype) for j, T in enumerate(Ts)]
    rows = [rnd(H, seed=seed + 20 + j) for j in range(len(Ts))]
    poss = [rnd(MAX_F, H, seed=seed + 30 + j) for j in range(len(Ts))]
    tss = []
    for j, T in enumerate(Ts):                          # repeats inside a slot, another pattern per slot, one stamp out of range
        ts = (torch.arange(T, device="cuda")[None, :] * (j + 1) + torch.arange(B, device="cuda")[:, None] * 3 + j) % (MAX_F - 2)
        ts[B - 1, T - 1] = MAX_F + 5 if j % 2 else -3
        tss.append(ts.contiguous())
    keep0 = (torch.rand(L, generator=gen(seed + 50), device="cuda") > 0.3).to(torch.uint8)
    return toks, rows, poss, tss, keep0


def dropout_of(ops, n, H, dtype, p=0.2, site=5):
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 11)
    drop = ops.dropout(state, site, p)
    pattern = torch.empty(n, H, dtype=dtype, device="cuda")
    ops.dropout_apply(torch.ones(n, H, dtype=dtype, device="cuda"), pattern, n, H, drop)
    return drop, pattern != 0, state


@pytest.mark.parametrize("with_pos", [True, False], ids=["table", "notable"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [32, 64])
def test_stitch_equal_lengths_is_uniform(ops, H, dtype, with_pos):
    T, M = 8, 2
    L = M * T
    toks, rows, poss, tss, keep0 = stitch_inputs((T,) * M, H, dtype)
    ts = tss[1]
    dx, dextra = rnd(B, L, H, seed=40, dtype=dtype), rnd(B, L, H, seed=41, dtype=dtype)
    drop, _, _state = dropout_of(ops, B * T, H, dtype)
    code = ops.dt(dx)
    nbytes = lib().mmfm_stitch_bwd_workspace(code, B, T, L, H, MAX_F)
    xs, es = ([nan(B, L, H, dtype=dtype) for _ in range(2)] for _ in range(2))
    for m in range(M):
        pos = poss[m] if with_pos else None
        ops.stitch_fwd(toks[m], rows[m], pos, ts, keep0, xs[0], es[0], B, T, L, m, H, MAX_F)
        ops.stitch_fwd_seg(toks[m], rows[m], pos, ts, keep0, xs[1], es[1], B, T, L, m * T, H, MAX_F)
        assert lib().mmfm_stitch_bwd_seg_workspace(code, B, T, L, m * T, H, MAX_F) == nbytes
        for with_extra, with_drop, acc in ((True, True, True), (False, False, False)):
            outs = []
            for seg in (False, True):
                d_tok, d_mod, d_pos = nan(B * T, H, dtype=dtype), rnd(H, seed=50), rnd(MAX_F, H, seed=51)
                buf, ws = guarded(nbytes)
                args = (dx, dextra if with_extra else None, ts, keep0, drop if with_drop else None, d_tok, d_mod, d_pos if with_pos else None, acc, acc,
                        B, T, L)
                if seg:
                    ops.stitch_bwd_seg(*args, m * T, H, MAX_F, ws)
                else:
                    ops.stitch_bwd(*args, m, H, MAX_F, ws)
                assert bool((buf[nbytes:] == SENT).all()), "wrote behind the workspace"
                outs.append((d_tok, d_mod, d_pos))
            for name, a, b in zip(("d_tok", "d_mod", "d_pos"), outs[1], outs[0]):
                same_bits(a, b, f"stitch_bwd_seg at equal lengths m={m} extra={with_extra} drop={with_drop}: {name}")
    same_bits(xs[1], xs[0], "stitch_fwd_seg at equal lengths: x")
    same_bits(es[1], es[0], "stitch_fwd_seg at equal lengths: emb")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [32, 64])
def test_layernorm_destitch_equal_lengths_is_uniform(ops, H, dtype):
    T, M = 8, 2
    L, R = M * T, B * M * T
    x, g, b, dy, dres = rnd(R, H, seed=1, dtype=dtype), rnd(H, seed=2), rnd(H, seed=3), rnd(R, H, seed=4, dtype=dtype), rnd(R, H, seed=5, dtype=dtype)
    nbytes = lib().mmfm_layernorm_bwd_workspace(R, H)
    outs = []
    for seg in (False, True):
        y, mean, rstd, dx, dgb = nan(R, H, dtype=dtype), nan(R), nan(R), nan(R, H, dtype=dtype), nan(2 * H)
        buf, ws = guarded(nbytes)
        if seg:
            ops.layernorm_fwd_seg(x, g, b, y, mean, rstd, R, H, (T,) * M)
            ops.layernorm_bwd_seg(dy, x, mean, rstd, g, dres, dx, dgb[:H], dgb[H:], R, H, ws, (T,) * M)
        else:
            ops.layernorm_fwd(x, g, b, y, mean, rstd, R, H, ds_L=L, ds_T=T)
            ops.layernorm_bwd(dy, x, mean, rstd, g, dres, dx, dgb[:H], dgb[H:], R, H, ws, ds_L=L, ds_T=T)
        assert bool((buf[nbytes:] == SENT).all()), "wrote behind the workspace"
        outs.append((y, mean, rstd, dx, dgb))
    for name, a, b_ in zip(("y", "mean", "rstd", "dx", "dgamma|dbeta"), outs[1], outs[0]):
        same_bits(a, b_, f"layernorm_*_seg at equal lengths: {name}")


# ------------------------------------------------------------------------------------------------- ragged slots
@pytest.mark.parametrize("Ts", RAGGED)
def test_mask_prep_ragged(ops, Ts):
    chans = [12, 2, 4][:len(Ts)]
    evals, attns = mask_inputs(Ts, chans, seed=3)
    ref = S.mask_prep(evals, chans, attns, chans)
    assert int(ref[1].sum()) < B * sum(Ts) and 0 < int(ref[2].sum()) < sum(Ts)          # some padding, some of sample 0 masked
    for name, a, b in zip(("tokmask", "keypad", "keep0", "mod_id", "count"), run_mask_prep_seg(ops, Ts, evals, attns, chans), ref):
        E.check_exact(a, b, f"mask_prep_seg {Ts}: {name}")


@pytest.mark.parametrize("with_pos", [True, False], ids=["table", "notable"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("Ts", RAGGED)
def test_stitch_ragged(ops, Ts, H, dtype, with_pos):
    L, off = sum(Ts), S.offsets(Ts)
    toks, rows, poss, tss, keep0 = stitch_inputs(Ts, H, dtype, seed=100)
    x, emb = nan(B, L, H, dtype=dtype), nan(B, L, H, dtype=dtype)
    zero_pos = torch.zeros(MAX_F, H, device="cuda")
    for j, T in enumerate(Ts):
        ops.stitch_fwd_seg(toks[j], rows[j], poss[j] if with_pos else None, tss[j] if with_pos else None, keep0, x, emb, B, T, L, off[j], H, MAX_F)
        for out in (x, emb):
            assert bool(torch.isfinite(out[:, :off[j + 1]]).all()) and bool(torch.isnan(out[:, off[j + 1]:]).all()), f"slot {j} missed its slice"
    for j, T in enumerate(Ts):
        xr, er, mag = S.stitch_fwd(toks[j], rows[j], poss[j] if with_pos else zero_pos, tss[j], keep0, off[j], MAX_F)
        for name, out, ref in (("x", x, xr), ("emb", emb, er)):
            sl, what = out[:, off[j]:off[j + 1]], f"stitch_fwd_seg {Ts} slot {j} {name}"
            if dtype == BF16:
                E.check_bf16(sl, ref, E.stitch_fwd_e32(mag), what)
            else:
                E.check_close(sl, ref, E.TOL_STITCH, what)
    dx, dextra = rnd(B, L, H, seed=140, dtype=dtype), rnd(B, L, H, seed=141, dtype=dtype)
    code, p = ops.dt(dx), 0.2
    for j, T in enumerate(Ts):
        n = B * T
        drop, keep, _state = dropout_of(ops, n, H, dtype, p)
        nbytes = lib().mmfm_stitch_bwd_seg_workspace(code, B, T, L, off[j], H, MAX_F)
        assert nbytes > 0
        for with_extra, with_drop, acc_mod, acc_pos in ((True, True, True, False), (False, False, False, True)):
            what = f"stitch_bwd_seg {Ts} slot {j} dextra={with_extra} drop={with_drop} acc=({acc_mod},{acc_pos})"
            extra = dextra if with_extra else None
            prior_mod, prior_pos = rnd(H, seed=150), rnd(MAX_F, H, seed=151)
            runs = []
            for _ in range(2):                          # twice: d_pos and d_mod_row must come out with the same bits
                d_tok, d_mod, d_pos = nan(n, H, dtype=dtype), prior_mod.clone(), prior_pos.clone()
                buf, ws = guarded(nbytes)
                ops.stitch_bwd_seg(dx, extra, tss[j] if with_pos else None, keep0, drop if with_drop else None, d_tok, d_mod, d_pos if with_pos else None,
                                   acc_mod, acc_pos, B, T, L, off[j], H, MAX_F, ws)
                assert bool((buf[nbytes:] == SENT).all()), f"{what}: wrote behind its {nbytes}-byte workspace"
                runs.append((d_tok, d_mod, d_pos))
            same_bits(runs[0][1], runs[1][1], f"{what}: d_mod_row of two calls")
            same_bits(runs[0][2], runs[1][2], f"{what}: d_pos of two calls")
            r = S.stitch_bwd(dx, extra, tss[j], keep0, keep if with_drop else None, p, off[j], MAX_F)
            check_stitch_bwd(what, runs[0], (prior_mod, prior_pos), r, with_pos, with_extra, with_drop, acc_mod, acc_pos)


def check_stitch_bwd(what, outs, priors, r, with_pos, with_extra, with_drop, acc_mod, acc_pos):
    """(d_tok, d_mod, d_pos) of one stitch backward over (prior_mod, prior_pos) against the reference dict r, at edge_refs' bounds."""
    (d_tok, d_mod, d_pos), (prior_mod, prior_pos) = outs, priors
    sums = [("d_mod", d_mod, prior_mod, acc_mod, r["d_mod"], r["n_mod"], r["abs_mod"])]
    if with_pos:
        sums.append(("d_pos", d_pos, prior_pos, acc_pos, r["d_pos"], r["n_pos"], r["abs_pos"]))
    else:
        E.check_exact(d_pos, prior_pos, f"{what}: d_pos untouched without a table")
    for name, out, prior, acc, ref, cnt, sabs in sums:
        terr = E.U32 * sabs if with_extra else 0.0
        if acc:
            ref, cnt, sabs = ref + E.f64(prior), cnt + 1, sabs + E.f64(prior).abs()
        E.check_sum(out, ref, cnt, sabs, f"{what} {name}", term_err=terr)
    if with_drop:
        if d_tok.dtype == BF16:
            E.check_bf16(d_tok, r["d_tok"], E.DROP_SCALE_REL * r["d_tok"].abs(), f"{what} d_tok")
        else:
            E.check_close(d_tok, r["d_tok"], E.TOL_STITCH, f"{what} d_tok")
    else:
        E.check_exact(d_tok, r["d_tok"].to(d_tok.dtype), f"{what} d_tok")


@pytest.mark.parametrize("with_pos", [True, False], ids=["table", "notable"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stitch_bwd_many_samples(ops, dtype, with_pos):
    """300 samples of two 2-bin slots at H = 32: more samples than the 256 slabs the bf16 column sum (no table) takes, so a slab sums
    two samples and the last slab index is not B - 1, and for the per-column kernel (fp32) a grid of 300 chunks, inside the 512 its
    chunk count is clamped to.  Both entry points at the second slot's offset as well as the first, against their own references."""
    Bn, T, M, H, p = 300, 2, 2, 32, 0.2
    L = M * T
    dx, dextra = rnd(Bn, L, H, seed=240, dtype=dtype), rnd(Bn, L, H, seed=241, dtype=dtype)
    keep0 = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device="cuda")
    tss = [((torch.arange(T, device="cuda")[None, :] * (j + 2) + torch.arange(Bn, device="cuda")[:, None] * 3 + j) % (MAX_F + 2) - 1).contiguous()
           for j in range(M)]                           # -1 .. MAX_F: every table row and both clamps
    drop, keep, _state = dropout_of(ops, Bn * T, H, dtype, p)
    code = ops.dt(dx)
    nbytes = lib().mmfm_stitch_bwd_workspace(code, Bn, T, L, H, MAX_F)
    assert nbytes > 0 and lib().mmfm_stitch_bwd_seg_workspace(code, Bn, T, L, T, H, MAX_F) == nbytes
    for m in range(M):
        for with_extra, with_drop, acc_mod, acc_pos in ((True, True, True, False), (False, False, False, True)):
            extra = dextra if with_extra else None
            refs = dict(stitch_bwd=E.stitch_bwd(dx, extra, tss[m], keep0, keep if with_drop else None, p, m, MAX_F),
                        stitch_bwd_seg=S.stitch_bwd(dx, extra, tss[m], keep0, keep if with_drop else None, p, m * T, MAX_F))
            prior_mod, prior_pos = rnd(H, seed=250), rnd(MAX_F, H, seed=251)
            outs = {}
            for entry, where in (("stitch_bwd", m), ("stitch_bwd_seg", m * T)):
                what = f"{entry} B={Bn} slot {m} dextra={with_extra} drop={with_drop} acc=({acc_mod},{acc_pos})"
                d_tok, d_mod, d_pos = nan(Bn * T, H, dtype=dtype), prior_mod.clone(), prior_pos.clone()
                buf, ws = guarded(nbytes)
                getattr(ops, entry)(dx, extra, tss[m] if with_pos else None, keep0, drop if with_drop else None, d_tok, d_mod,
                                    d_pos if with_pos else None, acc_mod, acc_pos, Bn, T, L, where, H, MAX_F, ws)
                assert bool((buf[nbytes:] == SENT).all()), f"{what}: wrote behind its {nbytes}-byte workspace"
                outs[entry] = (d_tok, d_mod, d_pos)
                check_stitch_bwd(what, outs[entry], (prior_mod, prior_pos), refs[entry], with_pos, with_extra, with_drop, acc_mod, acc_pos)
            for name, a, b in zip(("d_tok", "d_mod", "d_pos"), outs["stitch_bwd_seg"], outs["stitch_bwd"]):
                same_bits(a, b, f"stitch_bwd_seg and stitch_bwd at B={Bn} slot {m}: {name}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("Ts", RAGGED)
def test_layernorm_destitch_ragged(ops, Ts, H, dtype):
    """The bounds of test_edge_kernels_gpu.py::test_layernorm_destitch."""
    R = B * sum(Ts)
    x, g, b = (rnd(R, H, seed=1) * 2.0).to(dtype), rnd(H, seed=2), rnd(H, seed=3)
    dy, dres = rnd(R, H, seed=4, dtype=dtype), rnd(R, H, seed=5, dtype=dtype)
    tag = f"layernorm_seg {Ts} H={H}"
    y, mean, rstd = nan(R, H, dtype=dtype), nan(R), nan(R)
    ops.layernorm_fwd_seg(x, g, b, y, mean, rstd, R, H, Ts)
    yr, mr, rr = S.layernorm_fwd(x, g, b, Ts)
    E.check_elem(y, yr, E.TOL_LN_Y, f"{tag} y")
    E.check_close(mean, mr, E.TOL_LN_Y, f"{tag} mean")
    E.check_close(rstd, rr, E.TOL_LN_RSTD, f"{tag} rstd")
    nbytes = lib().mmfm_layernorm_bwd_workspace(R, H)
    for with_dres, acc in ((False, False), (True, True)):
        what = f"{tag} bwd dres={with_dres} accumulate={acc}"
        prior = rnd(2 * H, seed=7)
        flat = prior.clone()
        dx = nan(R, H, dtype=dtype)
        buf, ws = guarded(nbytes)
        ops.layernorm_bwd_seg(dy, x, mean, rstd, g, dres if with_dres else None, dx, flat[:H], flat[H:], R, H, ws, Ts, accumulate=acc)
        assert bool((buf[nbytes:] == SENT).all()), f"{what}: wrote behind its workspace"
        r = S.layernorm_bwd(dy, x, g, dres if with_dres else None, Ts)
        E.check_elem(dx, r["dx"], E.TOL_LN_DX, f"{what} dx")
        for name, out, pr, ref, sabs, terr in (("dgamma", flat[:H], prior[:H], r["dgamma"], r["abs_gamma"], r["err_gamma"]),
                                               ("dbeta", flat[H:], prior[H:], r["dbeta"], r["abs_beta"], 0.0)):
            cnt = r["n"]
            if acc:
                ref, cnt, sabs = ref + E.f64(pr), cnt + 1, sabs + E.f64(pr).abs()
            E.check_sum(out, ref, cnt, sabs, f"{what} {name}", term_err=terr)
