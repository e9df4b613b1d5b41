"""The per-sample token-mask kernels (MMFM_TOKEN_MASK_ROWS in include/mmfm.h) on the MI355X: B = 3, slots of 8, 5 and 1 bins, H = 32,
fp32 and bf16, guard bytes and NaN sentinels as in tests/test_mod_segments_kernels_gpu.py.

mmfm_mask_prep_rows is bit-exact against the torch restatement of tests/per_sample_mask.py (proved on the CPU by
tests/test_per_sample_mask_cpu.py) and, in the outputs it shares with them, against mmfm_mask_prep / mmfm_mask_prep_seg.  The stitch
pair gives the bits of the _seg and _live entry points at keep_ld = 0; under a per-sample mask it meets the restatement at the bounds
tests/test_mod_segments_kernels_gpu.py holds the same kernels to, writes exact zeros to d_tok at masked rows - the compact rows of a live
bin that a sample masks included - and draws the dropout decisions of the existing forms."""
import pytest
import torch

import edge_refs as E
import per_sample_mask as P

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
GUARD, SENT = 4096, 0xA5
B, MAX_F, H = 3, 8, 32
TS = (8, 5, 1)
OFF = (0, 8, 13, 14)


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


def guarded_u8(*shape):
    n = 1
    for s in shape:
        n *= s
    buf, v = guarded(n)
    v.fill_(0xEE)
    return buf, v.view(*shape)


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    view = lambda t: t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else t.dtype)
    assert torch.equal(view(a), view(b)), f"{what}: bits differ"


def mask_inputs(Ts, chans, seed=0):
    """Per slot an eval mask [B, T, channels] (the kernel reads [:, :, 0]: stride = channels) and an attention mask with right padding.
    Slot 0: bin 3 masked in every sample (a dead bin), bin 1 in samples 1, 2 only, bin 2 in sample 0 only."""
    evals = [(torch.rand(B, T, c, generator=gen(seed + j), device="cuda") > 0.5).long() for j, (T, c) in enumerate(zip(Ts, chans))]
    if Ts[0] > 3:
        evals[0][:, 3, 0] = 1
        evals[0][:, 1, 0] = torch.tensor([0, 1, 1], device="cuda")
        evals[0][:, 2, 0] = torch.tensor([1, 0, 0], device="cuda")
    attns = []
    for j, T in enumerate(Ts):
        a = torch.ones(B, T, dtype=torch.int64, device="cuda")
        if T > 4:
            a[j % B, T - 2:] = 0                        # two padded bins on sample j of slot j (sample 0 included)
        attns.append(a)
    return evals, attns


def run_mask_prep_rows(ops, Ts, evals, attns, chans):
    Ln, M = sum(Ts), len(Ts)
    bufs = [guarded_u8(*s) for s in ((B, Ln), (B, Ln), (B, Ln), (Ln,), (Ln,))]
    cbuf, cv = guarded(8 * M)
    count = cv.view(torch.int64)
    count.fill_(-7)
    ops.mask_prep_rows(B, Ts, evals, chans, attns, chans, *[v for _, v in bufs], count)
    torch.cuda.synchronize()
    for buf, v in bufs + [(cbuf, cv)]:
        assert bool((buf[v.numel():] == SENT).all()), "mask_prep_rows wrote behind an output"
    return dict(zip(("tokmask", "keypad", "keep", "keep_any", "mod_id"), (v for _, v in bufs)), count=count)


# ------------------------------------------------------------------------------------------------- mask preparation
@pytest.mark.parametrize("Ts", [TS, (8, 8), (1, 7)])
def test_mask_prep_rows(ops, Ts):
    chans = [12, 2, 4][:len(Ts)]
    evals, attns = mask_inputs(Ts, chans, seed=3)
    if len(set(Ts)) == 1:
        attns = [attns[1]] * len(Ts)                     # the uniform form: one attention mask for every slot
    out = run_mask_prep_rows(ops, Ts, evals, attns, chans)
    ref = P.mask_products([e[:, :, 0] for e in evals], attns, chans)
    for k in ("tokmask", "keypad", "keep", "keep_any", "mod_id", "count"):
        E.check_exact(out[k], ref[k], f"mask_prep_rows {Ts}: {k}")
    if Ts[0] > 3:
        assert int(out["keep_any"][3]) == 0 and not torch.equal(out["keep"][0], out["keep"][1]), "the inputs discriminate"
        assert not torch.equal(out["keep"], P.mask_products([e[:, :, 0] for e in evals], attns, chans, row0=True)["keep"])
    # the shared outputs against the existing entry points, bit for bit; their keep0 is row 0 of keep
    Ln, M = sum(Ts), len(Ts)
    old = [torch.full(s, 0xEE, dtype=torch.uint8, device="cuda") for s in ((B, Ln), (B, Ln), (Ln,), (Ln,))]
    count = torch.full((M,), -7, dtype=torch.int64, device="cuda")
    ops.mask_prep_seg(B, Ts, evals, chans, attns, chans, *old, count)
    forms = [("mask_prep_seg", old + [count])]
    if len(set(Ts)) == 1:
        uni = [torch.full(s, 0xEE, dtype=torch.uint8, device="cuda") for s in ((B, Ln), (B, Ln), (Ln,), (Ln,))]
        c2 = torch.full((M,), -7, dtype=torch.int64, device="cuda")
        ops.mask_prep(B, Ts[0], evals, chans, attns[0], chans, *uni, c2)
        forms.append(("mask_prep", uni + [c2]))
    for name, (tokmask, keypad, keep0, mod_id, cnt) in forms:
        for k, v in (("tokmask", tokmask), ("keypad", keypad), ("mod_id", mod_id), ("count", cnt)):
            E.check_exact(out[k], v, f"mask_prep_rows {Ts} vs {name}: {k}")
        E.check_exact(out["keep"][0], keep0, f"mask_prep_rows {Ts} vs {name}: row 0 of keep is keep0")
    # deterministic: a second call gives the same bytes
    again = run_mask_prep_rows(ops, Ts, evals, attns, chans)
    assert all(torch.equal(out[k], again[k]) for k in out)


# ------------------------------------------------------------------------------------------------- the stitch pair
def stitch_inputs(Ts, dtype, seed=0):
    toks = [rnd(B * T, H, seed=seed + 10 + j, dtype=dtype) for j, T in enumerate(Ts)]
    rows = [rnd(H, seed=seed + 20 + j) for j in range(len(Ts))]
    poss = [rnd(MAX_F, H, seed=seed + 30 + j) for j in range(len(Ts))]
    tss = []
    for j, T in enumerate(Ts):                          # repeats inside a slot, another pattern per slot, one stamp out of range
        ts = (torch.arange(T, device="cuda")[None, :] * (j + 1) + torch.arange(B, device="cuda")[:, None] * 3 + j) % (MAX_F - 2)
        ts[B - 1, T - 1] = MAX_F + 5 if j % 2 else -3
        tss.append(ts.contiguous())
    return toks, rows, poss, tss


def dropout_of(ops, n, dtype, p=0.2, site=5):
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 11)
    drop = ops.dropout(state, site, p)
    pattern = torch.empty(n, H, dtype=dtype, device="cuda")
    ops.dropout_apply(torch.ones(n, H, dtype=dtype, device="cuda"), pattern, n, H, drop)
    return drop, pattern != 0, state


def sample_keep(Ln, seed=50):
    """keep u8 [B, Ln]: random rows that differ between samples; position 3 masked in every sample, position 1 in samples 1, 2 only."""
    keep = (torch.rand(B, Ln, generator=gen(seed), device="cuda") > 0.35).to(torch.uint8)
    keep[:, 3] = 0
    keep[:, 1] = torch.tensor([1, 0, 0], dtype=torch.uint8, device="cuda")
    keep[:, 0] = 1
    assert not torch.equal(keep[0], keep[1]) and not torch.equal(keep[0], keep[2])
    return keep


def check_stitch_bwd(what, outs, priors, r, with_pos, with_extra, with_drop, acc_mod, acc_pos):
    """(d_tok, d_mod, d_pos) of one stitch backward over (prior_mod, prior_pos) against the reference dict r, at edge_refs' bounds:
    the body tests/test_mod_segments_kernels_gpu.py holds the _seg entry points to."""
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
def test_shared_row_is_the_seg_entry_points(ops, dtype, with_pos):
    """keep_ld = 0, rec = NULL: every output of the pair has the bits of mmfm_stitch_*_seg, slot by slot, dropout on and off."""
    Ln = sum(TS)
    toks, rows, poss, tss = stitch_inputs(TS, dtype)
    keep0 = (torch.rand(Ln, generator=gen(50), device="cuda") > 0.3).to(torch.uint8)
    dx, dextra = rnd(B, Ln, H, seed=40, dtype=dtype), rnd(B, Ln, H, seed=41, dtype=dtype)
    code = ops.dt(dx)
    xs, es = ([nan(B, Ln, H, dtype=dtype) for _ in range(2)] for _ in range(2))
    for j, T in enumerate(TS):
        pos, ts = (poss[j], tss[j]) if with_pos else (None, None)
        ops.stitch_fwd_seg(toks[j], rows[j], pos, ts, keep0, xs[0], es[0], B, T, Ln, OFF[j], H, MAX_F)
        ops.stitch_fwd_rows(toks[j], rows[j], pos, ts, keep0, 0, None, xs[1], es[1], B, T, Ln, OFF[j], H, MAX_F)
        drop, _, _state = dropout_of(ops, B * T, dtype)
        nbytes = lib().mmfm_stitch_bwd_seg_workspace(code, B, T, Ln, OFF[j], H, MAX_F)
        for with_extra, with_drop, acc in ((True, True, True), (False, False, False)):
            outs = []
            for rows_form in (False, True):
                d_tok, d_mod, d_pos = nan(B * T, H, dtype=dtype), rnd(H, seed=50), rnd(MAX_F, H, seed=51)
                buf, ws = guarded(nbytes)
                head = (dx, dextra if with_extra else None, ts, keep0)
                tail = (drop if with_drop else None, d_tok, d_mod, d_pos if with_pos else None, acc, acc, B, T, Ln, OFF[j], H, MAX_F, ws)
                if rows_form:
                    ops.stitch_bwd_rows(*head, 0, None, *tail)
                else:
                    ops.stitch_bwd_seg(*head, *tail)
                torch.cuda.synchronize()
                assert bool((buf[nbytes:] == SENT).all()), "wrote behind the workspace"
                outs.append((d_tok, d_mod, d_pos))
            for name, a, b in zip(("d_tok", "d_mod", "d_pos"), outs[1], outs[0]):
                same_bits(a, b, f"stitch_bwd_rows keep_ld=0 slot {j} extra={with_extra} drop={with_drop}: {name}")
    same_bits(xs[1], xs[0], "stitch_fwd_rows keep_ld=0: x")
    same_bits(es[1], es[0], "stitch_fwd_rows keep_ld=0: emb")


def live_record(ops, keep_any, T, M):
    from multi_modal_foundation_model_amd import _lib as L
    rec = torch.full((M, L.live_rec_ints(T)), -9, dtype=torch.int32, device="cuda")
    ops.live_bins(keep_any, T, M, rec)
    torch.cuda.synchronize()
    return rec


def test_shared_row_with_a_record_is_the_live_entry_points(ops):
    """keep_ld = 0, rec given, off = m * T (bf16): the bits of mmfm_stitch_*_live - compact tok rows in, compact d_tok rows out, the rows
    behind B * T_live untouched."""
    T, M, dtype = 8, 2, BF16
    Ln = M * T
    toks, rows, poss, tss = stitch_inputs((T,) * M, dtype)
    ts = tss[1]
    keep0 = torch.tensor([1, 0, 1, 0, 0, 1, 1, 1] + [0, 1, 1, 1, 1, 1, 1, 0], dtype=torch.uint8, device="cuda")
    rec = live_record(ops, keep0, T, M)
    dx, dextra = rnd(B, Ln, H, seed=40, dtype=dtype), rnd(B, Ln, H, seed=41, dtype=dtype)
    nbytes = lib().mmfm_stitch_bwd_workspace(ops.dt(dx), B, T, Ln, H, MAX_F)
    xs, es = ([nan(B, Ln, H, dtype=dtype) for _ in range(2)] for _ in range(2))
    for m in range(M):
        tl = int(rec[m, 0])
        assert 0 < tl < T
        ops.stitch_fwd_live(toks[m], rows[m], poss[m], ts, keep0, rec[m], xs[0], es[0], B, T, Ln, m, H, MAX_F)
        ops.stitch_fwd_rows(toks[m], rows[m], poss[m], ts, keep0, 0, rec[m], xs[1], es[1], B, T, Ln, m * T, H, MAX_F)
        drop, _, _state = dropout_of(ops, B * T, dtype)
        for with_drop in (True, False):
            outs = []
            for rows_form in (False, True):
                d_tok, d_mod, d_pos = nan(B * T, H, dtype=dtype), rnd(H, seed=50), rnd(MAX_F, H, seed=51)
                buf, ws = guarded(nbytes)
                tail = (drop if with_drop else None, d_tok, d_mod, d_pos, True, False, B, T, Ln)
                if rows_form:
                    ops.stitch_bwd_rows(dx, dextra, ts, keep0, 0, rec[m], *tail, m * T, H, MAX_F, ws)
                else:
                    ops.stitch_bwd_live(dx, dextra, ts, keep0, rec[m], *tail, m, H, MAX_F, ws)
                torch.cuda.synchronize()
                assert bool((buf[nbytes:] == SENT).all()), "wrote behind the workspace"
                assert bool(torch.isfinite(d_tok[:B * tl]).all()) and bool(torch.isnan(d_tok[B * tl:]).all())
                outs.append((d_tok, d_mod, d_pos))
            for name, a, b in zip(("d_tok", "d_mod", "d_pos"), outs[1], outs[0]):
                same_bits(a, b, f"stitch_bwd_rows keep_ld=0 with a record, slot {m} drop={with_drop}: {name}")
    same_bits(xs[1], xs[0], "stitch_fwd_rows keep_ld=0 with a record: x")
    same_bits(es[1], es[0], "stitch_fwd_rows keep_ld=0 with a record: emb")


@pytest.mark.parametrize("pad", [0, 5], ids=["ld=L", "ld=L+5"])
@pytest.mark.parametrize("with_pos", [True, False], ids=["table", "notable"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_per_sample_mask_vs_restatement(ops, dtype, with_pos, pad):
    """keep [B][keep_ld], keep_ld = L or L + 5 (the columns behind L hold the opposite of what a wrong stride would need): forward and
    backward of every slot against tests/per_sample_mask.py at the _seg kernels' bounds; exact zeros in d_tok at masked rows; with
    dropout on, the decisions of the _seg form: d_tok is the all-kept _seg launch's where the sample keeps the row."""
    Ln = sum(TS)
    ld = Ln + pad
    toks, rows, poss, tss = stitch_inputs(TS, dtype, seed=100)
    keep = sample_keep(Ln)
    kbuf, kv = guarded(B * ld)
    kfull = kv.view(B, ld)
    kfull[:] = 1
    kfull[:, :Ln] = keep
    if pad:
        kfull[:, Ln:] = 1 - keep[:, :pad]
    ones = torch.ones(Ln, dtype=torch.uint8, device="cuda")
    zero_pos = torch.zeros(MAX_F, H, device="cuda")
    x, emb = nan(B, Ln, H, dtype=dtype), nan(B, Ln, H, dtype=dtype)
    for j, T in enumerate(TS):
        ops.stitch_fwd_rows(toks[j], rows[j], poss[j] if with_pos else None, tss[j] if with_pos else None, kfull, ld, None, x, emb, B, T, Ln, OFF[j], H,
                            MAX_F)
        for out in (x, emb):
            assert bool(torch.isfinite(out[:, :OFF[j + 1]]).all()) and bool(torch.isnan(out[:, OFF[j + 1]:]).all()), f"slot {j} missed its slice"
    for j, T in enumerate(TS):
        xr, er, mag = P.stitch_fwd(toks[j], rows[j], poss[j] if with_pos else zero_pos, tss[j], keep, OFF[j], MAX_F)
        for name, out, ref in (("x", x, xr), ("emb", emb, er)):
            sl, what = out[:, OFF[j]:OFF[j + 1]], f"stitch_fwd_rows slot {j} {name}"
            if dtype == BF16:
                E.check_bf16(sl, ref, E.stitch_fwd_e32(mag), what)
            else:
                E.check_close(sl, ref, E.TOL_STITCH, what)
        # a masked row of x is its emb row, bit for bit
        gone = keep[:, OFF[j]:OFF[j + 1]] == 0
        same_bits(x[:, OFF[j]:OFF[j + 1]][gone], emb[:, OFF[j]:OFF[j + 1]][gone], f"slot {j}: masked rows of x")
    dx, dextra = rnd(B, Ln, H, seed=140, dtype=dtype), rnd(B, Ln, H, seed=141, dtype=dtype)
    code, p = ops.dt(dx), 0.2
    for j, T in enumerate(TS):
        n = B * T
        drop, dkeep, _state = dropout_of(ops, n, dtype, p)
        nbytes = lib().mmfm_stitch_bwd_seg_workspace(code, B, T, Ln, OFF[j], H, MAX_F)
        krow = keep[:, OFF[j]:OFF[j + 1]].reshape(n) != 0
        for with_extra, with_drop, acc_mod, acc_pos in ((True, True, True, False), (False, False, False, True)):
            what = f"stitch_bwd_rows slot {j} dextra={with_extra} drop={with_drop} acc=({acc_mod},{acc_pos})"
            extra = dextra if with_extra else None
            prior_mod, prior_pos = rnd(H, seed=150), rnd(MAX_F, H, seed=151)
            runs = []
            for _ in range(2):                          # twice: d_pos and d_mod_row must come out with the same bits
                d_tok, d_mod, d_pos = nan(n, H, dtype=dtype), prior_mod.clone(), prior_pos.clone()
                buf, ws = guarded(nbytes)
                ops.stitch_bwd_rows(dx, extra, tss[j] if with_pos else None, kfull, ld, None, drop if with_drop else None, d_tok, d_mod,
                                    d_pos if with_pos else None, acc_mod, acc_pos, B, T, Ln, OFF[j], H, MAX_F, ws)
                torch.cuda.synchronize()
                assert bool((buf[nbytes:] == SENT).all()), f"{what}: wrote behind its {nbytes}-byte workspace"
                runs.append((d_tok, d_mod, d_pos))
            same_bits(runs[0][1], runs[1][1], f"{what}: d_mod_row of two calls")
            same_bits(runs[0][2], runs[1][2], f"{what}: d_pos of two calls")
            r = P.stitch_bwd(dx, extra, tss[j], keep, dkeep if with_drop else None, p, OFF[j], MAX_F)
            check_stitch_bwd(what, runs[0], (prior_mod, prior_pos), r, with_pos, with_extra, with_drop, acc_mod, acc_pos)
            d_tok = runs[0][0]
            assert bool((d_tok[~krow].view(torch.int16 if dtype == BF16 else torch.int32) == 0).all()), f"{what}: masked rows of d_tok are +0"
            # the all-kept _seg launch: the same decisions, the same values where the sample keeps the row
            full = nan(n, H, dtype=dtype)
            ops.stitch_bwd_seg(dx, extra, tss[j] if with_pos else None, ones, drop if with_drop else None, full, prior_mod.clone(),
                               prior_pos.clone() if with_pos else None, acc_mod, acc_pos, B, T, Ln, OFF[j], H, MAX_F, guarded(nbytes)[1])
            same_bits(d_tok, torch.where(krow[:, None], full, torch.zeros_like(full)), f"{what}: d_tok vs the all-kept _seg launch")
    assert bool((kbuf[B * ld:] == SENT).all())


# ------------------------------------------------------------------------------------------------- live bins that a sample masks
def run_live(ops, keep, T, with_drop):
    """One slot of T bins (L = T), bf16, per-sample keep [Bn, T] with its record from keep_any: the compact forward and backward.
    Returns x, the reference x, d_tok (compact, NaN-prefilled), the full-row d_tok of the all-kept _seg launch and the record."""
    Bn, dtype = keep.shape[0], BF16
    keep_any = keep.any(0).to(torch.uint8)
    rec = live_record(ops, keep_any, T, 1)[0]
    tl = int(rec[0])
    lt = rec[4:4 + tl].long()
    tok_full = rnd(Bn * T, H, seed=7, dtype=dtype)
    row, pos = rnd(H, seed=8), rnd(MAX_F, H, seed=9)
    ts = (torch.arange(T, device="cuda")[None] + torch.arange(Bn, device="cuda")[:, None]) % MAX_F
    # compact tok: the live bins' rows; a live bin's row of a sample that masks it holds NaN - the forward must not read it
    tok = nan(Bn * T, H, dtype=dtype)
    comp = tok_full.view(Bn, T, H)[:, lt].clone()
    comp[keep[:, lt] == 0] = float("nan")
    tok[:Bn * tl] = comp.reshape(Bn * tl, H)
    x, emb = nan(Bn, T, H, dtype=dtype), nan(Bn, T, H, dtype=dtype)
    ops.stitch_fwd_rows(tok, row, pos, ts, keep, T, rec, x, emb, Bn, T, T, 0, H, MAX_F)
    xr = nan(Bn, T, H, dtype=dtype)
    ops.stitch_fwd_rows(tok_full, row, pos, ts, keep, T, None, xr, None, Bn, T, T, 0, H, MAX_F)
    dx = rnd(Bn, T, H, seed=10, dtype=dtype)
    drop, _, _state = dropout_of(ops, Bn * T, dtype)
    nbytes = lib().mmfm_stitch_bwd_seg_workspace(ops.dt(dx), Bn, T, T, 0, H, MAX_F)
    d_tok, full = nan(Bn * T, H, dtype=dtype), nan(Bn * T, H, dtype=dtype)
    mods = [torch.zeros(H, device="cuda") for _ in range(2)]
    poss = [torch.zeros(MAX_F, H, device="cuda") for _ in range(2)]
    buf, ws = guarded(nbytes)
    ops.stitch_bwd_rows(dx, None, ts, keep, T, rec, drop if with_drop else None, d_tok, mods[0], poss[0], False, False, Bn, T, T, 0, H, MAX_F, ws)
    ops.stitch_bwd_seg(dx, None, ts, torch.ones(T, dtype=torch.uint8, device="cuda"), drop if with_drop else None, full, mods[1], poss[1], False,
                       False, Bn, T, T, 0, H, MAX_F, guarded(nbytes)[1])
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == SENT).all())
    same_bits(mods[0], mods[1], "d_mod_row does not depend on the keep mask or the record")
    same_bits(poss[0], poss[1], "d_pos does not depend on the keep mask or the record")
    return x, xr, d_tok, full, rec


@pytest.mark.parametrize("with_drop", [False, True], ids=["nodrop", "drop"])
def test_live_bin_masked_in_one_sample_smallest_case(ops, with_drop):
    """B = 2, T = 2, bin 0 masked in sample 1 only: both bins are live (keep_any), so sample 1's compact row of bin 0 exists.  The forward
    ignores it (it holds NaN); the backward writes zeros to it - the weight-gradient product over the compact rows reads it."""
    keep = torch.tensor([[1, 1], [0, 1]], dtype=torch.uint8, device="cuda")
    x, xr, d_tok, full, rec = run_live(ops, keep, 2, with_drop)
    assert rec[:4].tolist() == [2, 0, 0, 0]
    same_bits(x, xr, "x under the record vs the full-row launch")
    assert bool(torch.isfinite(d_tok).all()), "a compact d_tok row was left unwritten"
    assert bool((d_tok[2].view(torch.int16) == 0).all()), "the masked sample's compact row of a live bin is +0"
    same_bits(d_tok[[0, 1, 3]], full[[0, 1, 3]], "the kept rows: the values and dropout decisions of the full-row launch")


@pytest.mark.parametrize("with_drop", [False, True], ids=["nodrop", "drop"])
def test_live_bins_dead_in_all_and_masked_in_some(ops, with_drop):
    """B = 3, T = 8: bin 3 dead (masked in every sample), bins 1 and 6 masked in some samples, bin 5 in sample 0 only.  Compact rows:
    B * 7; those of masked (sample, bin) pairs are zeros, the others carry the full-row launch's values at the ORIGINAL row's dropout
    counter, and nothing is written behind B * T_live."""
    T = 8
    keep = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    keep[:, 3] = 0
    keep[1:, 1] = 0
    keep[2, 6] = 0
    keep[0, 5] = 0
    x, xr, d_tok, full, rec = run_live(ops, keep, T, with_drop)
    tl = int(rec[0])
    assert tl == 7 and rec[4:4 + tl].tolist() == [0, 1, 2, 4, 5, 6, 7] and int(rec[4 + T + 3]) == -1
    same_bits(x, xr, "x under the record vs the full-row launch")
    assert bool(torch.isfinite(d_tok[:B * tl]).all()) and bool(torch.isnan(d_tok[B * tl:]).all())
    lt = rec[4:4 + tl].long()
    want = full.view(B, T, H)[:, lt].clone()
    want[keep[:, lt] == 0] = 0
    same_bits(d_tok[:B * tl], want.reshape(B * tl, H), "compact d_tok")
    assert int((keep[:, lt] == 0).sum()) == 4
