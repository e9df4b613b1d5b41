"""The masked losses under a row mask x channel mask (mmfm_masked_loss_chan_fwd / _bwd, padded neurons) through the C ABI, fp32 and
bf16: against the fp64 references of tests/loss_elem_refs.py on the expanded product mask at tests/loss_refs.py's derived bounds, and
bit for bit against the row-mask entry points (all-ones channel mask) and the per-element entry points (the expanded product).
Runs on the MI355X only."""
import pytest
import torch

import edge_refs as E
import loss_elem_refs as X

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
# N around the 64 lanes of a row's wavefront; B * T = 15 rows leave the last 4-row block ragged; 4100 rows wrap the 1024-block grid;
# N = 2048 is the widest row whose channel bits a lane gathers into one register, 2049 the first that reads its bytes inside the walk
SHAPES = [(3, 5, 1), (3, 5, 2), (3, 5, 63), (3, 5, 64), (3, 5, 65), (3, 5, 668), (41, 100, 5), (2, 3, 2048), (2, 3, 2049)]
CHAN = ("ones", "right", "left", "third", "shared")
ROWS = ("BT1", "none", "sample0", "shared")
GUARD, SENT = 4096, 0xA5


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def ibits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def guarded(nbytes):
    buf = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[:nbytes]


def chan_mask(name, B, N):
    """u8 [B, N] (or [1, N] for "shared") on the CPU.  right / left: sample b has (N, ceil(N/2), 0)[b % 3] real channels at the low /
    high end, so there is a sample with every channel and one with none."""
    counts = [(N, (N + 1) // 2, 0)[b % 3] for b in range(B)]
    v = torch.zeros(1 if name == "shared" else B, N, dtype=torch.uint8)
    if name == "ones":
        v[:] = 1
    elif name == "right":
        for b, n in enumerate(counts):
            v[b, :n] = 1
    elif name == "left":
        for b, n in enumerate(counts):
            v[b, N - n:] = 1
    elif name == "third":
        v[:, ::3] = 1
    else:
        v[0, :(N + 1) // 2] = 1
    return v


def row_mask(name, B, T, N):
    """(u8 mask on the CPU, mask_ld): [B, T] with mask_ld = T, or one [T] mask for all samples with mask_ld = 0."""
    if name == "shared":
        return X.mask("1T1", B, T, N).reshape(T).contiguous(), 0
    m = X.mask("BT1", B, T, N)[:, :, 0].contiguous()
    if name == "none":
        m.zero_()
    elif name == "sample0":
        m[0] = 0
    return m, T


def product(rm, v, B, T, N):
    """The expanded [B, T, N] u8 product of a row mask and a channel mask."""
    return (rm.reshape(-1, T).expand(B, T)[:, :, None] * v.expand(B, N)[:, None, :]).contiguous()


def run_fwd(ops, spec, pred, tgt, rm, ld, T, v):
    R, N = pred.shape
    nbytes = ops.masked_loss_chan_workspace(R, N)
    out, cnt = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
    buf, ws = guarded(nbytes)
    ops.masked_loss_chan_fwd(*spec, pred, tgt, rm, ld, T, R, N, v, out, cnt, ws)
    assert bool((buf[nbytes:] == SENT).all()), f"wrote behind its {nbytes}-byte workspace"
    return out, cnt


def run_bwd(ops, spec, pred, tgt, rm, ld, T, v, gout, inv_n):
    R, N = pred.shape
    dpred = torch.full((R, N), 7.0, dtype=pred.dtype, device="cuda")
    ops.masked_loss_chan_bwd(*spec, pred, tgt, rm, ld, T, R, N, v, gout, inv_n, dpred)
    return dpred


def elem_fwd(ops, spec, pred, tgt, full, B, T, N):
    out, cnt = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ops.masked_loss_elem_fwd(*spec, pred, tgt, full, B, T, N, out, cnt, guarded(ops.masked_loss_elem_workspace(B, T, N))[1])
    return out, cnt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,N", SHAPES)
@pytest.mark.parametrize("case", list(X.CASES))
def test_chan_loss_against_fp64_and_the_element_form(ops, case, B, T, N, dtype):
    """Every (channel mask, row mask) pair: the sum, the exact count and dpred against fp64 on the expanded product, the same bits on a
    second call, and the bits of mmfm_masked_loss_elem_* on the expanded product (bit-identity B)."""
    spec = X.CASES[case]
    kind, param, flags = spec
    pred, tgt = (t.cuda() for t in X.inputs(case, B * T, N, dtype))
    gout = torch.tensor([0.5], device="cuda")
    for cname in CHAN:
        v = chan_mask(cname, B, N).cuda()
        for rname in ROWS:
            what = f"chan loss {case} [{B}x{T}x{N}] chan {cname} rows {rname}"
            rm, ld = row_mask(rname, B, T, N)
            rm = rm.cuda()
            full = product(rm, v, B, T, N)
            out, cnt = run_fwd(ops, spec, pred, tgt, rm, ld, T, v)
            s, n, sabs, terr = X.elem_loss_sum(kind, pred, tgt, full, param, flags)
            assert cnt.item() == n == int(full.sum().item()), f"{what}: count {cnt.item()} != {n}"
            E.check_sum(out, s.reshape(1), n, sabs, f"{what} sum", term_err=terr)
            out2, cnt2 = run_fwd(ops, spec, pred, tgt, rm, ld, T, v)
            E.check_exact(ibits(out2), ibits(out), f"{what}: a second call gives other bits")
            assert cnt2.item() == n
            inv_n = torch.tensor([1.0 / (n + 7)], device="cuda")
            dpred = run_bwd(ops, spec, pred, tgt, rm, ld, T, v, gout, inv_n)
            E.check_elem(dpred, X.elem_loss_bwd(kind, pred, tgt, full, gout, inv_n, param), E.TOL_DPRED, f"{what} dpred")
            assert bool((dpred[(full == 0).reshape(B * T, N)] == 0).all()), f"{what}: dpred must be exactly zero where the product is 0"
            E.check_exact(ibits(run_bwd(ops, spec, pred, tgt, rm, ld, T, v, gout, inv_n)), ibits(dpred), f"{what}: a second backward gives other bits")
            eout, ecnt = elem_fwd(ops, spec, pred, tgt, full, B, T, N)
            edpred = torch.full((B * T, N), 7.0, dtype=dtype, device="cuda")
            ops.masked_loss_elem_bwd(*spec, pred, tgt, full, B, T, N, gout, inv_n, edpred)
            E.check_exact(ibits(out), ibits(eout), f"{what}: sum bits differ from the element form's")
            assert cnt.item() == ecnt.item()
            E.check_exact(ibits(dpred), ibits(edpred), f"{what}: dpred bits differ from the element form's")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,N", SHAPES)
@pytest.mark.parametrize("case", list(X.CASES))
def test_all_ones_channel_mask_gives_the_row_mask_kernels_bits(ops, case, B, T, N, dtype):
    """Bit-identity A: an all-ones channel mask ([B, N] and [1, N]) gives mmfm_masked_loss_kind_*'s bits under the same row mask, and
    the count is masked rows x N."""
    from multi_modal_foundation_model_amd import _lib as Lb
    spec = X.CASES[case]
    pred, tgt = (t.cuda() for t in X.inputs(case, B * T, N, dtype))
    gout, inv_n = torch.tensor([0.5], device="cuda"), torch.tensor([1.0 / 1234.0], device="cuda")
    nbytes = Lb.lib().mmfm_masked_loss_workspace(B * T, N)
    for rname in ROWS:
        rm, ld = row_mask(rname, B, T, N)
        rm = rm.cuda()
        rows = rm.reshape(-1, T).expand(B, T).contiguous()                # the row form takes mask_ld >= T only
        ref, dref = torch.full((1,), float("nan"), device="cuda"), torch.full((B * T, N), 7.0, dtype=dtype, device="cuda")
        ops.masked_loss_kind_fwd(*spec, pred, tgt, rows, T, T, B * T, N, ref, guarded(nbytes)[1])
        ops.masked_loss_kind_bwd(*spec, pred, tgt, rows, T, T, B * T, N, gout, inv_n, dref)
        for v in (torch.ones(B, N, dtype=torch.uint8, device="cuda"), torch.ones(1, N, dtype=torch.uint8, device="cuda")):
            out, cnt = run_fwd(ops, spec, pred, tgt, rm, ld, T, v)
            dpred = run_bwd(ops, spec, pred, tgt, rm, ld, T, v, gout, inv_n)
            E.check_exact(ibits(out), ibits(ref), f"{case} rows {rname}: sum bits")
            E.check_exact(ibits(dpred), ibits(dref), f"{case} rows {rname}: dpred bits")
            assert cnt.item() == int(rows.sum().item()) * N


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["poisson_log", "mse", "poisson_rate_full", "huber", "bce"])
def test_nothing_set_and_poisoned_unset_elements(ops, case, dtype):
    B, T, N = 3, 5, 65
    spec = X.CASES[case]
    pred, tgt = (t.cuda() for t in X.inputs(case, B * T, N, dtype))
    gout = torch.tensor([0.5], device="cuda")
    # nothing set - no row, or no channel: sum 0, count 0, dpred exactly 0 under a finite inv_n and NaN under inf
    bt1, ld = row_mask("BT1", B, T, N)
    for rm, v in ((torch.zeros(B, T, dtype=torch.uint8), chan_mask("ones", B, N)), (bt1, torch.zeros(B, N, dtype=torch.uint8)),
                  (bt1, torch.zeros(1, N, dtype=torch.uint8))):
        rm, v = rm.cuda(), v.cuda()
        out, cnt = run_fwd(ops, spec, pred, tgt, rm, T, T, v)
        assert out.item() == 0.0 and cnt.item() == 0
        dpred = run_bwd(ops, spec, pred, tgt, rm, T, T, v, gout, torch.tensor([0.25], device="cuda"))
        assert bool((dpred == 0).all())
        dpred = run_bwd(ops, spec, pred, tgt, rm, T, T, v, gout, torch.tensor([float("inf")], device="cuda"))
        assert bool(torch.isnan(dpred).all()), "nothing set and inv_n = inf: dpred must be NaN everywhere"
    # NaN / Inf / -1 on unmasked rows and under cleared channels reach neither the sum, the count nor dpred
    for cname in CHAN[1:]:
        v = chan_mask(cname, B, N).cuda()
        for rname in ("BT1", "sample0", "shared"):
            rm, ld = row_mask(rname, B, T, N)
            rm = rm.cuda()
            off = (product(rm, v, B, T, N) == 0).reshape(B * T, N)
            assert bool(off.any()) and not bool(off.all())
            inv_n = torch.tensor([1.0 / 99.0], device="cuda")
            clean, cnt = run_fwd(ops, spec, pred, tgt, rm, ld, T, v)
            dclean = run_bwd(ops, spec, pred, tgt, rm, ld, T, v, gout, inv_n)
            assert bool(torch.isfinite(clean).all())
            bad_p, bad_t = pred.clone(), tgt.clone()
            idx = torch.nonzero(off.reshape(-1)).reshape(-1)
            bad_p.view(-1)[idx[0::4]] = float("nan")
            bad_p.view(-1)[idx[1::4]] = float("inf")
            bad_t.view(-1)[idx[2::4]] = float("nan")
            bad_t.view(-1)[idx[0::4]] = float("-inf")
            bad_p.view(-1)[idx[3::4]] = -1.0
            bad_t.view(-1)[idx[3::4]] = -1.0
            out, cnt2 = run_fwd(ops, spec, bad_p, bad_t, rm, ld, T, v)
            what = f"{case} chan {cname} rows {rname}"
            E.check_exact(ibits(out), ibits(clean), f"{what}: a NaN / Inf / -1 outside the product reached the sum")
            assert cnt2.item() == cnt.item() and bool(torch.isfinite(out).all())
            E.check_exact(ibits(run_bwd(ops, spec, bad_p, bad_t, rm, ld, T, v, gout, inv_n)), ibits(dclean),
                          f"{what}: a NaN / Inf / -1 outside the product reached dpred")


def test_argument_checks(ops):
    """Every refused call returns -1 with an error text and leaves its outputs untouched."""
    from multi_modal_foundation_model_amd import _lib as Lb
    lib = Lb.lib()
    B, T, N = 2, 3, 4
    R = B * T
    pred, tgt = torch.zeros(R, N, device="cuda"), torch.zeros(R, N, device="cuda")
    rm, v = torch.ones(B, T, dtype=torch.uint8, device="cuda"), torch.ones(B, N, dtype=torch.uint8, device="cuda")
    out, cnt = torch.full((1,), 3.0, device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
    gout, inv_n = torch.ones(1, device="cuda"), torch.ones(1, device="cuda")
    dpred = torch.full((R, N), 7.0, device="cuda")
    nbytes = ops.masked_loss_chan_workspace(R, N)
    assert nbytes == lib.mmfm_masked_loss_chan_workspace(R, N) >= 12
    ws = torch.zeros(nbytes // 4 + 2, device="cuda")
    P = lambda t: t.data_ptr()
    good = dict(dtype=0, kind=1, param=0.0, flags=0, pred=P(pred), target=P(tgt), rowmask=P(rm), mask_ld=T, T=T, R=R, N=N, chanmask=P(v), chan_ld=N)
    bad = [("null pointer", dict(pred=None)), ("null pointer", dict(target=None)), ("null pointer", dict(rowmask=None)),
           ("null pointer", dict(chanmask=None)), ("bad dtype", dict(dtype=2)), ("bad kind", dict(kind=7)), ("bad kind", dict(kind=-1)),
           ("bad kind", dict(param=-0.5)), ("bad kind", dict(flags=1)), ("bad kind", dict(kind=0, flags=2)),
           ("bad arguments", dict(R=R + 1)), ("bad arguments", dict(R=0)), ("bad arguments", dict(N=0)), ("bad arguments", dict(T=0)),
           ("bad arguments", dict(mask_ld=-1)), ("bad arguments", dict(mask_ld=T - 1)), ("bad arguments", dict(chan_ld=-1)),
           ("bad arguments", dict(chan_ld=N - 1))]
    order = ("dtype", "kind", "param", "flags", "pred", "target", "rowmask", "mask_ld", "T", "R", "N", "chanmask", "chan_ld")
    for text, change in bad:
        a = [dict(good, **change)[k] for k in order]
        rc = lib.mmfm_masked_loss_chan_fwd(*a, P(out), P(cnt), P(ws), ws.numel() * 4, None)
        assert rc == -1 and text in lib.mmfm_last_error().decode(), f"fwd {change}: {rc} {lib.mmfm_last_error()}"
        rc = lib.mmfm_masked_loss_chan_bwd(*a, P(gout), P(inv_n), P(dpred), None)
        assert rc == -1 and text in lib.mmfm_last_error().decode(), f"bwd {change}: {rc} {lib.mmfm_last_error()}"
    a = [good[k] for k in order]
    for tail, text in (((None, P(cnt), P(ws), ws.numel() * 4), "null pointer"), ((P(out), None, P(ws), ws.numel() * 4), "null pointer"),
                       ((P(out), P(cnt), None, ws.numel() * 4), "workspace"), ((P(out), P(cnt), P(ws), nbytes - 1), "workspace"),
                       ((P(out), P(cnt), P(ws) + 4, ws.numel() * 4), "workspace")):
        assert lib.mmfm_masked_loss_chan_fwd(*a, *tail, None) == -1 and text in lib.mmfm_last_error().decode(), tail
    for tail in ((None, P(inv_n), P(dpred)), (P(gout), None, P(dpred)), (P(gout), P(inv_n), None)):
        assert lib.mmfm_masked_loss_chan_bwd(*a, *tail, None) == -1 and "null pointer" in lib.mmfm_last_error().decode(), tail
    torch.cuda.synchronize()
    assert out.item() == 3.0 and cnt.item() == -7 and bool((dpred == 7.0).all()), "a refused call wrote its outputs"
    with pytest.raises(ValueError, match="channel mask"):
        ops.masked_loss_chan_fwd(1, 0.0, 0, pred, tgt, rm, T, T, R, N, v[:, :3], out, cnt, ws)
    with pytest.raises(ValueError, match="channel mask"):
        ops.masked_loss_chan_bwd(1, 0.0, 0, pred, tgt, rm, T, T, R, N, v.bool(), gout, inv_n, dpred)
    # mask_ld = 0 and chan_ld = 0 together are a legal call
    assert lib.mmfm_masked_loss_chan_fwd(*[dict(good, mask_ld=0, chan_ld=0)[k] for k in order], P(out), P(cnt), P(ws), ws.numel() * 4, None) == 0
    assert cnt.item() == R * N
