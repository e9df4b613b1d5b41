"""The masked losses under a per-element mask (mmfm_masked_loss_elem_fwd / _bwd) and the masked staging copy (mmfm_stage_masked)
through the C ABI, fp32 and bf16, against the fp64 references of tests/loss_elem_refs.py at tests/loss_refs.py's derived bounds, and
bit for bit against the row-mask entry points where the two must agree.  Runs on the MI355X only."""
import pytest
import torch

import edge_refs as E
import loss_elem_refs as X

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
# N around the 64 lanes of a row's wavefront; B * T = 15 rows leave the last 4-row block ragged.  The last shape has 4100 rows: past the
# 1024 blocks x 4 rows of the grid, so the grid-stride loop wraps
SHAPES = [(3, 5, 1), (3, 5, 2), (3, 5, 63), (3, 5, 64), (3, 5, 65), (3, 5, 668), (41, 100, 5)]
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


def run_fwd(ops, spec, pred, tgt, m, B, T, N):
    nbytes = ops.masked_loss_elem_workspace(B, T, N)
    out, cnt = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
    buf, ws = guarded(nbytes)
    ops.masked_loss_elem_fwd(*spec, pred, tgt, m, B, T, N, out, cnt, ws)
    assert bool((buf[nbytes:] == SENT).all()), f"wrote behind its {nbytes}-byte workspace"
    return out, cnt


def run_bwd(ops, spec, pred, tgt, m, B, T, N, gout, inv_n):
    dpred = torch.full((B * T, N), 7.0, dtype=pred.dtype, device="cuda")
    ops.masked_loss_elem_bwd(*spec, pred, tgt, m, B, T, N, gout, inv_n, dpred)
    return dpred


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,N", SHAPES)
@pytest.mark.parametrize("case", list(X.CASES))
def test_elem_loss_against_fp64(ops, case, B, T, N, dtype):
    spec = X.CASES[case]
    kind, param, flags = spec
    pred, tgt = (t.cuda() for t in X.inputs(case, B * T, N, dtype))
    gout = torch.tensor([0.5], device="cuda")
    for pattern in X.PATTERNS:
        what = f"elem loss {case} [{B}x{T}x{N}] {pattern}"
        m = X.mask(pattern, B, T, N).cuda()
        full = X.expand(m, B, T, N)
        out, cnt = run_fwd(ops, spec, pred, tgt, m, B, T, N)
        s, n, sabs, terr = X.elem_loss_sum(kind, pred, tgt, full, param, flags)
        assert cnt.item() == n == int(full.sum().item()), f"{what}: count {cnt.item()} != {n}"
        E.check_sum(out, s.reshape(1), n, sabs, f"{what} sum", term_err=terr)
        out2, cnt2 = run_fwd(ops, spec, pred, tgt, m, B, T, N)
        E.check_exact(ibits(out2), ibits(out), f"{what}: a second call gives other bits")
        assert cnt2.item() == n
        inv_n = torch.tensor([1.0 / (n + 7)], device="cuda")
        dpred = run_bwd(ops, spec, pred, tgt, m, B, T, N, gout, inv_n)
        E.check_elem(dpred, X.elem_loss_bwd(kind, pred, tgt, full, gout, inv_n, param), E.TOL_DPRED, f"{what} dpred")
        assert bool((dpred[(full == 0).reshape(B * T, N)] == 0).all()), f"{what}: dpred must be exactly zero on unset elements"
        E.check_exact(ibits(run_bwd(ops, spec, pred, tgt, m, B, T, N, gout, inv_n)), ibits(dpred), f"{what}: a second backward gives other bits")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,N", SHAPES)
@pytest.mark.parametrize("case", list(X.CASES))
def test_elem_loss_bits_of_the_row_mask_kernels(ops, case, B, T, N, dtype):
    """An all-ones mask (in every compact form) gives mmfm_masked_loss_kind_*'s bits with every row masked, a [B,T,1] mask their bits
    with that row mask."""
    from multi_modal_foundation_model_amd import _lib as Lb
    spec = X.CASES[case]
    pred, tgt = (t.cuda() for t in X.inputs(case, B * T, N, dtype))
    gout, inv_n = torch.tensor([0.5], device="cuda"), torch.tensor([1.0 / 1234.0], device="cuda")
    ones = lambda *shape: torch.ones(shape, dtype=torch.uint8, device="cuda")
    bt1 = X.mask("BT1", B, T, N).cuda()
    masks = [("ones BTN", ones(B, T, N), ones(B, T)), ("ones 111", ones(1, 1, 1), ones(B, T)), ("ones B1N", ones(B, 1, N), ones(B, T)),
             ("BT1", bt1, bt1[:, :, 0].contiguous())]
    nbytes = Lb.lib().mmfm_masked_loss_workspace(B * T, N)
    for name, m, rowmask in masks:
        out, cnt = run_fwd(ops, spec, pred, tgt, m, B, T, N)
        dpred = run_bwd(ops, spec, pred, tgt, m, B, T, N, gout, inv_n)
        ref, dref = torch.full((1,), float("nan"), device="cuda"), torch.full((B * T, N), 7.0, dtype=dtype, device="cuda")
        ops.masked_loss_kind_fwd(*spec, pred, tgt, rowmask, T, T, B * T, N, ref, guarded(nbytes)[1])
        ops.masked_loss_kind_bwd(*spec, pred, tgt, rowmask, T, T, B * T, N, gout, inv_n, dref)
        E.check_exact(ibits(out), ibits(ref), f"{case} {name}: sum bits")
        E.check_exact(ibits(dpred), ibits(dref), f"{case} {name}: dpred bits")
        assert cnt.item() == int(rowmask.sum().item()) * N


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["poisson_log", "mse", "poisson_rate_full", "huber", "bce"])
def test_all_zero_mask_and_unmasked_nonfinite(ops, case, dtype):
    B, T, N = 3, 5, 65
    spec = X.CASES[case]
    pred, tgt = (t.cuda() for t in X.inputs(case, B * T, N, dtype))
    gout = torch.tensor([0.5], device="cuda")
    # nothing set: sum 0, count 0, dpred exactly 0 under a finite inv_n and NaN under inf
    for zero in (torch.zeros(B, T, N, dtype=torch.uint8, device="cuda"), torch.zeros(1, 1, N, dtype=torch.uint8, device="cuda")):
        out, cnt = run_fwd(ops, spec, pred, tgt, zero, B, T, N)
        assert out.item() == 0.0 and cnt.item() == 0
        dpred = run_bwd(ops, spec, pred, tgt, zero, B, T, N, gout, torch.tensor([0.25], device="cuda"))
        assert bool((dpred == 0).all())
        dpred = run_bwd(ops, spec, pred, tgt, zero, B, T, N, gout, torch.tensor([float("inf")], device="cuda"))
        assert bool(torch.isnan(dpred).all()), "nothing set and inv_n = inf: dpred must be NaN everywhere"
    # NaN / Inf in unset elements of pred and target reach neither the sum nor dpred
    for pattern in X.PATTERNS:
        m = X.mask(pattern, B, T, N).cuda()
        off = (X.expand(m, B, T, N) == 0).reshape(B * T, N)
        assert bool(off.any())
        inv_n = torch.tensor([1.0 / 99.0], device="cuda")
        clean, cnt = run_fwd(ops, spec, pred, tgt, m, B, T, N)
        dclean = run_bwd(ops, spec, pred, tgt, m, B, T, N, gout, inv_n)
        bad_p, bad_t = pred.clone(), tgt.clone()
        idx = torch.nonzero(off.reshape(-1)).reshape(-1)
        bad_p.view(-1)[idx[0::3]] = float("nan")
        bad_p.view(-1)[idx[1::3]] = float("inf")
        bad_t.view(-1)[idx[2::3]] = float("nan")
        bad_t.view(-1)[idx[0::3]] = float("-inf")
        out, cnt2 = run_fwd(ops, spec, bad_p, bad_t, m, B, T, N)
        E.check_exact(ibits(out), ibits(clean), f"{case} {pattern}: a NaN / Inf under the mask reached the sum")
        assert cnt2.item() == cnt.item()
        E.check_exact(ibits(run_bwd(ops, spec, bad_p, bad_t, m, B, T, N, gout, inv_n)), ibits(dclean),
                      f"{case} {pattern}: a NaN / Inf under the mask reached dpred")


def test_argument_checks(ops):
    from multi_modal_foundation_model_amd import _lib as Lb
    B, T, N = 2, 3, 4
    pred, tgt = torch.zeros(B * T, N, device="cuda"), torch.zeros(B * T, N, device="cuda")
    m = torch.ones(B, T, N, dtype=torch.uint8, device="cuda")
    out, cnt = torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(ops.masked_loss_elem_workspace(B, T, N) // 4 + 2, device="cuda")
    with pytest.raises(Lb.MmfmError, match="bad kind"):
        ops.masked_loss_elem_fwd(7, 0.0, 0, pred, tgt, m, B, T, N, out, cnt, ws)
    with pytest.raises(Lb.MmfmError, match="bad kind"):
        ops.masked_loss_elem_bwd(1, 0.0, 1, pred, tgt, m, B, T, N, out, out, pred.clone())      # the Stirling flag on MSE
    with pytest.raises(Lb.MmfmError, match="workspace"):
        ops.masked_loss_elem_fwd(1, 0.0, 0, pred, tgt, m, B, T, N, out, cnt, ws[:1])
    with pytest.raises(ValueError, match="element mask"):
        ops.masked_loss_elem_fwd(1, 0.0, 0, pred, tgt, m[:, :2], B, T, N, out, cnt, ws)
    with pytest.raises(ValueError, match="element mask"):
        ops.stage_masked(pred.view(B, T, N), m.bool(), B, T, N, pred.clone(), N)
    with pytest.raises(Lb.MmfmError, match="bad arguments"):
        ops.stage_masked(pred.view(B, T, N), m, B, T, N, pred.clone(), N - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,N", [(3, 5, 1), (3, 5, 12), (3, 5, 16), (3, 5, 65), (3, 5, 668), (41, 100, 5)])
def test_stage_masked_is_torch_where(ops, B, T, N, dtype):
    """dst = where(cm, 0, src) in the engine's input layout: rows padded to a multiple of 8 elements, the padding left alone."""
    ld = (N + 7) // 8 * 8
    src = torch.randn(B, T, N, generator=torch.Generator().manual_seed(3)).cuda() * 3
    src.view(-1)[0] = float("nan")                                   # set in every pattern: the select makes it 0
    for pattern in X.PATTERNS:
        cm = X.mask(pattern, B, T, N).cuda()
        dst = torch.zeros(B * T, ld, dtype=dtype, device="cuda")
        ops.stage_masked(src, cm, B, T, N, dst, ld)
        ref = X.stage_ref(src, X.expand(cm, B, T, N), dtype, ld)
        E.check_exact(ibits(dst), ibits(ref), f"stage_masked [{B}x{T}x{N}] {dtype} {pattern}")
    none = torch.zeros(1, 1, 1, dtype=torch.uint8, device="cuda")
    src.view(-1)[0] = 1.5
    dst = torch.zeros(B * T, ld, dtype=dtype, device="cuda")
    ops.stage_masked(src, none, B, T, N, dst, ld)
    E.check_exact(ibits(dst), ibits(X.stage_ref(src, X.expand(none, B, T, N), dtype, ld)), "stage_masked: no mask = the plain copy")
