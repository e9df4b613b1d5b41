"""The two-workgroups-per-CU form of the dX + norm-backward kernels at K = 512 / 768 (csrc/rowgemm.hip rowgemm_lnbwd2_kernel) behind
mmfm_rowgemm (ln_bwd = 1, 2) and mmfm_rowgemm_groups (backward, 2 and 5 groups):

  * element by element against the fp64 reference of tests/rowowner_refs.py (norm_bwd) under the bound derived there, and
  * bit for bit (torch.equal) against the one-workgroup kernels it replaces - same k order through the ring, same MFMA accumulation,
    same reductions of the norm backward; only the owner of a row differs.

MMFM_ROWGEMM_LNBWD_WG is read at every launch of these kernels: 2 forces the new form at every row count (the default takes it only
beyond 256 row passes), 1 forces the old kernels.  Row counts: a pass is 32 * NW = 128 rows (NW = 4 waves, one 32-row tile each); beyond
2 x 256 passes a workgroup of the new form walks more than one pass (66,085 rows = 517 passes, the last one of 37 rows).  Every output
buffer carries guard rows and a sentinel, the strided case NaN pad columns, as in tests/test_rowowner_elementwise_gpu.py."""
import os

import pytest
import torch

import rowowner_refs as RR

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FILL = 1e30
GUARD = 3
NAN = float("nan")
NW = 4
ROWS = [1, 31, 32 * NW - 1, 32 * NW, 32 * NW + 1, 5 * 32 * NW + 7, 516 * 32 * NW + 37]
ENV = "MMFM_ROWGEMM_LNBWD_WG"


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


@pytest.fixture(autouse=True)
def _restore_env():
    old = os.environ.get(ENV)
    yield
    if old is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = old


def form(v, R, K):
    """Select the kernel form of the following launches: 2 = two workgroups per CU, 1 = the one-workgroup kernels, None = the default
    (two workgroups beyond 256 row passes).  The dispatcher's own answer (mmfm_rowgemm_lnbwd_form) must follow: a switch that was ignored
    would let the bit-identity assertions compare a kernel with itself."""
    from multi_modal_foundation_model_amd import _lib as L
    if v is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = str(v)
    want = v if v is not None else (2 if (R + 32 * NW - 1) // (32 * NW) > 256 else 1)
    got = L.lib().mmfm_rowgemm_lnbwd_form(R, K)
    assert got == want, f"{ENV}={v} R={R} K={K}: the dispatcher takes form {got}, expected {want}"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda") * scale


def obuf(R, N, ld=None):
    return torch.full((R + GUARD, ld or N), FILL, device="cuda", dtype=BF)


def done(buf, R, N, what):
    out = buf[:R, :N]
    RR.assert_written(out, FILL, what)
    RR.assert_untouched(buf[R:], FILL, f"{what}: guard rows")
    if buf.shape[1] > N:
        RR.assert_untouched(buf[:R, N:], FILL, f"{what}: pad columns")
    return out


def padded(t, ld):
    buf = torch.full((t.shape[0], ld), NAN, device="cuda", dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf


_cache = {}


def operands(R, K, norm, groups=1):
    """dY operands per group, weights (slices of one tensor), x_hat / rstd as a norm prologue saves them (ScaleNorm: one clamped row,
    rstd < 0), residual gradient.  Computed once per (R, K, norm, groups) and left unchanged."""
    key = (R, K, norm, groups)
    if key not in _cache:
        _cache.clear()                                  # one large case resident at a time
        dys = [rnd(R, K, seed=1 + g).to(BF) for g in range(groups)]
        W = (rnd(groups, 256, K, seed=2) * K ** -0.5 * (16.0 if norm == 2 else 1.0)).to(BF)
        x = (rnd(R, 256, seed=4) * 2 + rnd(R, 1, seed=8) * 3).to(BF)
        if norm == 2:
            x[R // 2] = 0.0
        xh64, rs64, _ = RR.norm_fwd(x, norm)
        _cache[key] = (dys, W, xh64.to(BF).contiguous(), rs64.float().contiguous(), rnd(R, 256, seed=5).to(BF))
    return _cache[key]


def run_single(ops, v, R, K, norm, dys, W, xhat, rstd, res, what, ld=None):
    form(v, R, K)
    ldx, ldy, ldr = ld or (K, 256, 256)
    dx = obuf(R, 256, ldy)
    ops.rowgemm(dys[0] if ld is None else padded(dys[0], ldx), W[0], dx, R, 256, K, ldx=ldx, ldw=K, ldy=ldy,
                residual=None if res is None else (res if ld is None else padded(res, ldr)), ldr=ldr if res is not None else 0,
                ln_bwd=norm, bwd_xhat=xhat, bwd_rstd=rstd)
    torch.cuda.synchronize()
    return done(dx, R, 256, f"{what} form={v}")


@pytest.mark.parametrize("K", [512, 768])
@pytest.mark.parametrize("R", ROWS)
def test_rowgemm_lnbwd_two_wg(ops, R, K):
    for norm in (1, 2):
        dys, W, xhat, rstd, dres = operands(R, K, norm)
        for res in (dres, None):
            what = f"two-wg rowgemm ln_bwd={norm} R={R} K={K} res={res is not None}"
            new = run_single(ops, 2, R, K, norm, dys, W, xhat, rstd, res, what)
            RR.check_norm_bwd(new, dys, [W[0]], xhat, rstd, res, norm, what)
            old = run_single(ops, 1, R, K, norm, dys, W, xhat, rstd, res, what)
            assert torch.equal(new, old), f"{what}: differs from the one-workgroup kernel in {int((new != old).sum())} elements"
            dflt = run_single(ops, None, R, K, norm, dys, W, xhat, rstd, res, what)
            assert torch.equal(dflt, old), f"{what}: the default dispatch differs from the one-workgroup kernel"


@pytest.mark.parametrize("K", [512, 768])
def test_rowgemm_lnbwd_two_wg_strided(ops, K):
    """ldx / ldy / ldr larger than the row: NaN pad columns in the inputs, sentinel pad columns in the output."""
    R = 5 * 32 * NW + 7
    for norm in (1, 2):
        dys, W, xhat, rstd, dres = operands(R, K, norm)
        what = f"two-wg strided rowgemm ln_bwd={norm} K={K}"
        ld = (K + 8, 264, 272)
        new = run_single(ops, 2, R, K, norm, dys, W, xhat, rstd, dres, what, ld=ld)
        RR.check_norm_bwd(new, dys, [W[0]], xhat, rstd, dres, norm, what)
        assert torch.equal(new, run_single(ops, 1, R, K, norm, dys, W, xhat, rstd, dres, what, ld=ld)), f"{what}: differs from the one-workgroup kernel"
        assert torch.equal(new, run_single(ops, 2, R, K, norm, dys, W, xhat, rstd, dres, what)), f"{what}: differs from the packed launch"


def run_groups(ops, v, R, G, norm, dys, W, xhat, rstd, res, what, ld=None):
    form(v, R, 512)
    ldx, ldy, ldr = ld or (512, 256, 256)
    dx = obuf(R, 256, ldy)
    ops.rowgemm_groups(dys if ld is None else [padded(t, ldx) for t in dys], [W[g] for g in range(G)], [dx], R, 256, 512, ldx=ldx, ldw=512, ldy=ldy,
                       residual=None if res is None else (res if ld is None else padded(res, ldr)), ldr=ldr if res is not None else 0,
                       ln_bwd=norm, bwd_xhat=xhat, bwd_rstd=rstd)
    torch.cuda.synchronize()
    return done(dx, R, 256, f"{what} form={v}")


@pytest.mark.parametrize("G", [2, 5])
@pytest.mark.parametrize("R", ROWS)
def test_rowgemm_groups_lnbwd_two_wg(ops, R, G):
    for norm in (1, 2):
        dys, W, xhat, rstd, dres = operands(R, 512, norm, groups=G)
        for res in (dres, None):
            what = f"two-wg groups bwd ln_bwd={norm} R={R} G={G} res={res is not None}"
            new = run_groups(ops, 2, R, G, norm, dys, W, xhat, rstd, res, what)
            RR.check_norm_bwd(new, dys, [W[g] for g in range(G)], xhat, rstd, res, norm, what)
            old = run_groups(ops, 1, R, G, norm, dys, W, xhat, rstd, res, what)
            assert torch.equal(new, old), f"{what}: differs from the one-workgroup kernel in {int((new != old).sum())} elements"
            assert torch.equal(run_groups(ops, None, R, G, norm, dys, W, xhat, rstd, res, what), old), f"{what}: the default dispatch differs"


def test_rowgemm_groups_lnbwd_two_wg_strided(ops):
    R, G = 5 * 32 * NW + 7, 5
    for norm in (1, 2):
        dys, W, xhat, rstd, dres = operands(R, 512, norm, groups=G)
        what = f"two-wg strided groups bwd ln_bwd={norm}"
        ld = (520, 264, 272)
        new = run_groups(ops, 2, R, G, norm, dys, W, xhat, rstd, dres, what, ld=ld)
        RR.check_norm_bwd(new, dys, [W[g] for g in range(G)], xhat, rstd, dres, norm, what)
        assert torch.equal(new, run_groups(ops, 1, R, G, norm, dys, W, xhat, rstd, dres, what, ld=ld)), f"{what}: differs from the one-workgroup kernel"
