"""The masked-loss kinds beyond PoissonNLL(log_input) / MSE through the C ABI (mmfm_masked_loss_kind_fwd / _bwd), fp32 and bf16,
against the fp64 references and derived bounds of tests/loss_refs.py (proved on the CPU by tests/test_loss_family_cpu.py), and kinds
0 / 1 through the new entry points bit for bit against the two-kind ones.  Runs on the MI355X only."""
import pytest
import torch

import edge_refs as E
import loss_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]
SHAPES = [(60, 668, 10),          # N is no multiple of the 64 lanes
          (4100, 12, 100),        # rows on both sides of the 4096-row grid stride
          (4100, 2, 100)]
GUARD, SENT = 4096, 0xA5
# name: (kind, param, flags)
CASES = {"poisson_rate": (R.POISSON_RATE, 1e-8, 0), "poisson_rate_full": (R.POISSON_RATE, 1e-8, R.FULL),
         "poisson_log_full": (R.POISSON_LOG, 0.0, R.FULL), "l1": (R.L1, 0.0, 0), "smooth_l1": (R.SMOOTH_L1, 0.5, 0),
         "smooth_l1_beta0": (R.SMOOTH_L1, 0.0, 0), "huber": (R.HUBER, 0.5, 0), "bce": (R.BCE_LOGITS, 0.0, 0)}


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=gen(seed), device="cuda") * scale


def guarded(nbytes):
    buf = torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[:nbytes]


def row_masks(B, T, M):
    """The four [B, M*T] token masks of test_edge_kernels_gpu.py::test_masked_loss; the loss reads modality 1's slice."""
    Rr = B * T
    bern = (torch.rand(B, M * T, generator=gen(6), device="cuda") < 0.3).to(torch.uint8)
    ones = torch.ones(B, M * T, dtype=torch.uint8, device="cuda")
    other_only = ones.clone()
    other_only[:, T:] = 0
    edges = torch.zeros(Rr, dtype=torch.uint8, device="cuda")
    edges[[r for r in (0, 4095, 4096, Rr - 2, Rr - 1) if 0 <= r < Rr]] = 1
    e2 = torch.zeros(B, M * T, dtype=torch.uint8, device="cuda")
    e2[:, T:] = edges.view(B, T)
    return [("bernoulli", bern), ("all", ones), ("none of this modality", other_only), ("edge rows", e2)]


def inputs(case, Rr, N, dtype):
    """(pred in dtype, fp32 target) with the values at which the kind can go wrong."""
    if case.startswith("poisson"):
        tgt = torch.poisson(torch.full((Rr, N), 0.3, device="cuda"), generator=gen(2))
        assert bool((tgt >= 2).any()), "no target >= 2: the Stirling term would not be exercised"
        if case == "poisson_log_full":
            pred = rnd(Rr, N, seed=1, scale=2.5).clamp_(-8.0, 8.0).to(dtype)
        else:
            pred = (1e-3 + (20.0 - 1e-3) * torch.rand(Rr, N, generator=gen(1), device="cuda")).clamp_(1e-3, 20.0).to(dtype)
            assert pred.min().item() > 0 and pred.max().item() <= 20.0
    elif case == "bce":
        pred = rnd(Rr, N, seed=1, scale=3.5).clamp_(-12.0, 12.0)
        pred.view(-1)[:4] = torch.tensor([7.5, -7.5, 9.0, -9.0], device="cuda")          # row 0 is in the 'all' and 'edge rows' masks
        pred = pred.to(dtype)
        assert pred.abs().max().item() >= 7.0
        tgt = (torch.rand(Rr, N, generator=gen(2), device="cuda") < 0.5).float()
    else:
        tgt = torch.randint(-3, 4, (Rr, N), generator=gen(2), device="cuda").float()
        pred = tgt + rnd(Rr, N, seed=1)
        i = torch.arange(Rr * N, device="cuda").view(Rr, N)
        pred = torch.where(i % 5 == 0, tgt, pred)                          # d == 0
        pred = torch.where(i % 5 == 1, tgt + 0.5, pred)                    # |d| == beta == delta, exact in bf16 (|t| <= 3)
        pred = torch.where(i % 5 == 2, tgt - 0.5, pred).to(dtype)
        d = pred.float() - tgt
        assert bool((d == 0).any()) and bool((d == 0.5).any()) and bool((d == -0.5).any())
    return pred, tgt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R_,N,T", SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_masked_loss_kinds(ops, case, R_, N, T, dtype):
    from multi_modal_foundation_model_amd import _lib as Lb
    kind, param, flags = CASES[case]
    B, M = R_ // T, 2
    pred, tgt = inputs(case, R_, N, dtype)
    nbytes = Lb.lib().mmfm_masked_loss_workspace(R_, N)
    gout = torch.tensor([0.5], device="cuda")
    other_sum, other_n = 3.0, 7
    for name, tokmask in row_masks(B, T, M):
        what = f"masked_loss {case} [{R_}x{N}] {name}"
        rowmask = tokmask[:, T:]
        out = torch.full((1,), float("nan"), device="cuda")
        buf, ws = guarded(nbytes)
        ops.masked_loss_kind_fwd(kind, param, flags, pred, tgt, rowmask, M * T, T, R_, N, out, ws)
        assert bool((buf[nbytes:] == SENT).all()), f"{what}: wrote behind its {nbytes}-byte workspace"
        s, n, sabs, terr = R.masked_loss_sum(kind, pred, tgt, rowmask, param, flags)
        E.check_sum(out, s.reshape(1), n, sabs, f"{what} sum", term_err=terr)
        if n == 0:
            assert out.item() == 0.0
        sums = torch.stack([torch.tensor(other_sum, device="cuda"), out[0]])
        cnt = torch.tensor([other_n, int(rowmask.sum().item()) * N], dtype=torch.int64, device="cuda")
        loss, inv_n = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        ops.loss_finalize(sums, cnt, 2, loss, inv_n)
        dpred = torch.full((R_, N), 7.0, dtype=dtype, device="cuda")
        ops.masked_loss_kind_bwd(kind, param, flags, pred, tgt, rowmask, M * T, T, R_, N, gout, inv_n, dpred)
        ref = R.masked_loss_bwd(kind, pred, tgt, rowmask, gout, inv_n, param)
        E.check_elem(dpred, ref, E.TOL_DPRED, f"{what} dpred")
        off = (rowmask == 0).reshape(R_)
        assert bool((dpred[off] == 0).all()), f"{what}: dpred must be exactly zero on un-masked rows"
    # nothing masked in any modality: 0 / 0 = NaN, inv_n = inf, and every gradient NaN
    none = torch.zeros(B, M * T, dtype=torch.uint8, device="cuda")
    loss, inv_n = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    ops.loss_finalize(torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), 2, loss, inv_n)
    assert bool(torch.isnan(loss[0])) and bool(torch.isinf(inv_n[0]))
    dpred = torch.full((R_, N), 7.0, dtype=dtype, device="cuda")
    ops.masked_loss_kind_bwd(kind, param, flags, pred, tgt, none[:, T:], M * T, T, R_, N, gout, inv_n, dpred)
    assert bool(torch.isnan(R.masked_loss_bwd(kind, pred, tgt, none[:, T:], gout, inv_n, param)).all())
    assert bool(torch.isnan(dpred).all()), "nothing masked: dpred must be NaN everywhere"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R_,N,T", SHAPES)
@pytest.mark.parametrize("kind", [0, 1])
def test_original_kinds_bit_identical_through_the_new_entry_points(ops, kind, R_, N, T, dtype):
    from multi_modal_foundation_model_amd import _lib as Lb
    B, M = R_ // T, 2
    pred = rnd(R_, N, seed=1, scale=2.5).clamp_(-8.0, 8.0).to(dtype)
    tgt = torch.poisson(torch.full((R_, N), 0.3, device="cuda"), generator=gen(2)) if kind == 0 else rnd(R_, N, seed=2)
    nbytes = Lb.lib().mmfm_masked_loss_workspace(R_, N)
    gout, inv_n = torch.tensor([0.5], device="cuda"), torch.tensor([1.0 / 1234.0], device="cuda")
    for name, tokmask in row_masks(B, T, M):
        rowmask = tokmask[:, T:]
        outs, grads = [], []
        for new in (False, True):
            out = torch.full((1,), float("nan"), device="cuda")
            dpred = torch.full((R_, N), 7.0, dtype=dtype, device="cuda")
            buf, ws = guarded(nbytes)
            if new:
                ops.masked_loss_kind_fwd(kind, 0.0, 0, pred, tgt, rowmask, M * T, T, R_, N, out, ws)
                ops.masked_loss_kind_bwd(kind, 0.0, 0, pred, tgt, rowmask, M * T, T, R_, N, gout, inv_n, dpred)
            else:
                ops.masked_loss_fwd(kind, pred, tgt, rowmask, M * T, T, R_, N, out, ws)
                ops.masked_loss_bwd(kind, pred, tgt, rowmask, M * T, T, R_, N, gout, inv_n, dpred)
            assert bool((buf[nbytes:] == SENT).all())
            outs.append(out)
            grads.append(dpred)
        E.check_exact(outs[1].view(torch.int32), outs[0].view(torch.int32), f"kind {kind} {name}: sum bits")
        E.check_exact(grads[1].view(torch.int32 if dtype == F32 else torch.int16), grads[0].view(torch.int32 if dtype == F32 else torch.int16),
                      f"kind {kind} {name}: dpred bits")
