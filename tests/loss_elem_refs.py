"""fp64 references for the masked losses under a per-element mask (include/mmfm.h, MMFM_LOSS_ELEM) and for the masked staging copy.

The elements, their magnitudes and their fp32 error bounds are tests/loss_refs.py's own (`loss_elem`, `loss_grad`), unchanged: a
per-element mask only selects which of them enter the sum, so the sum bound stays edge_refs.check_sum's
n 2^-24 sum|terms| + term_err with n the number of SET elements, and the gradient bound stays edge_refs.TOL_DPRED.
"""
import torch

import loss_refs as R
from edge_refs import f64

# name: (kind, param, flags) - every kind, with the Stirling flag where it is legal
CASES = {"poisson_log": (R.POISSON_LOG, 0.0, 0), "poisson_log_full": (R.POISSON_LOG, 0.0, R.FULL), "mse": (R.MSE, 0.0, 0),
         "poisson_rate": (R.POISSON_RATE, 1e-8, 0), "poisson_rate_full": (R.POISSON_RATE, 1e-8, R.FULL), "l1": (R.L1, 0.0, 0),
         "smooth_l1": (R.SMOOTH_L1, 0.5, 0), "huber": (R.HUBER, 0.5, 0), "bce": (R.BCE_LOGITS, 0.0, 0)}
PATTERNS = ("BT1", "B1N", "11N", "1T1", "BTN", "BTN_strided")


def inputs(case, Rr, N, dtype, seed=0):
    """(pred in dtype, fp32 target) on the CPU, with the values at which the kind can go wrong planted in the first elements."""
    g = torch.Generator().manual_seed(seed)
    if case.startswith("poisson"):
        tgt = torch.poisson(torch.full((Rr, N), 0.6), generator=g)
        tgt.view(-1)[:3] = torch.tensor([0.0, 1.0, 3.0])                  # the Stirling term: off at t <= 1, on at 3
        if case.startswith("poisson_log"):
            pred = (torch.randn(Rr, N, generator=g) * 2.5).clamp_(-8.0, 8.0)
        else:
            pred = 1e-3 + (20.0 - 1e-3) * torch.rand(Rr, N, generator=g)
    elif case == "bce":
        pred = (torch.randn(Rr, N, generator=g) * 3.5).clamp_(-12.0, 12.0)
        pred.view(-1)[:2] = torch.tensor([7.5, -9.0])
        tgt = (torch.rand(Rr, N, generator=g) < 0.5).float()
    else:
        tgt = torch.randint(-3, 4, (Rr, N), generator=g).float()
        pred = tgt + torch.randn(Rr, N, generator=g)
        pred.view(-1)[:3] = tgt.view(-1)[:3] + torch.tensor([0.0, 0.5, -0.5])      # d == 0, |d| == beta == delta
    return pred.to(dtype), tgt


def mask(pattern, B, T, N, density=0.4, seed=1):
    """A compact u8 mask of broadcast pattern `pattern` on the CPU: broadcast dimensions are kept at size 1; "BTN_strided" is a full
    mask that is not contiguous (a transposed view).  Elements 0..2 of row 0 are set where the pattern allows."""
    g = torch.Generator().manual_seed(seed)
    shape = {"BT1": (B, T, 1), "B1N": (B, 1, N), "11N": (1, 1, N), "1T1": (1, T, 1), "BTN": (B, T, N), "BTN_strided": (B, N, T)}[pattern]
    m = (torch.rand(shape, generator=g) < density).to(torch.uint8)
    m.view(-1)[0] = 1
    return m.transpose(1, 2) if pattern == "BTN_strided" else m


def expand(m, B, T, N):
    return m.expand(B, T, N)


def elem_loss_sum(kind, pred, target, full_mask, param=0.0, flags=0):
    """(sum, n, sum_abs, term_err) over the set elements of full_mask [B, T, N]; unset elements are dropped before the sum (the kernel
    never loads them), so a NaN there does not reach it."""
    on = (full_mask != 0).reshape(-1)
    el, mag, err = R.loss_elem(kind, f64(pred).reshape(-1)[on], f64(target).reshape(-1)[on], param, flags)
    return el.sum(), int(on.sum()), mag.sum(), err.sum()


def elem_loss_bwd(kind, pred, target, full_mask, grad_out, inv_n, param=0.0):
    """dpred = grad_out * inv_n * mask * d/dp: mask * inf = NaN everywhere when nothing is set anywhere (inv_n = inf)."""
    mk = f64(full_mask != 0).reshape(pred.shape)
    g = R.loss_grad(kind, f64(pred), f64(target), param)
    g = torch.where(mk != 0, g, torch.zeros_like(g))
    return (f64(grad_out).reshape(()) * f64(inv_n).reshape(())) * mk * g


def stage_ref(src, cm_full, dtype, ld):
    """torch.where(cm, 0, src) in `dtype`, in rows of pitch ld whose padding columns keep the value 0."""
    B, T, N = src.shape
    out = torch.zeros(B * T, ld, dtype=dtype, device=src.device)
    out[:, :N] = torch.where(cm_full != 0, torch.zeros_like(src), src).reshape(B * T, N).to(dtype)
    return out
