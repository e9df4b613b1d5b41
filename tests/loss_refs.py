"""fp64 references and derived error bounds for the masked-loss kinds beyond PoissonNLL(log_input) / MSE (include/mmfm.h,
MMFM_LOSS_*; kinds 0 and 1 themselves are in tests/edge_refs.py, and kind 0 with the Stirling flag is here).

As in tests/edge_refs.py every reference takes the kernel's own inputs, upcasts them to fp64 (exact for bf16 and fp32) and returns
fp64; the kind's parameter is the fp32 value the kernel receives (`f32`).  tests/test_loss_family_cpu.py proves the references
against the torch modules in fp64; tests/test_loss_family_gpu.py compares the HIP kernels with them.

The forward sum is checked with edge_refs.check_sum: |out - ref| <= n 2^-24 sum|terms| + term_err.  term_err is the sum of the
per-element fp32 bounds derived below, with u = 2^-24 (one rounding), and these documented errors of the device functions:
  * __expf                       edge_refs.exp_rel_err: (2 + 2 |x|) u relative
  * logf, log1pf                 3 ulp = 6 u and 2 ulp = 4 u relative: the OpenCL full-profile bounds the ROCm device library is
                                 written to
  * a / b in fp32                correctly rounded (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt): u
A contracted multiply-add drops a rounding and stays inside the bound of the two separate operations.  Per kind, d = p - t:

  POISSON_RATE   p - t log(p + eps).  fl(p + eps) = (p + eps)(1 + u) moves the logarithm by u; logf adds 6 u |lg|; the product
                 u |t lg|; the subtraction u (|p| + |t lg|):      u (|p| + |t| (8 |lg| + 1)), stated with + 2 for the second order
  FULL           + t log t - t + log(2 pi t) / 2 where t > 1 (t is exact).  t logf(t): (6 + 1) u t lg t; - t: u (t lg t + t);
                 fl(fl(2 pi) t) moves the second logarithm by 2 u, logf by 6 u, halved: u (3 lg2 + 1); the sum of the two parts:
                 u st_mag with st_mag = t lg t + t + lg2 / 2.  Together u (9 t lg t + 2 t + 3.5 lg2 + 1), stated as
                 u (10 t lg t + 3 t + 4 lg2 + 1); adding the term to the element of magnitude mag:   + u (mag + st_mag)
  L1             |fl(p - t)|:                                     u |d|
  SMOOTH_L1      the function is 1-Lipschitz in d and continuous where the branches meet, so the rounded d (and a branch taken on
                 it) costs at most u |d|; then ((0.5 d) d) / beta: 2 u el, or |d| - 0.5 beta: u el:      u (|d| + 3 el)
  HUBER          delta-Lipschitz: delta u |d|; then (0.5 d) d: u el, or delta (|d| - 0.5 delta): 2 u el:  u (delta |d| + 3 el)
  BCE_LOGITS     max(p, 0) - p t + log1p(exp(-|p|)), x = exp(-|p|) <= 1.  p t: u |p t|; the subtraction u (|p| + |p t|);
                 __expf moves log1p's argument by exp_rel_err x and d log1p / dx <= 1; log1pf 4 u l1p; the last sum
                 u (|p| + |p t| + l1p):                           u (2 |p| + 3 |p t| + (2 + 2 |p|) x + 5 l1p)
"""
import math

import torch

from edge_refs import U32, exp_rel_err, f64

POISSON_LOG, MSE, POISSON_RATE, L1, SMOOTH_L1, HUBER, BCE_LOGITS = range(7)      # MMFM_LOSS_*
FULL = 1                                                                       # MMFM_LOSS_FULL


def f32(x):
    """The fp32 value a float parameter has once it is passed to the library."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _stirling(t):
    """(term, magnitude, fp32 bound without the final u * mag of the element it is added to); zero where t <= 1."""
    on = t > 1
    ts = torch.where(on, t, torch.ones_like(t))
    tl, lg2 = ts * torch.log(ts), torch.log(2 * math.pi * ts)
    z = torch.zeros_like(t)
    st = torch.where(on, tl - ts + 0.5 * lg2, z)
    mag = torch.where(on, tl + ts + 0.5 * lg2, z)
    err = torch.where(on, U32 * (10 * tl + 3 * ts + 4 * lg2 + 1), z)
    return st, mag, err, on


def loss_elem(kind, p, t, param=0.0, flags=0):
    """Per-element (loss, magnitude, fp32 error bound) in fp64 for fp64 p, t; the derivations are in the module docstring.
    Kinds 0 / 1 restate edge_refs.masked_loss_sum's terms, so that kind 0 can carry the Stirling flag."""
    a = f32(param)
    if kind == POISSON_LOG:
        e, b = torch.exp(p), t * p
        el, mag, err = e - b, e + b.abs(), (exp_rel_err(p) + U32) * e + 2 * U32 * b.abs()
    elif kind == MSE:
        el = (p - t) ** 2
        mag, err = el, 4 * U32 * el
    elif kind == POISSON_RATE:
        lg = torch.log(p + a)
        el, mag = p - t * lg, p.abs() + (t * lg).abs()
        err = U32 * (p.abs() + t.abs() * (8 * lg.abs() + 2))
    elif kind == BCE_LOGITS:
        x = torch.exp(-p.abs())
        l1p, pt = torch.log1p(x), p * t
        el, mag = p.clamp_min(0) - pt + l1p, p.clamp_min(0) + pt.abs() + l1p
        err = U32 * (2 * p.abs() + 3 * pt.abs() + (2 + 2 * p.abs()) * x + 5 * l1p)
    elif kind in (L1, SMOOTH_L1, HUBER):
        d = p - t
        ad = d.abs()
        if kind == L1 or (kind == SMOOTH_L1 and a == 0):
            el, lip = ad, 1.0
        elif kind == SMOOTH_L1:
            el, lip = torch.where(ad < a, 0.5 * d * d / a, ad - 0.5 * a), 1.0
        else:
            el, lip = torch.where(ad <= a, 0.5 * d * d, a * (ad - 0.5 * a)), a
        mag, err = el, U32 * (lip * ad + 3 * el)
    else:
        raise ValueError(f"kind {kind}")
    if flags & FULL:
        assert kind in (POISSON_LOG, POISSON_RATE)
        st, smag, serr, on = _stirling(t)
        err = err + serr + torch.where(on, U32 * (mag + smag), torch.zeros_like(t))
        el, mag = el + st, mag + smag
    return el, mag, err


def loss_grad(kind, p, t, param=0.0):
    """d loss_elem / dp in fp64 (the Stirling term has none), with torch's conventions at the ties: torch.sign(0) = 0, the smooth-L1
    branch is quadratic for |d| < beta only, Huber's for |d| <= delta (both continuous there)."""
    a = f32(param)
    d = p - t
    if kind == POISSON_LOG:
        return torch.exp(p) - t
    if kind == MSE:
        return 2.0 * d
    if kind == POISSON_RATE:
        return 1.0 - t / (p + a)
    if kind == BCE_LOGITS:
        return torch.sigmoid(p) - t
    if kind == L1 or (kind == SMOOTH_L1 and a == 0):
        return torch.sign(d)
    if kind == SMOOTH_L1:
        return torch.where(d.abs() < a, d / a, torch.sign(d))
    if kind == HUBER:
        return torch.where(d.abs() <= a, d, a * torch.sign(d))
    raise ValueError(f"kind {kind}")


def masked_loss_sum(kind, pred, target, rowmask, param=0.0, flags=0):
    """mm.py:217-239 with the kind's element: the modality's sum over masked rows.  rowmask: u8 [B, T] (any strides), row b*T + t
    of pred.  Returns (sum, n, sum_abs, term_err) as edge_refs.masked_loss_sum does.  Un-masked rows are dropped before the sum (the
    kernel never reads them), so a NaN there - log of a negative rate - does not reach it."""
    on = (rowmask != 0).reshape(-1)
    el, mag, err = loss_elem(kind, f64(pred)[on], f64(target)[on], param, flags)
    return el.sum(), float(on.sum()) * pred.shape[1], mag.sum(), err.sum()


def masked_loss_bwd(kind, pred, target, rowmask, grad_out, inv_n, param=0.0):
    """Autograd of (loss * mask).sum() / mask.sum(): dpred = grad_out * inv_n * mask * d/dp, as edge_refs.masked_loss_bwd: with
    nothing masked inv_n is inf and mask * inf = NaN on every row."""
    mk = f64(rowmask != 0).reshape(-1, 1)
    g = loss_grad(kind, f64(pred), f64(target), param)
    g = torch.where(mk != 0, g, torch.zeros_like(g))        # an un-masked row's own NaN / inf does not pass the mask
    return (f64(grad_out).reshape(()) * f64(inv_n).reshape(())) * mk * g


# ------------------------------------------------------------------------------------------------ the loss-family model
# tests/test_loss_family_model_gpu.py's three-modality model and batch shape; tests/plan_sig.py pins its step plans
FAMILY_MODS = [("ap", 12), ("behavior", 2), ("choice", 3)]
FAMILY_B, FAMILY_T = 2, 8


def make_family_model(dtype):
    import torch.nn as nn
    from helpers import build_model_mods, tiny_config
    model = build_model_mods(tiny_config(n_modality=3), FAMILY_MODS, seed=0)
    model.loss_mod["ap"] = nn.PoissonNLLLoss(log_input=False, full=True, reduction="none")
    model.loss_mod["behavior"] = nn.HuberLoss(reduction="none", delta=0.5)
    model.loss_mod["choice"] = nn.BCEWithLogitsLoss(reduction="none")
    with torch.no_grad():                      # a rate head: predictions must be positive for the reference itself to be finite
        model.decoder_embeddings["ap"].out.bias.fill_(4.0)
    model.compute_dtype = dtype
    return model.cuda()
