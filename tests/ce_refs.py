"""fp64 reference and derived fp32 error bounds for the softmax cross-entropy of categorical modalities (include/mmfm.h,
MMFM_LOSS_SOFTMAX_CE; csrc/softmax_ce.hip), the inputs its kernel tests run on, and the categorical model of the whole-model tests.

As in tests/loss_refs.py every reference takes the kernel's own inputs, upcasts them to fp64 (exact for bf16 and fp32) and returns
fp64; the smoothing is the fp32 value the kernel receives (`f32`).  tests/test_softmax_ce_cpu.py proves the reference against
F.cross_entropy and autograd in fp64; tests/test_softmax_ce_gpu.py compares the HIP kernels with it.  For logits p[c], targets t[c]
>= 0, class weights w[c] (None: 1) and smoothing eps, with C classes:

    t'[c] = (1 - eps) t[c] + eps / C        e[c] = w[c] t'[c] (lse(p) - p[c])        d/dp[j] = softmax(p)[j] S - w[j] t'[j],  S = sum_c w[c] t'[c]

The bounds, with u = 2^-24 (one fp32 rounding), x_c = p_c - m (m the row maximum), d_c = lse - p_c >= 0, and the documented errors
tests/loss_refs.py uses: __expf (2 + 2 |x|) u relative (edge_refs.exp_rel_err), logf 3 ulp = 6 u relative.  A sum of C non-negative
terms carries at most (C - 1) u relative in ANY order, so no bound depends on how the lanes share a row:

  wt = w t'        fl(1 - eps), fl(eps / C), one fmaf, one product: 4 u relative (every part is non-negative)
  s = sum exp(x)   fl(p_c - m): u |x_c| in the argument; __expf: (2 + 2 |x_c|) u; the sum: (C - 1) u.
                   ds = sum_c exp(x_c) (2 + 3 |x_c|) u / s + (C - 1) u      relative
  ls = logf(s)     d log s = ds, logf 6 u |log s|:   dls = ds + 6 u log s     absolute
  lse = m + ls     dlse = dls + u |lse|                                        absolute (this is rowstat[0]; rowstat[1] = S: (C + 3) u relative)
  forward term     wt_c fl(fl(m - p_c) + ls): u (m - p_c) + dls + u d_c inside, 4 u for wt, u for the product:
                   wt_c (dls + u (m - p_c) + 6 u d_c), stated with 7 u d_c for the second order
                   The row sum and the sum over rows are checked with edge_refs.check_sum: n u sum|terms| + the sum of these.
  gradient         sm_j = __expf(fl(p_j - lse)), y_j = p_j - lse: dlse shifts the argument, fl() u |y_j|, __expf (2 + 2 |y_j|) u:
                   relative dlse + (2 + 3 |y_j|) u.  S: (C + 3) u.  A = sm_j S, one product: rA = dlse + (2 + 3 |y_j|) u + (C + 4) u.
                   d = fl(A - wt_j): A rA + 4 u wt_j + u |d|.  g = fl(grad_out inv_n) and the last product: 2 u |g d|:
                   |g| (A rA + 4 u wt_j + 3 u |d|), stated as |g| (A rA + 5 u wt_j + 4 u |d|)
Underflow: an exponential below the smallest normal fp32 number, 2^-126, comes back as a denormal or as 0 (the relative bound of
__expf does not hold there), at most 2^-126 off; so may the gradient's last product.  ds takes + C 2^-126 and the gradient's bound
+ 2^-126 (|g| S + 1): nothing next to the other terms unless a softmax value is itself that small (logits 180 apart).
A bf16 dpred is that value rounded once: edge_refs.check_bf16 with the bound above (times 1 + 2^-8) as e32.
Non-finite logits are outside the contract.  With nothing masked inv_n is inf and every dpred is NaN; an un-masked row's dpred is
g * 0 exactly.
"""
import math

import torch

from edge_refs import HALF_ULP_BF16, U32, exp_rel_err, f64
from loss_refs import f32

SOFTMAX_CE = 7                       # MMFM_LOSS_SOFTMAX_CE
TINY32 = 2.0 ** -126                 # the smallest normal fp32 number


def group_lanes(C):
    """The lanes that own a row of C classes: the smallest power of two >= min(C, 64)."""
    g = 1
    while g < C and g < 64:
        g <<= 1
    return g


def smooth(t, eps, C=None):
    """t' = (1 - eps) t + eps / C over the last axis."""
    e = f32(eps)
    return (1.0 - e) * t + e / (t.shape[-1] if C is None else C)


def _wt(t, w, eps, C=None):
    tp = smooth(t, eps, C)
    return tp if w is None else w.to(tp.dtype) * tp


def ce_elem(p, t, w=None, eps=0.0):
    """The [..., C] tensor e = - w t' log_softmax(p) in fp64 for fp64 p, t."""
    return _wt(t, w, eps) * (torch.logsumexp(p, -1, keepdim=True) - p)


def ce_grad(p, t, w=None, eps=0.0):
    """d (sum_c e[c]) / dp in fp64."""
    wt = _wt(t, w, eps)
    return torch.softmax(p, -1) * wt.sum(-1, keepdim=True) - wt


def _row_terms(p, t, w, eps):
    """Per row, what the bounds are made of: wt, m - p, lse, d = lse - p, dls and dlse (absolute)."""
    C = p.shape[-1]
    wt = _wt(t, w, eps)
    m = p.max(-1, keepdim=True).values
    x = p - m
    ex = torch.exp(x)
    s = ex.sum(-1, keepdim=True)
    ds = (ex * (2.0 + 3.0 * x.abs())).sum(-1, keepdim=True) * U32 / s + (C - 1) * U32 + C * TINY32
    dls = ds + 6.0 * U32 * torch.log(s)
    lse = m + torch.log(s)
    return wt, -x, lse, lse - p, dls, dls + U32 * lse.abs()


def rowstat(pred, target, w=None, eps=0.0):
    """(lse, S) per row with their fp32 bounds: ([R, 2] fp64, [R, 2] fp64 absolute bounds)."""
    p, t = f64(pred), f64(target)
    wt, _, lse, _, _, dlse = _row_terms(p, t, w, eps)
    S = wt.sum(-1, keepdim=True)
    return torch.cat([lse, S], -1), torch.cat([dlse, (p.shape[-1] + 3) * U32 * S], -1)


def masked_ce_sum(pred, target, rowmask, w=None, eps=0.0):
    """mm.py:217-239 with e: the modality's sum over masked rows.  rowmask: u8 [B, T] (any strides), row b*T + t of pred.  Returns
    (sum, n, sum_abs, term_err) as loss_refs.masked_loss_sum does; n = C * (masked rows), upstream's n_examples."""
    on = (rowmask != 0).reshape(-1)
    p, t = f64(pred)[on], f64(target)[on]
    wt, mp, _, d, dls, _ = _row_terms(p, t, w, eps)
    el = wt * d
    err = wt * (dls + U32 * mp + 7.0 * U32 * d)
    return el.sum(), float(on.sum()) * pred.shape[1], el.sum(), err.sum()


def masked_ce_bwd(pred, target, rowmask, grad_out, inv_n, w=None, eps=0.0):
    """Autograd of (e * mask).sum() / mask.sum(): (dpred in fp64, its fp32 bound).  Un-masked rows: g * 0 - exactly 0, or NaN when
    nothing is masked anywhere (inv_n = inf)."""
    mk = f64(rowmask != 0).reshape(-1, 1)
    p, t = f64(pred), f64(target)
    C = p.shape[-1]
    g = f64(grad_out).reshape(()) * f64(inv_n).reshape(())
    wt, _, lse, d, _, dlse = _row_terms(p, t, w, eps)
    A = torch.exp(-d) * wt.sum(-1, keepdim=True)
    grad = A - wt
    rA = dlse + (2.0 + 3.0 * d) * U32 + (C + 4) * U32
    bound = g.abs() * (A * rA + 5.0 * U32 * wt + 4.0 * U32 * grad.abs()) + TINY32 * (g.abs() * wt.sum(-1, keepdim=True) + 1.0)
    zero = torch.zeros_like(grad)
    return g * mk * torch.where(mk != 0, grad, zero), torch.where(mk != 0, bound, zero)


def check_dpred(out, ref, bound, what):
    """fp32: |out - ref| <= bound; bf16: within one bf16 rounding of it (edge_refs.check_bf16)."""
    from edge_refs import _report, _worst, check_bf16
    if out.dtype == torch.bfloat16:
        return check_bf16(out, ref, bound * (1.0 + HALF_ULP_BF16), what)
    assert out.dtype == torch.float32, f"{what}: expected fp32, got {out.dtype}"
    o = f64(out).reshape(ref.shape)
    err = (o - ref).abs()
    bad, ratio = _worst(err, bound)
    return _report(what, "derived fp32 bound", bad, ratio, err, o, ref)


def within(out, ref, bound):
    """True where every element of `out` is inside `bound` of `ref` (a NaN or inf on either side is outside)."""
    return bool(((f64(out).reshape(ref.shape) - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ the kernel tests' inputs
# Made on the CPU from seeded generators, so that tests/test_softmax_ce_cpu.py judges the bounds on the very tensors
# tests/test_softmax_ce_gpu.py hands to the kernels.
# both sides of the 64-lane group, a partly filled group, more than one column per lane; 300 and 1030: the wider register form
# (up to 1024 columns) and the streamed rows beyond it
CLASSES = (1, 2, 3, 5, 64, 65, 130, 300, 1030)
SHAPES = ((3, 1, 1, 0), (20, 5, 13, 8))      # (R, T, mask_ld, first mask column): R = 20 reads a strided view of a [4, 13] token mask
VARIANTS = ("plain", "weighted", "unnormalised", "scaled")
NEAR = 90.0                                  # exp(90) overflows fp32: the row that needs the maximum subtracted


def variant_params(variant, C, seed=0):
    """(class weights or None, label smoothing) of a variant."""
    if variant in ("plain", "scaled"):
        return None, 0.0
    g = torch.Generator().manual_seed(1000 + seed + C)
    return 0.25 + 1.5 * torch.rand(C, generator=g), (0.1 if variant == "weighted" else 0.3)


def make_inputs(variant, C, R, dtype, seed=0):
    """(pred in dtype, fp32 target) on the CPU.  plain / weighted: index (one-hot) targets on even rows, probability targets on odd
    rows; unnormalised: non-negative weights that do not sum to 1; scaled: logits times 30, row 1 alternating +-NEAR with the target
    on a -NEAR class (index targets)."""
    g = torch.Generator().manual_seed(7 * C + R + seed)
    pred = torch.randn(R, C, generator=g) * (30.0 if variant == "scaled" else 2.0)
    onehot = torch.nn.functional.one_hot(torch.randint(0, C, (R,), generator=g), C).float()
    prob = torch.softmax(torch.randn(R, C, generator=g), -1)
    if variant == "unnormalised":
        tgt = 3.0 * torch.rand(R, C, generator=g)
    elif variant == "scaled":
        tgt = onehot
        pred[1] = NEAR * (1.0 - 2.0 * (torch.arange(C) % 2).float())           # +90, -90, +90, ...
        tgt[1] = 0.0
        tgt[1, min(1, C - 1)] = 1.0
    else:
        tgt = torch.where((torch.arange(R) % 2 == 0)[:, None], onehot, prob)
    return pred.to(dtype), tgt.contiguous()


def make_masks(R, T, mask_ld, off):
    """name -> u8 token-mask storage [B, mask_ld]; the loss reads the view [:, off:off + T].  'mixed' has masked and un-masked rows
    and keeps row 1 (the scaled variant's +-NEAR row) masked; 'none' masks nothing of this modality."""
    B = R // T
    g = torch.Generator().manual_seed(R + 3)
    out = {}
    for name in ("mixed", "none"):
        st = (torch.rand(B, mask_ld, generator=g) < 0.5).to(torch.uint8)          # the other modalities' columns: anything
        view = st[:, off:off + T]
        if name == "none":
            view.zero_()
        else:
            flat = (torch.rand(R, generator=g) < 0.6).to(torch.uint8)
            flat[0], flat[1], flat[R - 1] = 0, 1, 1
            view.copy_(flat.view(B, T))
        out[name] = st
    return out


# ------------------------------------------------------------------------------------------------ three faulty kernels
# What the bounds must reject (tests/test_softmax_ce_cpu.py), each restated on the CPU.
def faulty_grad_without_weight_sum(pred, target, rowmask, grad_out, inv_n, w, eps):
    """softmax - w t': the hard-label gradient, wrong as soon as sum w t' != 1."""
    mk = f64(rowmask != 0).reshape(-1, 1)
    p, t = f64(pred), f64(target)
    g = f64(grad_out).reshape(()) * f64(inv_n).reshape(())
    return g * mk * (torch.softmax(p, -1) - _wt(t, w, eps))


def faulty_smoothing_by_group(pred, target, rowmask, w, eps):
    """eps / G instead of eps / C: the lanes of the group taken for the classes."""
    on = (rowmask != 0).reshape(-1)
    p, t = f64(pred)[on], f64(target)[on]
    wt = _wt(t, w, eps, C=group_lanes(p.shape[-1]))
    return (wt * (torch.logsumexp(p, -1, keepdim=True) - p)).sum()


def faulty_sum_without_max(pred, target, rowmask, w, eps):
    """log(sum exp(p)) in fp32 without the maximum subtracted."""
    on = (rowmask != 0).reshape(-1)
    p, t = pred.float()[on], target[on]
    lse = torch.log(torch.exp(p).sum(-1, keepdim=True))
    wt = smooth(t, eps).float() if w is None else w.float() * smooth(t, eps).float()
    return (wt * (lse - p)).sum()


# ------------------------------------------------------------------------------------------------ confusion
def first_argmax(x):
    """The lowest index of the maximum over the last axis (torch.argmax does not promise which index a tie gets)."""
    C = x.shape[-1]
    idx = torch.arange(C, device=x.device).expand_as(x)
    return torch.where(x == x.max(-1, keepdim=True).values, idx, torch.full_like(idx, C)).min(-1).values


def confusion(pred, target, rowmask=None):
    """int64 [C, C], row = target class, over the masked rows, in plain torch."""
    C = pred.shape[-1]
    pi, ti = first_argmax(pred.float().reshape(-1, C)), first_argmax(target.float().reshape(-1, C))
    if rowmask is not None:
        on = (rowmask != 0).reshape(-1)
        pi, ti = pi[on], ti[on]
    return torch.bincount(ti * C + pi, minlength=C * C).view(C, C)


# ------------------------------------------------------------------------------------------------ the categorical models
# The two fixture cases (tests/golden/softmax_ce_fwd_bwd.npz, scripts/make_softmax_ce_goldens.py): a per-trial label - a segmented
# plan - and a per-bin label - the uniform plan.  Tiny config H = 32 / 4 heads / inter 64 / max_F 8 / dropout 0, n_modality = 3.
CE_B, CE_MODEL_SEED, CE_DATA_SEED, CE_MASKER_SEED = 3, 7, 3, 11
CE_CASES = {
    "choice": dict(mods=[("ap", 12), ("behavior", 2), ("choice", 3)], T=(8, 8, 1), weight=(0.5, 2.0, 1.25), eps=0.1),
    "state": dict(mods=[("ap", 12), ("behavior", 2), ("state", 5)], T=(8, 8, 8), weight=None, eps=0.0),
}
CE_OBJECTIVES = ("eval_masks", "token_masking")


def one_hot(labels, C):
    return torch.nn.functional.one_hot(labels, C).to(torch.float32)


def ce_batch(case, seed=CE_DATA_SEED):
    """mod -> dict(inputs [B, T_mod, N_mod], ts, attn): Poisson(0.3) spikes, N(0, 1) behaviour and one-hot labels from one generator."""
    c = CE_CASES[case]
    g = torch.Generator().manual_seed(seed)
    out = {}
    for (mod, n), T in zip(c["mods"], c["T"]):
        if mod == "ap":
            x = torch.poisson(torch.full((CE_B, T, n), 0.3), generator=g)
        elif mod == "behavior":
            x = torch.randn(CE_B, T, n, generator=g)
        else:
            x = one_hot(torch.randint(0, n, (CE_B, T), generator=g), n)
        out[mod] = dict(inputs=x, ts=torch.arange(T, dtype=torch.int64)[None].repeat(CE_B, 1), attn=torch.ones(CE_B, T, dtype=torch.int64))
    return out


def ce_mod_dict(case, batch, objective):
    """What upstream's trainer would build of the batch, each modality with its own bins.  eval_masks: the categorical modality fully
    masked, half of the behaviour bins, no spikes; token_masking: the model's masker draws."""
    import numpy as np
    c = CE_CASES[case]
    md = {}
    n_ap = batch["ap"]["inputs"].shape[-1]
    for i, (mod, n) in enumerate(c["mods"]):
        s = batch[mod]
        x = s["inputs"]
        d = dict(inputs_modality=torch.tensor(i), targets_modality=torch.tensor(i), inputs_attn_mask=s["attn"], inputs_timestamp=s["ts"],
                 targets_timestamp=s["ts"], eid="synthetic", num_neuron=n_ap, masking_mode=None, inputs=x.clone(), targets=x.clone())
        if mod == "ap":
            d["inputs_regions"] = np.full((x.shape[0], n_ap), "XX")
        if objective == "token_masking":
            d["eval_mask"] = None
        elif objective == "eval_masks":
            mk = torch.zeros_like(x).to(torch.int64)
            if mod == "behavior":
                mk[:, ::2] = 1
            elif mod != "ap":
                mk[:] = 1
            d["eval_mask"] = mk
        else:
            raise ValueError(objective)
        md[mod] = d
    return md


def make_ce_model(case, dtype="fp32"):
    """The mirror's model of a fixture case on the GPU: the construction order and seed of scripts/make_softmax_ce_goldens.py, the
    categorical modality's loss_mod entry a multi_modal.losses.SoftmaxCrossEntropy."""
    from helpers import build_model_mods, tiny_config
    from multi_modal.losses import SoftmaxCrossEntropy
    c = CE_CASES[case]
    model = build_model_mods(tiny_config(n_modality=3), c["mods"], seed=CE_MODEL_SEED)
    model.loss_mod[c["mods"][2][0]] = SoftmaxCrossEntropy(weight=c["weight"], label_smoothing=c["eps"])
    model.compute_dtype = dtype
    return model.cuda()
