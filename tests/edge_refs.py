"""fp64 references and derived error bounds for the edge kernels (stitch / destitch, mask preparation, the masked loss,
LayerNorm, AdamW, the bf16 cast, column sums and slab reductions).

Every reference restates the operation from its semantics (mm.py / encoder_embeddings.py as cited in include/mmfm.h, and
oracle/mm_oracle.py where a function exists), takes the kernel's own inputs, upcasts them to fp64 (exact for bf16, fp32 and
the integer types) and returns fp64: no fp32 intermediate anywhere.  tests/test_edge_refs_cpu.py proves them against torch
autograd in fp64; tests/test_edge_kernels_gpu.py compares the HIP kernels with them.

Bounds are derived, not tuned:
  * bf16 outputs        |out - ref| <= 2^-8 |ref| + e32      2^-8 |ref| = half a bf16 ulp (8 significand bits, round to
                                                             nearest even); e32 = the fp32 bound of the arithmetic before it
  * fp32 sums           |out - ref| <= n 2^-24 sum|terms| + term_err
                                                             the worst case of recursive summation of n fp32 terms (any
                                                             order is inside it); term_err = sum of the per-term fp32 error
                                                             bounds where a term is itself computed (exp, (x - mu) rstd),
                                                             0 where the terms are stored values or exact products
  * fp32 elementwise    |out - ref| <= atol + rtol |ref|     the rtol / atol of the same kernel's test in test_kernels_gpu.py
  * integer / bit       exact
"""
import math

import torch

U32 = 2.0 ** -24          # unit roundoff of fp32 (24 significand bits, round to nearest)
HALF_ULP_BF16 = 2.0 ** -8  # half a bf16 ulp relative to the value (8 significand bits)

# fp32 elementwise tolerances (rtol, atol), each the one tests/test_kernels_gpu.py already uses for that kernel
TOL_STITCH = (2e-5, 2e-5)      # test_stitch_fwd_bwd: close() defaults for x, emb and d_tok
TOL_LN_Y = (2e-5, 2e-5)        # test_layernorm: close() defaults for y and mean
TOL_LN_DX = (1e-4, 1e-4)       # test_layernorm: "ln dx"
TOL_DPRED = (1e-5, 1e-8)       # test_masked_loss: "dpred"
TOL_LOSS = (1e-5, 2e-5)        # test_masked_loss: "loss" (rtol=1e-5, close()'s default atol)
TOL_ADAMW = (1e-6, 1e-7)       # test_adamw_matches_torch
# rstd has no test in test_kernels_gpu.py.  rstd = rsqrt(var + eps): var is a mean of H squares ((H + 3) 2^-24 worst case,
# half of it after the square root) and v_rsq_f32 is good to 1 ulp (2^-23): (H / 2 + 4) 2^-24 <= 3.1e-5 at H = 1024.  The
# bound below is that worst case at the largest H the kernel takes; there is no absolute part (rstd > 0 always).
TOL_LN_RSTD = ((1024 / 2 + 4) * U32, 0.0)


def f64(t):
    return t.to(torch.float64)


def exp_rel_err(p):
    """Relative error bound of the device's fast exp, __expf(p) = v_exp_f32(p * log2(e)).  V_EXP_F32 is documented to 1 ulp
    (2^-23) in the CDNA ISA guides; the argument y = fl(p * fl(log2 e)) carries two roundings, |dy| <= 2 * 2^-24 |y|, and
    2^(y + dy) = 2^y (1 + ln2 dy), ln2 |y| = |p|: together (2 + 2 |p|) 2^-24.  (The same shape as the 2 + floor(1.173 |x|) ulp
    the CUDA programming guide documents for its __expf.)  test_edge_refs_cpu.py checks that a plain fp32 exp sits inside it."""
    return (2.0 + 2.0 * f64(p).abs()) * U32


# ------------------------------------------------------------------------------------------------- tolerance helpers
def _worst(err, bound):
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(torch.finfo(torch.float64).tiny))
    bad = ~(err <= bound)                  # a NaN on either side fails
    return bad, (float(ratio.max()) if ratio.numel() else 0.0)


def _report(what, kind, bad, ratio, err, out, ref):
    print(f"[edge] {what}: {kind}, worst |err| / bound = {ratio:.3e}, max |err| = {float(err.max()) if err.numel() else 0.0:.3e}")
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the {kind}; worst |err| / bound = {ratio:.3e}; "
                             f"first at flat index {i}: out {float(out.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r}")
    return ratio


def check_bf16(out, ref, e32, what):
    """|out - ref| <= 2^-8 |ref| + e32 for a bf16 output; e32 (number or tensor) bounds the fp32 arithmetic before the rounding."""
    assert out.dtype == torch.bfloat16, f"{what}: expected a bf16 output, got {out.dtype}"
    o, r = f64(out).reshape(ref.shape), ref
    err = (o - r).abs()
    bound = HALF_ULP_BF16 * r.abs() + e32
    bad, ratio = _worst(err, bound + torch.zeros_like(r))
    return _report(what, "bf16 bound 2^-8 |ref| + e32", bad, ratio, err, o, r)


def check_sum(out, ref, n, sum_abs, what, term_err=0.0):
    """|out - ref| <= n 2^-24 sum|terms| + term_err for an fp32 sum of n terms (n, sum_abs, term_err: numbers or tensors)."""
    assert out.dtype == torch.float32, f"{what}: expected an fp32 output, got {out.dtype}"
    o, r = f64(out).reshape(ref.shape), ref
    err = (o - r).abs()
    bound = n * U32 * sum_abs + term_err
    bad, ratio = _worst(err, bound + torch.zeros_like(r))
    return _report(what, "fp32 sum bound n 2^-24 sum|terms|", bad, ratio, err, o, r)


def check_close(out, ref, tol, what):
    """|out - ref| <= atol + rtol |ref| for an fp32 elementwise output, against fp64; tol = (rtol, atol)."""
    assert out.dtype == torch.float32, f"{what}: expected an fp32 output, got {out.dtype}"
    rtol, atol = tol
    o, r = f64(out).reshape(ref.shape), ref
    err = (o - r).abs()
    bad, ratio = _worst(err, atol + rtol * r.abs())
    return _report(what, f"fp32 bound {atol:g} + {rtol:g} |ref|", bad, ratio, err, o, r)


def check_elem(out, ref, tol, what):
    """An elementwise output of either dtype: fp32 against tol, bf16 against half an ulp + the fp32 bound tol as e32."""
    if out.dtype == torch.bfloat16:
        return check_bf16(out, ref, tol[1] + tol[0] * ref.abs(), what)
    return check_close(out, ref, tol, what)


def check_exact(out, ref, what):
    assert out.dtype == ref.dtype and out.shape == ref.shape, f"{what}: {out.dtype} {tuple(out.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    if not torch.equal(out, ref):
        ne = out != ref
        i = int(torch.nonzero(ne.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ; first at flat index {i}: "
                             f"out {out.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r}")


def bits(t):
    """The raw 16-bit patterns of a bf16 tensor."""
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------- stitch
def clamp_ts(ts, max_F):
    """include/mmfm.h: time stamps are clamped into [0, max_F) (upstream indexes the table with them unchecked)."""
    return ts.clamp(0, max_F - 1)


def stitch_fwd(tok, mod_row, pos, ts, keep0, m, max_F):
    """encoder_embeddings.py:56-61 + mm.py:143-149,289 for modality m (oracle embed / zero_masked_tokens):
        emb[b, t] = mod_row + pos[ts[b, t]];   x[b, t] = keep0[m*T + t] * tok[b*T + t] + emb[b, t]
    Returns (x, emb, mag), each [B, T, H] fp64: the modality's slice [:, m*T:(m+1)*T] of the [B, L, H] outputs, and
    mag = |keep0 tok| + |mod_row| + |pos[ts]|, the scale of the two fp32 additions."""
    B, T = ts.shape
    H = tok.shape[-1]
    pe = f64(pos)[clamp_ts(ts, max_F)]
    emb = f64(mod_row)[None, None, :] + pe
    kt = f64(tok).view(B, T, H) * f64(keep0[m * T:(m + 1) * T])[None, :, None]
    return kt + emb, emb, kt.abs() + f64(mod_row).abs()[None, None, :] + pe.abs()


def stitch_fwd_e32(mag):
    """Two fp32 additions, each within 2^-24 of a partial sum that is itself <= mag: 2 * 2^-24 mag; 3 covers the second-order
    terms and the 2^-8 e32 by which half an ulp of the computed value can exceed half an ulp of the reference."""
    return 3 * U32 * mag


def stitch_bwd(dx, dextra, ts, keep0, keep, p, m, max_F):
    """Autograd of stitch_fwd for modality m (include/mmfm.h):
        d_tok[b*T + t] = keep0[m*T + t] * dropout'(dx[b, m*T + t])     dropout' = keep / (1 - p), keep a [B*T, H] 0/1 mask or None
        d_mod = sum_{b,t} (dx + dextra);   d_pos[f] = sum over (b, t) with ts[b, t] == f of (dx + dextra)
    Returns a dict: d_tok [B*T, H], d_mod [H], d_pos [max_F, H], and for the two sums the number of terms n_* and sum|terms|
    abs_* (the terms are the stored dx and dextra values)."""
    B, T = ts.shape
    H = dx.shape[-1]
    g = f64(dx)[:, m * T:(m + 1) * T].reshape(B * T, H)
    d_tok = g * f64(keep0[m * T:(m + 1) * T]).repeat(B)[:, None]
    if keep is not None:
        d_tok = d_tok * f64(keep).reshape(B * T, H) / (1.0 - p)
    terms = [g] + ([f64(dextra)[:, m * T:(m + 1) * T].reshape(B * T, H)] if dextra is not None else [])
    idx = clamp_ts(ts, max_F).reshape(-1)
    d_pos = torch.zeros(max_F, H, dtype=torch.float64, device=dx.device)
    abs_pos = torch.zeros_like(d_pos)
    for t in terms:
        d_pos.index_add_(0, idx, t)
        abs_pos.index_add_(0, idx, t.abs())
    n_pos = f64(torch.bincount(idx, minlength=max_F))[:, None] * len(terms)
    return dict(d_tok=d_tok, d_pos=d_pos, abs_pos=abs_pos, n_pos=n_pos, d_mod=sum(t.sum(0) for t in terms),
                abs_mod=sum(t.abs().sum(0) for t in terms), n_mod=B * T * len(terms))


# dropout' multiplies by fl(1 / fl(1 - p)) in fp32: two roundings in the factor and one in the product, 3 * 2^-24 relative
DROP_SCALE_REL = 3 * U32


# ------------------------------------------------------------------------------------------------- mask preparation
def mask_prep(masks, strides, attn, channels):
    """mm.py:270 (mask = eval_mask[:, :, 0] & attn_mask), :102 (mod_mask), :145,167 (argwhere(mask[0] == 1): sample 0 decides
    for every sample), :229-233 (n_examples = the mask expanded over the channels, summed); include/mmfm.h for the u8 outputs.
    masks[m] holds element (b, t) at flat index (b*T + t) * strides[m].  Returns tokmask, keypad [B, M*T] u8, keep0, mod_id
    [M*T] u8 and count [M] int64 = channels[m] * sum(mask & attn)."""
    B, T = attn.shape
    v = torch.cat([mk.reshape(-1)[::s][:B * T].view(B, T) & attn for mk, s in zip(masks, strides)], 1)
    M = len(masks)
    tokmask = (v != 0).to(torch.uint8)
    keypad = (attn != 0).to(torch.uint8).repeat(1, M)
    keep0 = (v[0] != 1).to(torch.uint8)
    mod_id = torch.arange(M, device=attn.device).repeat_interleave(T).to(torch.uint8)
    count = torch.stack([v[:, m * T:(m + 1) * T].sum() * int(channels[m]) for m in range(M)]).to(torch.int64)
    return tokmask, keypad, keep0, mod_id, count


# ------------------------------------------------------------------------------------------------- masked loss
def masked_loss_sum(kind, pred, target, rowmask):
    """mm.py:79-82,217-239 (oracle forward): the modality's sum over masked rows of exp(p) - t p (kind 0, PoissonNLLLoss with
    log_input=True, full=False) or (p - t)^2 (kind 1, MSELoss).  rowmask: u8 [B, T] (any strides), row b*T + t of pred.
    Returns (sum, n, sum_abs, term_err): n terms; sum_abs = sum of exp(p) + |t p| resp. (p - t)^2; term_err = the sum of the
    per-term fp32 bounds: (exp_rel_err(p) + 2^-24) exp(p) + 2 * 2^-24 |t p| (the fast exp, the product, the subtraction) resp.
    4 * 2^-24 (p - t)^2 (a subtraction and a product of the two rounded differences: (1 + u)^3)."""
    p, t = f64(pred), f64(target)
    mk = f64(rowmask != 0).reshape(-1, 1)
    if kind == 0:
        a, b = torch.exp(p), t * p
        el, mag, terr = a - b, a + b.abs(), (exp_rel_err(p) + U32) * a + 2 * U32 * b.abs()
    else:
        el = (p - t) ** 2
        mag, terr = el, 4 * U32 * el
    return (el * mk).sum(), float(mk.sum()) * p.shape[1], (mag * mk).sum(), (terr * mk).sum()


def loss_finalize(loss_sums, counts):
    """mm.py:237: loss = sum of the modality sums / sum of n_examples (0 / 0 = NaN, as upstream); inv_n = 1 / n."""
    n = f64(counts).sum()
    return f64(loss_sums).sum() / n, 1.0 / n


def masked_loss_bwd(kind, pred, target, rowmask, grad_out, inv_n):
    """Autograd of (loss * mask).sum() / mask.sum(): dpred = grad_out * inv_n * mask * d/dp.  With nothing masked inv_n is inf and
    mask * inf = NaN on every un-masked row, which is what upstream hands to autograd."""
    p, t = f64(pred), f64(target)
    mk = f64(rowmask != 0).reshape(-1, 1)
    d = torch.exp(p) - t if kind == 0 else 2.0 * (p - t)
    return (f64(grad_out).reshape(()) * f64(inv_n).reshape(())) * mk * d


# ------------------------------------------------------------------------------------------------- LayerNorm
def destitch_perm(R, L, T, device):
    """Row r = b*L + (m*T + t) of the stitched [B, L, H] sequence -> row m*(B*T) + b*T + t of the per-modality [M][B*T][H]
    layout (decoder_embeddings.py:95-97: dec_out[mod_mask == m] gathers modality m's rows); identity when T == 0."""
    r = torch.arange(R, device=device)
    if T <= 0:
        return r
    b, l = r // L, r % L
    return (l // T) * ((R // L) * T) + b * T + l % T


def layernorm_fwd(x, gamma, beta, eps=1e-5, ds_L=0, ds_T=0):
    """torch.nn.LayerNorm over the last dim (biased variance); y's rows in destitched order when ds_T > 0.
    Returns (y, mean, rstd)."""
    xd = f64(x)
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (xd - mu) * rstd * f64(gamma) + f64(beta)
    out = torch.empty_like(y)
    out[destitch_perm(x.shape[0], ds_L, ds_T, x.device)] = y
    return out, mu[:, 0], rstd[:, 0]


def layernorm_bwd(dy, x, gamma, dres, eps=1e-5, ds_L=0, ds_T=0):
    """Autograd of layernorm_fwd (dy's rows in destitched order when ds_T > 0) plus the residual gradient dres:
        dx = dres + rstd (g dy - mean(g dy) - xhat mean(g dy xhat));  dgamma = sum_r dy xhat;  dbeta = sum_r dy
    Returns a dict with dx, dgamma, dbeta, the sums' term count n, abs_gamma / abs_beta = sum|terms| and err_gamma, the sum of
    the per-term bounds of dgamma's computed terms: xhat = (x - mu) rstd in fp32 is within
        (H + 8) 2^-24 (|xhat| + rstd mean|x|)
    (the mean: H additions and a product, (H + 2) 2^-24 mean|x|; rstd: half the variance's (H + 3) 2^-24 plus rsqrt and the
    products), and the product with dy adds 2^-24 |dy xhat|.  dbeta's terms are the stored dy: no per-term error."""
    R, H = x.shape
    xd, g = f64(x), f64(gamma)
    d = f64(dy)[destitch_perm(R, ds_L, ds_T, x.device)]
    mu = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (xd - mu) * rstd
    gd = d * g
    dx = rstd * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + f64(dres)
    xh_err = (H + 8) * U32 * (xh.abs() + rstd * xd.abs().mean(-1, keepdim=True))
    return dict(dx=dx, dgamma=(d * xh).sum(0), dbeta=d.sum(0), n=R, abs_gamma=(d * xh).abs().sum(0), abs_beta=d.abs().sum(0),
                err_gamma=(d.abs() * xh_err).sum(0) + U32 * (d * xh).abs().sum(0))


# ------------------------------------------------------------------------------------------------- AdamW
def adamw_hyper(step, lr, beta1, beta2=0.999, eps=1e-8, wd=0.01, grad_scale=1.0):
    """The hyper[8] vector of mmfm_adamw_step (csrc/optim.hip), computed in double; step is 1-based:
    [1 - lr wd, 1 - beta1, beta2, 1 - beta2, lr / bias_correction1, sqrt(bias_correction2), eps, grad_scale]."""
    return [1 - lr * wd, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1 ** step), math.sqrt(1 - beta2 ** step), eps, grad_scale]


def adamw_step(p, g, m, v, hyper):
    """torch.optim.AdamW's single-tensor update (oracle adamw_step) written from the hyper vector; the gradient is multiplied by
    grad_scale first.  p, m, v are fp64 state tensors, updated in place; g and hyper are upcast."""
    h = [float(x) for x in f64(hyper).reshape(-1).tolist()]
    gs = f64(g) * h[7]
    p.mul_(h[0])
    m.add_(h[1] * (gs - m))                      # exp_avg.lerp_(grad, 1 - beta1)
    v.mul_(h[2]).add_(h[3] * gs * gs)            # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    p.sub_(h[4] * (m / (v.sqrt() / h[5] + h[6])))


# ------------------------------------------------------------------------------------------------- fp32 reductions
def colsum(x, prior=None):
    """out[n] = (prior[n] +) sum_r x[r, n].  Returns (sum, n_terms, sum_abs); the terms are stored values."""
    xd = f64(x)
    s, a, n = xd.sum(0), xd.abs().sum(0), x.shape[0]
    if prior is not None:
        s, a, n = s + f64(prior), a + f64(prior).abs(), n + 1
    return s, n, a


def reduce_slabs(src, n, nslabs, stride, prior=None):
    """dst[i] = (prior[i] +) sum_s src[s * stride + i], i < n.  Returns (sum, n_terms, sum_abs)."""
    sl = torch.stack([f64(src.reshape(-1)[s * stride:s * stride + n]) for s in range(nslabs)])
    return colsum(sl, prior)
