"""fp64 references, derived error bounds and exact-integer inputs for the row-owner kernels (mmfm_rowgemm, mmfm_rowgemm_groups,
mmfm_mlp_fwd, mmfm_mlp_bwd), in the style of tests/edge_refs.py, whose helpers this file reuses.

Every reference takes the kernel's own inputs - and, where a stage reads a bf16 tensor an earlier stage of the same kernel stored
(x_hat, du), that stored tensor - upcasts them to fp64 (exact) and returns fp64.  One bf16 rounding then separates kernel and
reference, and every element of every row is compared: no norm is taken over a tensor anywhere.  tests/test_rowowner_refs_cpu.py
proves the references against torch autograd and the checks against injected faults; tests/test_rowowner_elementwise_gpu.py
compares the HIP kernels with them.

Two kinds of case:

  exact     generators of inputs for which every product, every fp32 partial sum and the final value is an integer (or, for the
            ScaleNorm x_hat, a sixteenth of one) of magnitude <= 256.  Such values are exact in bf16 (8 significand bits: every
            integer up to 256) and in fp32 accumulation in any order (every integer up to 2^24), so the kernel output must be
            torch.equal to the reference whatever its tiling, summation order or launch shape.  The condition is part of each
            generator: it asserts |value| <= 256 for the result and for every intermediate the kernel rounds to bf16.

  bounds    randn-type inputs.  With u = 2^-24 (fp32 unit roundoff):
              one product + epilogue   |out - ref| <= 2^-8 |ref| + (K + 3) u (sum_k |x_k w_k| + |bias| + |res|)
                  K - 1 fp32 additions of exact bf16 x bf16 products in any order, the bias and the residual additions, and one
                  for the second-order terms and the 2^-8 e32 by which half an ulp of the computed value can exceed half an ulp
                  of the reference (as edge_refs.stitch_fwd_e32)
              x_hat / rstd             edge_refs' LayerNorm bounds; the ScaleNorm analogue is derived at norm_fwd
              norm backward epilogue   derived at norm_bwd
              MLP stages               derived at mlp_bwd_refs / mlp_fwd_ref; the activation error terms are the ones the project
                                       has established (act_err below), not fitted to these kernels
"""
import math

import torch

from edge_refs import HALF_ULP_BF16, TOL_LN_RSTD, U32, check_bf16, check_close, check_exact, f64  # noqa: F401 (re-exported for the tests)

BF = torch.bfloat16
H = 256                    # the row-owner kernels' model width
INTER = 512                # and their MLP's intermediate width
EXACT_MAX = 256            # integers up to here are exact in bf16

# The row counts of the GPU tests: the smallest that reach each launch shape of the dispatchers (csrc/rowgemm.hip grid_for and
# mmfm_rowgemm / mmfm_rowgemm_groups, csrc/mlp_fused.hip grid_for and mmfm_mlp_fwd / mmfm_mlp_bwd).  A pass is 128 rows (4 row tiles of
# 32: 4 waves, or 4 wave pairs) in every kernel but the MLP backward's front half, whose 8 waves own 256.
#   33        one partial 32-row tile beside a full one
#   129       one pass plus one row
#   1000      a ragged pass; 8 passes < 128, so the K = 256 forward splits N into column blocks (ny > 1; grid.y = 4 on the residual path)
#   16,424    129 passes: the first size (beyond 128 passes = 16,384 rows) at which the column split is off
#   66,085    grid_for(R, per_cu, nw) = min(ceil(R / 32 nw), 256 per_cu) workgroups, and a workgroup walks a second pass once there are
#             more passes than workgroups.  per_cu = 1, 128-row passes (the ln_bwd kernels, the K = 512 / 768 forward, the grouped dX,
#             mmfm_mlp_fwd, the one-launch mmfm_mlp_bwd): beyond 256 x 128 = 32,768 rows.  per_cu = 1, 256-row passes (the MLP backward's
#             front half) and per_cu = 2, 128-row passes (the K = 256 forward, single and grouped): beyond 65,536 rows.  66,085 =
#             516 x 128 + 37 rows are 517 passes of 128 (5 workgroups of the two-per-CU forward walk a second one, the one-per-CU
#             kernels two or three each) and 259 of 256 (3 workgroups of the front half walk a second one); the last pass holds 37 rows:
#             one full tile, one of 5 rows, the rest idle
ROWS = [33, 129, 1000, 16384 + 40, 516 * 128 + 37]

# mmfm_mlp_desc.act (include/mmfm.h)
ACT_GELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2


# ------------------------------------------------------------------------------------------------- activations
def _phi(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _Phi(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2)))


def act_f(kind, u, beta=1.0):
    """The activation in fp64: exact-erf GELU, ReLU, u sigmoid(beta u)."""
    if kind == ACT_GELU:
        return u * _Phi(u)
    if kind == ACT_RELU:
        return u.clamp_min(0)
    return u * torch.sigmoid(beta * u)


def act_d1(kind, u, beta=1.0):
    """Its derivative (ReLU: 0 at u = 0 and below, as torch's threshold backward and the kernels' select)."""
    if kind == ACT_GELU:
        return _Phi(u) + u * _phi(u)
    if kind == ACT_RELU:
        return (u > 0).to(u.dtype)
    s = torch.sigmoid(beta * u)
    return s + beta * u * s * (1 - s)


def act_d2(kind, u, beta=1.0):
    """Its second derivative: how an error of u moves act'(u) (ReLU: 0 away from the step, where the exact cases keep it)."""
    if kind == ACT_GELU:
        return _phi(u) * (2 - u * u)
    if kind == ACT_RELU:
        return torch.zeros_like(u)
    s = torch.sigmoid(beta * u)
    ds = beta * s * (1 - s)
    return ds * (2 + beta * u * (1 - 2 * s))


def act_err(kind, u, beta=1.0):
    """(|f error|, |f' error|) of the kernels' fp32 activation forms at an exact argument u, from what the project has established:
      GELU     the packed degree-9 polynomial Phi (csrc/common.h phi2): 5e-5 + 4e-5 |u| and 1e-4, the fp32 parts of the bounds
               test_gemm_bf16_gelu_polynomial_accuracy (tests/test_kernels_gpu.py) holds the same functions to on [-9, 9]
      sigmoid  v_exp_f32 / v_rcp_f32: 1e-6 |u| and 1e-6 (1 + |beta u|) (a few fp32 ulp of s; f' = s (1 + z (1 - s)), z = beta u)
      ReLU     a select: none."""
    a = u.abs()
    if kind == ACT_GELU:
        return 5e-5 + 4e-5 * a, torch.full_like(u, 1e-4)
    if kind == ACT_RELU:
        return torch.zeros_like(u), torch.zeros_like(u)
    return 1e-6 * a, 1e-6 * (1 + beta * a)


# ------------------------------------------------------------------------------------------------- one product + epilogue
def product(x, w, bias=None, res=None):
    """y = x . w^T + bias + res for x [R, K] and w [N, K] (any strides).  Returns (ref, e32) with
    e32 = (K + 3) 2^-24 (sum_k |x_k w_k| + |bias| + |res|), the fp32 bound of the module docstring."""
    xd, wd = f64(x), f64(w)
    ref, mag = xd @ wd.T, xd.abs() @ wd.abs().T
    for t in (bias, res):
        if t is not None:
            ref, mag = ref + f64(t), mag + f64(t).abs()
    return ref, (x.shape[1] + 3) * U32 * mag


def check_product(out, x, w, bias, res, what):
    ref, e32 = product(x, w, bias, res)
    return check_bf16(out, ref, e32, what)


# ------------------------------------------------------------------------------------------------- norm prologue
def norm_fwd(x, norm, eps=1e-5):
    """The row prologue of a norm-fed product (csrc/rowchain.h ln_rows / sn_rows), without the affine part (folded into the prepared
    weights).  norm = 1: x_hat = (x - mean) rstd, rstd = 1 / sqrt(var + eps) (biased variance);  norm = 2: x_hat = x rstd,
    rstd = 1 / max(||x||, eps), saved NEGATED for a clamped row (||x|| <= eps).  Returns (x_hat [R, H], rstd [R] as saved, e32):
    e32 bounds the fp32 arithmetic behind the bf16 x_hat:
      LayerNorm   (H + 8) 2^-24 (|x_hat| + rstd mean|x|): edge_refs.layernorm_bwd's x_hat term (the mean: H additions and a product;
                  rstd: half the variance's (H + 3) 2^-24 plus the reciprocal square root and the products)
      ScaleNorm   ||x||^2 is a sum of H rounded squares, all positive: (H + 1) 2^-24 relative, half of it after the square root, which
                  adds 2^-24; the reciprocal is good to 1 ulp (2 * 2^-24): rstd within (H / 2 + 4) 2^-24 - edge_refs.TOL_LN_RSTD's
                  shape, which check_norm therefore uses for both norms - and the product x rstd adds 2^-24, one more for the
                  second-order terms: (H / 2 + 6) 2^-24 |x_hat|."""
    xd = f64(x)
    n = xd.shape[1]
    if norm == 1:
        mu = xd.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + eps)
        xh = (xd - mu) * rstd
        return xh, rstd[:, 0], (n + 8) * U32 * (xh.abs() + rstd * xd.abs().mean(1, keepdim=True))
    nrm = xd.norm(dim=1, keepdim=True)
    rstd = 1.0 / nrm.clamp_min(eps)
    xh = xd * rstd
    return xh, torch.where(nrm > eps, rstd, -rstd)[:, 0], (n / 2 + 6) * U32 * xh.abs()


def check_norm(xhat, rstd, x, norm, what, eps=1e-5):
    """x_hat (bf16) and rstd (fp32) as saved by a norm prologue against norm_fwd of the same x."""
    xh, rs, e32 = norm_fwd(x, norm, eps)
    return check_bf16(xhat, xh, e32, f"{what} x_hat"), check_close(rstd, rs, TOL_LN_RSTD, f"{what} rstd")


# ------------------------------------------------------------------------------------------------- norm backward epilogue
def norm_bwd(xs, ws, xhat, rstd, res, norm):
    """mmfm_rowgemm / mmfm_rowgemm_groups with ln_bwd = norm (include/mmfm.h), from the kernel's operands:
        v = sum_g xs[g] . ws[g]^T          xs[g] [R, K], ws[g] [H, K] (WpT of group g's forward linear); v stays fp64 here
        norm = 1:  y = res + rstd (v - mean(v) - x_hat mean(v x_hat))
        norm = 2:  y = res + |rstd| (v - x_hat sum(v x_hat)),  the sum dropped where rstd < 0 (clamped row)
    Returns (ref, e32).  Derivation of e32, u = 2^-24, H = 256 features, n = the number of products summed into one v (groups x K):
      * the kernel's v is an fp32 sum of n exact products in some order:      |dv_j| <= n u sum|x w|  =: ev_j
      * m1 = mean(v): H fp32 additions of the computed v_j and an exact scaling by 2^-8:
                                                                              |dm1| <= mean(ev) + H u mean|v|
      * m2 = mean(v x_hat) (ScaleNorm: the sum): each term one more rounded product:
                                                                              |dm2| <= mean(ev |x_hat|) + (H + 1) u mean|v x_hat|
      * t = v - m1 - x_hat m2: a product and two subtractions, every intermediate within A = |v| + |m1| + |x_hat m2|:
                                                                              |dt| <= ev + |dm1| + |x_hat| |dm2| + 3 u A
      * y = res + rstd t: a product and an addition, every intermediate within |res| + rstd A:  2 u (|res| + rstd A)
      and one more u (|res| + rstd A) for the second-order terms and the 2^-8 e32 of the bf16 half ulp:
        e32 = rstd (ev + |dm1| + |x_hat| |dm2|) + 6 u (|res| + rstd A)
    (the 3 u A of t enters multiplied by rstd: 3 + 2 + 1 = 6).  Lane exchanges and the order of any of the sums stay inside it."""
    v = sum(f64(x) @ f64(w).T for x, w in zip(xs, ws))
    ev = sum(x.shape[1] for x in xs) * U32 * sum(f64(x).abs() @ f64(w).abs().T for x, w in zip(xs, ws))
    xh, rs = f64(xhat), f64(rstd).reshape(-1, 1)
    n = v.shape[1]
    if norm == 1:
        m1, m2 = v.mean(1, keepdim=True), (v * xh).mean(1, keepdim=True)
        dm1 = ev.mean(1, keepdim=True) + n * U32 * v.abs().mean(1, keepdim=True)
        dm2 = (ev * xh.abs()).mean(1, keepdim=True) + (n + 1) * U32 * (v * xh).abs().mean(1, keepdim=True)
    else:
        live = (rs > 0).to(v.dtype)
        m1, m2 = torch.zeros_like(rs), (v * xh).sum(1, keepdim=True) * live
        dm1 = torch.zeros_like(rs)
        dm2 = ((ev * xh.abs()).sum(1, keepdim=True) + (n + 1) * U32 * (v * xh).abs().sum(1, keepdim=True)) * live
        rs = rs.abs()
    A = v.abs() + m1.abs() + (xh * m2).abs()
    ref, mag = rs * (v - m1 - xh * m2), rs * A
    if res is not None:
        ref, mag = ref + f64(res), mag + f64(res).abs()
    return ref, rs * (ev + dm1 + xh.abs() * dm2) + 6 * U32 * mag


def check_norm_bwd(out, xs, ws, xhat, rstd, res, norm, what):
    ref, e32 = norm_bwd(xs, ws, xhat, rstd, res, norm)
    return check_bf16(out, ref, e32, what)


# ------------------------------------------------------------------------------------------------- the fused MLP
def _up(xhat, w_up, b_up):
    """u = x_hat . W_up^T + b_up in fp64 and the fp32 bound of the kernels' u (one product: (K + 3) u sum|terms|)."""
    return product(xhat, w_up, b_up)


def mlp_fwd_ref(x, xhat, w_up, b_up, w_down, b_down, kind, beta=1.0):
    """y = x + act(x_hat . W_up^T + b_up) . W_down^T + b_down from the kernel's own stored x_hat (w_down [H, INTER] in natural
    order).  The 512-wide intermediate g never leaves the CU: the kernel rounds act(u) to bf16 and multiplies that, so its rounding
    is propagated through the second product instead of being read back:
        dg_j = 2^-8 |g_j| + e_act(u_j) + |act'(u_j)| e32(u_j)          rounding + activation form + the fp32 error of u
        e32  = sum_j |W_down[n][j]| dg_j + (INTER + 4) 2^-24 (sum_j |g_j W_down[n][j]| + |b_down| + |x|)
    (the second sum: INTER - 1 additions, bias, residual, and the second-order terms).  Returns (ref, e32)."""
    u, eu = _up(xhat, w_up, b_up)
    g = act_f(kind, u, beta)
    ef, _ = act_err(kind, u, beta)
    dg = HALF_ULP_BF16 * g.abs() + ef + act_d1(kind, u, beta).abs() * eu
    wd = f64(w_down)
    ref, mag = f64(x) + g @ wd.T, f64(x).abs() + g.abs() @ wd.abs().T
    if b_down is not None:
        ref, mag = ref + f64(b_down), mag + f64(b_down).abs()
    return ref, dg @ wd.abs().T + (wd.shape[1] + 4) * U32 * mag


def mlp_bwd_refs(xhat, w_up, b_up, t1, w_down_t, kind, beta=1.0):
    """g and du of mmfm_mlp_bwd (one launch or front half) from its inputs; t1 = dropout'(dy) = dy without dropout:
        u = x_hat . W_up^T + b_up (recomputed),   g = act(u),   du = (t1 . W_down) act'(u)        w_down_t = W_down^T [INTER, H]
    Returns a dict with g, e_g, du, e_du.  One product each, then the activation:
        e_g  = e_act(u) + |act'(u)| e32(u)
        e_du = |act'(u)| e32(t1 . W_down) + |t1 . W_down| (e_act'(u) + |act''(u)| e32(u)) + 2 * 2^-24 |du|
    (the product's fp32 error scaled by the factor; the factor's own form error and the move of act' under the error of u; the
    product of the two and the second-order terms)."""
    u, eu = _up(xhat, w_up, b_up)
    ef, ed = act_err(kind, u, beta)
    d1 = act_d1(kind, u, beta)
    dg, edg = product(t1, w_down_t)
    du = dg * d1
    return dict(u=u, g=act_f(kind, u, beta), e_g=ef + d1.abs() * eu, du=du,
                e_du=d1.abs() * edg + dg.abs() * (ed + act_d2(kind, u, beta).abs() * eu) + 2 * U32 * du.abs())


def check_mlp_bwd(g, du, xhat, w_up, b_up, t1, w_down_t, kind, what, beta=1.0):
    r = mlp_bwd_refs(xhat, w_up, b_up, t1, w_down_t, kind, beta)
    return check_bf16(g, r["g"], r["e_g"], f"{what} g"), check_bf16(du, r["du"], r["e_du"], f"{what} du")


# ------------------------------------------------------------------------------------------------- sentinels
def assert_written(out, fill, what):
    """No element of the rows a launch owns may still hold the fill value (a sentinel the result cannot take)."""
    left = out == torch.tensor(fill, dtype=out.dtype, device=out.device)
    assert not bool(left.any()), f"{what}: {int(left.sum())} elements still hold the fill value {fill}, first at flat index {int(torch.nonzero(left.reshape(-1))[0])}"


def assert_untouched(buf, fill, what):
    """Guard rows and pad columns must still hold the fill value (NaN fills compare as NaN)."""
    ok = torch.isnan(buf) if fill != fill else buf == torch.tensor(fill, dtype=buf.dtype, device=buf.device)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} guard / pad elements were overwritten"


# ------------------------------------------------------------------------------------------------- exact-integer inputs
def _gen(seed, device="cpu"):
    """The generators draw on the device they build the case for (the large cases would otherwise spend their time in the host's
    generator); the streams of the two devices differ, which is why every generator asserts its condition itself on every call."""
    return torch.Generator(device=device).manual_seed(seed)


def _randint(lo, hi, shape, g):
    return torch.randint(lo, hi, shape, generator=g, device=g.device)


def _pm(m, shape, g):
    """Uniform on {-m .. -1, 1 .. m}: no zero operands, so every dropped or doubled product changes a result."""
    return _randint(1, m + 1, shape, g) * (_randint(0, 2, shape, g) * 2 - 1)


def _ints(m, shape, g):
    return _randint(-m, m + 1, shape, g)


def _sparse_pm1(inv_density, shape, g):
    return _pm(1, shape, g) * (_randint(0, inv_density, shape, g) == 0)


def balanced_rows(R, g):
    """Rows that are a random arrangement of exactly H / 2 values +1 and H / 2 values -1: mean 0, variance 1, so the LayerNorm's
    x_hat = +-1 / sqrt(1 + eps) = +-0.999995 rounds to bf16 +-1 exactly."""
    return torch.where(torch.rand(R, H, generator=g, device=g.device).argsort(1) < H // 2, 1, -1)


def _exact(name, t):
    """t (fp64, integer valued) -> bf16, asserting the condition that makes the case exact."""
    m = float(t.abs().max())
    assert m <= EXACT_MAX, f"exact case: max |{name}| = {m} > {EXACT_MAX}: not exactly representable in bf16"
    assert bool((t == t.round()).all()), f"exact case: {name} is not integer valued"
    return t.to(BF)


def exact_rowgemm(R, N, K, device, seed=0, bias=True, residual=True):
    """Plain mmfm_rowgemm: x in {-1, 1} (K = 256: {-2, -1, 1, 2}), W in {-1, 1}, integer bias in [-8, 8] and residual in [-16, 16].
    The sum of K such products has sigma sqrt(K) <= 27.8 (K = 256: sqrt(2.5 K) = 25.3): 256 - 24 is more than 8 sigma away."""
    g = _gen(seed, device)
    x = _pm(2 if K == 256 else 1, (R, K), g)
    W = _pm(1, (N, K), g)
    b = _ints(8, (N,), g).float() if bias else None
    r = _ints(16, (R, N), g).to(BF) if residual else None
    ref, _ = product(x, W, b, r)
    return dict(x=x.to(BF), W=W.to(BF), bias=b, res=r, ref=_exact("y", ref))


def exact_norm_rowgemm(R, N, norm, device, seed=0, bias=True, residual=False, groups=1):
    """Norm-fed mmfm_rowgemm / grouped forward.  LayerNorm: balanced_rows, x_hat = +-1 bit for bit.  ScaleNorm: x in {-1, 1}, ||x|| = 16,
    x_hat = +-1/16 exactly, and the gain 16 folds into integer prepared weights (mmfm_prep_weights with scalar_gain = 1).  W in
    {-1, 1} and integer biases: y = x . W^T + bias (+ res), sigma 16.  Returns the master weights W / gamma / bias per group (to be
    prepared by the kernel under test), what the preparation must produce (Wp, bp) and the references."""
    g = _gen(seed, device)
    x = (balanced_rows(R, g) if norm == 1 else _pm(1, (R, H), g))
    Ws = [_pm(1, (N, H), g).float() for _ in range(groups)]
    bs = [_ints(8, (N,), g).float() if bias else None for _ in range(groups)]
    r = _ints(16, (R, N), g).to(BF) if residual else None
    gain = 1.0 if norm == 1 else 16.0
    refs = [_exact("y", product(x, W, b, r)[0]) for W, b in zip(Ws, bs)]
    rstd = 1.0 / math.sqrt(1.0 + 1e-5) if norm == 1 else 1.0 / 16
    return dict(x=x.to(BF), Ws=Ws, gamma=None if norm == 1 else torch.tensor([gain], device=device), biases=bs, res=r,
                Wp=[_exact("Wp", f64(W) * gain) for W in Ws], xhat=(f64(x) / gain).to(BF), rstd=torch.full((R,), rstd, dtype=torch.float64, device=device),
                refs=refs)


def exact_mlp(R, device, seed=0, b_down=True):
    """The fused MLP with act = ReLU: x = balanced_rows (x_hat = +-1), W_up in {0, +-1} at density 1/16 (u: sigma 4) with integer
    b_up in [-2, 2], W_down in {0, +-1} at density 1/8 (64 terms of relu(u): sigma about 23) with integer b_down in [-4, 4], integer
    dy in {-2, -1, 1, 2}:
        u, g = relu(u), y = x + g . W_down^T + b_down, t1 = dy and du = (t1 . W_down) [u > 0] (32 terms: sigma 9) are exact integers.
    dx goes through the LayerNorm backward and is not exact: norm_bwd bounds it from the kernel's du."""
    g = _gen(seed, device)
    x = balanced_rows(R, g)
    Wu = _sparse_pm1(16, (INTER, H), g).float()
    bu = _ints(2, (INTER,), g).float()
    Wd = _sparse_pm1(8, (H, INTER), g).float()
    bd = _ints(4, (H,), g).float() if b_down else None
    dy = _pm(2, (R, H), g).to(BF)
    u, _ = product(x, Wu, bu)
    gg = act_f(ACT_RELU, u)
    y, _ = product(gg, Wd, bd, x)
    dg, _ = product(dy, Wd.T)
    _exact("u", u), _exact("t1 . W_down", dg)
    return dict(x=x.to(BF), Wu=Wu, bu=bu, Wd=Wd, bd=bd, dy=dy, xhat=x.to(BF), rstd=torch.full((R,), 1.0 / math.sqrt(1.0 + 1e-5), dtype=torch.float64, device=device),
                y=_exact("y", y), g=_exact("g", gg), du=_exact("du", dg * act_d1(ACT_RELU, u)))
