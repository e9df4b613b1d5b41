"""fp64 references, derived per-element bounds and structured inputs for the attention kernels (csrc/attention.hip, attention_bf16.hip,
attention_fast.hip, attention_long.hip), in the style of edge_refs.py and rowowner_refs.py.

Both references take the kernel's OWN inputs, upcast them to fp64 (exact for bf16 and fp32) and return fp64.  The backward reference is
handed the forward's STORED o and lse, which is the contract of mmfm_attn_desc (include/mmfm.h: "bwd: the forward's output"): P is
recomputed as exp(s - lse) and delta = rowsum(d_o * o) from the stored tensors, so one rounding chain separates kernel and reference.
tests/test_attn_refs_cpu.py proves both against fp64 autograd and proves that the bounds below accept an honest emulation of the kernels'
arithmetic and reject injected faults; tests/test_attention_elementwise_gpu.py compares the HIP kernels with them.

Tensors are [B, heads, L, dh] here (the GPU test packs them into the kernels' [B * L, ld] rows), `allowed` is bool [B, Lq, Lk]
(dropout_refs.allowed_mask), mult_p [B, heads, Lq, Lk] the drop_p multiplier (0 or 1 / keep) and mult_o [B, heads, Lq, dh] the drop_o one.

Bounds - derived, not tuned.  Every term is one rounding the kernels perform; u = 2^-24 (fp32), h = 2^-8 (half a bf16 ulp).
Two family groups:
  "f32"   fp32 compute: F32 and F32_TILED, on fp32 or bf16 storage (attention.hip: attn_fwd_kernel, attn_bwd_kernel and the tiled twins)
  "bf16"  bf16 MFMA: BF16, BF16_TILED (attention_bf16.hip), KEEPBIT_DH32 (attention_fast.hip), KEEPBIT_LONG (attention_long.hip)

  e_s  the exponent of a probability.  The score is an fp32 accumulation of dh products (exact bf16 x bf16 products on the MFMA, rounded
       fp32 ones in attention.hip, whose q is pre-scaled: attn_fwd_kernel "qreg[s] = ... * d.scale"): (dh + 2) u A, A = scale |q|.|k|.
       bf16 group: one fma(st, c2, -m) with c2 = fl(scale * log2 e) and m the reference exponent (fwd_tile in attention_bf16.hip,
       attention_fast.hip; the tile loop of attn_fwd_long_kernel): u (|s| + |m|) for the result, u |s| for c2, u |m| for m itself.
       |m| <= smax, the largest |s| over the row's allowed keys - NOT |s| at the row maximum: the keep-bit forwards hold the FIRST
       key tile's maximum as the reference exponent (attention_fast.hip "FAST PASS").  Then the exponential, exp_rel_err(s - m),
       |s - m| <= |s| + smax.  Forward:  e_p = u ((dh + 3) A + 2 |s| + 4 smax + 2) + exp_rel_err = u ((dh + 3) A + 4 |s| + 6 smax + 4).
       Backward: the exponent is fma(s, c2, -lse log2 e) (bwd_tile in attention_fast.hip, the phase kernels of attention_bf16.hip and
       attention_long.hip, "__expf(s[r] * d.scale - lse[q])" in attention.hip): the same with |lse| in the place of smax.
  o    sum_k bf16(p_k) v_k / l:
         h sum_k P|v|                            P packed to bf16 for the MFMA (pack2 in attn_common.h, called by fwd_tile of
                                                 attention_fast.hip / attention_long.hip; pack8(pd) in attention_bf16.hip) - bf16 group only
         sum_k P e_p |v| + |o| sum_k P e_p       the probabilities' own error, in the numerator and in l.  l sums the UNROUNDED
                                                 probabilities in every family ("ps0 = v_add(ps0, p0)" precedes pack2 in attention_fast.hip
                                                 fwd_tile; "ps += p0 + p1" precedes pd[] in attention_bf16.hip; "ps += p" in attention.hip),
                                                 so the packing adds no term to l
         2 n u sum_k P|v|, n = Lk + 3 ceil(Lk / 32) + 8
                                                 the fp32 accumulation of the numerator (Lk terms; online rescaling multiplies the tile
                                                 and l by alpha once per 32-key tile: 3 roundings per tile), of l, the division and the
                                                 dropout scale; |o| <= sum_k P|v| gives the factor 2
         h |o| resp. u |o|                       the stored output (bf16 or fp32)
  lse  m log 2 + log(l) in fp32 in every family (attention_fast.hip "m_ref * LN2 + __logf(l_tot)"): fp32 statistics of exact-product
       scores.  |log l| <= |lse| + smax:  u (4 |lse| + 8 smax + 2) + sum_k P e_p + Lk u.
  dv   sum_q bf16(p) dO: h sum_q P~|dO| (the packed probabilities, pack8(pd) / pack2(pm..) - bf16 group) + sum_q P~ e_p |dO| +
       (Lq + 8) u sum_q P~|dO| + the stored output.  P~ = P mult_p.
  dS   p (mult dP - delta) as one fma ("ds[e] = fmaf(pm, dpv[r], -v_mul(p, dq_[i]))"): both terms carry the same p, so its error is
       relative to dS itself: e_p |dS|; dP = dO.V and delta = dO.o are fp32 sums of dh exact products, delta from the STORED (bf16) o,
       as the reference's: (dh + 4) u P (|dO|.|V| + |dO|.|o|); packed to bf16 for both MFMAs (pack8(ds) / pack2(ds..)): h |dS|, bf16 group.
  dq   scale sum_k dS K: scale (sum_k E_dS |K| + (Lk + 8) u sum_k |dS||K|) + the stored output;  dk: the transposes, with Q and Lq.
With drop_o the bf16 kernels store dO' = dropout'(d_o) as bf16 (pack8(gd) in the backward prologues): h on dP's and dv's terms; without it
dO' = d_o exactly.
The half ulp of the stored value is taken of the computed value, not the reference: every e32 below carries the factor (1 + h).
An element whose magnitude sum is zero has bound zero: a key no query may attend to has dk = dv = 0 EXACTLY, and so has every element of
a disallowed pair in the single-pair read-outs."""
import math

import torch

import dropout_refs as DR
import edge_refs as ER
from edge_refs import HALF_ULP_BF16, U32, f64

GROUPS = ("f32", "bf16")


# ------------------------------------------------------------------------------------------------- references
def attn_fwd_ref(q, k, v, allowed, scale, mult_p=None, mult_o=None):
    """softmax((q k^T) scale | allowed) -> mult_p -> P v -> mult_o in fp64.  Returns a dict: o [B, h, Lq, dh], lse [B, h, Lq], and what the
    bounds need: abs_pv = sum_k P~|v| (|mult_o| applied), smax = max over the allowed keys of |s| (>= |s| at the row maximum, module
    docstring), the matrices P, Pt = P mult_p, s (unmasked) and A = scale |q|.|k|, and n = the number of allowed keys."""
    qd, kd, vd = f64(q), f64(k), f64(v)
    al = allowed[:, None]
    s = (qd @ kd.transpose(-1, -2)) * scale
    sm = s.masked_fill(~al, float("-inf"))
    lse = torch.logsumexp(sm, -1)
    P = torch.exp(sm - lse[..., None])
    Pt = P if mult_p is None else P * f64(mult_p)
    o, abs_pv = Pt @ vd, Pt @ vd.abs()
    if mult_o is not None:
        o, abs_pv = o * f64(mult_o), abs_pv * f64(mult_o).abs()
    return dict(o=o, lse=lse, abs_pv=abs_pv, smax=s.abs().masked_fill(~al, 0.0).amax(-1), P=P, Pt=Pt, s=s,
                A=(qd.abs() @ kd.abs().transpose(-1, -2)) * scale, n=allowed.sum(-1), v=vd, mult_o=mult_o)


def attn_bwd_ref(q, k, v, o, lse, d_o, allowed, scale, mult_p=None, mult_o=None):
    """The backward of include/mmfm.h from the kernel's own inputs and the forward's STORED o and lse, in fp64:
        P = exp(s - lse) | allowed;  dO' = d_o mult_o;  dP = dO' v^T;  delta = rowsum(d_o o);  dS = P (mult_p dP - delta)
        dq = scale dS k;  dk = scale dS^T q;  dv = (P mult_p)^T dO'
    Returns a dict with dq, dk, dv and the magnitudes of the module docstring: abs_dv = sum_q P~|dO'|; absS_k = sum_k |dS||k| and
    absP_k = sum_k P (|dO'|.|v| mult_p + |d_o|.|o|) |k| for dq; absS_q, absP_q = their transposes with |q| for dk; plus P, Pt, dS, s, A."""
    qd, kd, vd, od, gd = f64(q), f64(k), f64(v), f64(o), f64(d_o)
    al = allowed[:, None]
    s = (qd @ kd.transpose(-1, -2)) * scale
    P = torch.exp(s - f64(lse)[..., None]).masked_fill(~al, 0.0)
    mp = torch.ones((), dtype=torch.float64, device=P.device) if mult_p is None else f64(mult_p)
    ge = gd if mult_o is None else gd * f64(mult_o)
    Pt = P * mp
    dP = ge @ vd.transpose(-1, -2)
    delta = (gd * od).sum(-1, keepdim=True)
    dS = P * (mp * dP - delta)
    magP = P * mp * (ge.abs() @ vd.abs().transpose(-1, -2))
    mag = magP + P * (gd.abs() * od.abs()).sum(-1, keepdim=True)
    return dict(dq=scale * (dS @ kd), dk=scale * (dS.transpose(-1, -2) @ qd), dv=Pt.transpose(-1, -2) @ ge,
                abs_dv=Pt.transpose(-1, -2) @ ge.abs(), absS_k=dS.abs() @ kd.abs(), absP_k=mag @ kd.abs(),
                absS_q=dS.abs().transpose(-1, -2) @ qd.abs(), absP_q=mag.transpose(-1, -2) @ qd.abs(),
                P=P, Pt=Pt, dS=dS, mag=mag, magP=magP, dropped_o=mult_o is not None, s=s, A=(qd.abs() @ kd.abs().transpose(-1, -2)) * scale, lse=f64(lse), q=qd, k=kd, ge=ge)


# ------------------------------------------------------------------------------------------------- bounds (module docstring)
def _pack(group):
    assert group in GROUPS, group
    return HALF_ULP_BF16 if group == "bf16" else 0.0


def _e_p(A, s, ref_exp, dh):
    """Relative error of one probability: u ((dh + 3) A + 4 |s| + 6 |m| + 4), m = the reference exponent's magnitude [B, h, Lq]."""
    return U32 * ((dh + 3) * A + 4 * s.abs() + 6 * ref_exp[..., None] + 4)


def fwd_e32(f, group, dh):
    """(e32 of o, bound of lse) of a forward reference dict: everything but the stored output's own rounding."""
    Lk = f["s"].shape[-1]
    ep = _e_p(f["A"], f["s"], f["smax"], dh)
    n = Lk + 3 * math.ceil(Lk / 32) + 8
    num = (f["Pt"] * ep) @ f["v"].abs()
    if f["mult_o"] is not None:
        num = num * f64(f["mult_o"]).abs()
    rel_l = (f["P"] * ep).sum(-1)
    e_o = (1 + HALF_ULP_BF16) * (_pack(group) * f["abs_pv"] + num + f["o"].abs() * rel_l[..., None] + 2 * n * U32 * f["abs_pv"])
    e_lse = U32 * (4 * f["lse"].abs() + 8 * f["smax"] + 2) + rel_l + Lk * U32
    return e_o, e_lse


def bwd_e32(b, group, dh, scale):
    """(e32 of dq, dk, dv) of a backward reference dict."""
    Lq, Lk = b["s"].shape[-2:]
    ep = _e_p(b["A"], b["s"], b["lse"].abs(), dh)
    pk = _pack(group)
    po = pk if b["dropped_o"] else 0.0                         # dO' = dropout'(d_o) is stored as bf16 (pack8(gd)): exact without drop_o
    E = (ep + pk) * b["dS"].abs() + (dh + 4) * U32 * b["mag"] + po * b["magP"]      # per-pair error of dS as the MFMAs see it
    e_dq = scale * (E @ b["k"].abs() + (Lk + 8) * U32 * b["absS_k"])
    e_dk = scale * (E.transpose(-1, -2) @ b["q"].abs() + (Lq + 8) * U32 * b["absS_q"])
    e_dv = (pk + po + (Lq + 8) * U32) * b["abs_dv"] + (b["Pt"] * ep).transpose(-1, -2) @ b["ge"].abs()
    g = 1 + HALF_ULP_BF16
    return g * e_dq, g * e_dk, g * e_dv


def check_out(out, ref, e32, what):
    """One stored tensor against its reference: bf16 storage through edge_refs.check_bf16 (2^-8 |ref| + e32), fp32 storage against
    2^-24 |ref| + e32.  Every element is compared; a NaN on either side fails."""
    if out.dtype == torch.bfloat16:
        return ER.check_bf16(out, ref, e32, what)
    assert out.dtype == torch.float32, f"{what}: {out.dtype}"
    o = f64(out).reshape(ref.shape)
    err = (o - ref).abs()
    bad, ratio = ER._worst(err, U32 * ref.abs() + e32 + torch.zeros_like(ref))
    return ER._report(what, "fp32 bound 2^-24 |ref| + e32", bad, ratio, err, o, ref)


def check_all(out, q, k, v, d_o, allowed, scale, group, what, mult_p=None, mult_o=None, only=None):
    """out: dict of the kernel's o, lse and (when d_o is given) dq, dk, dv, each [B, h, L, dh] / [B, h, Lq] in the stored dtype.  Every element
    of every tensor against attn_fwd_ref / attn_bwd_ref (the latter fed out["o"], out["lse"]).  Returns {tensor: worst err / bound}."""
    dh = q.shape[-1]
    f = attn_fwd_ref(q, k, v, allowed, scale, mult_p, mult_o)
    e_o, e_lse = fwd_e32(f, group, dh)
    todo = [("o", f["o"], e_o), ("lse", f["lse"], e_lse)]
    if d_o is not None:
        b = attn_bwd_ref(q, k, v, out["o"], out["lse"], d_o, allowed, scale, mult_p, mult_o)
        e_dq, e_dk, e_dv = bwd_e32(b, group, dh, scale)
        todo += [("dq", b["dq"], e_dq), ("dk", b["dk"], e_dk), ("dv", b["dv"], e_dv)]
    ratios = {}
    for name, ref, e32 in todo:
        if only is not None and name not in only:
            continue
        if name == "lse":
            assert out["lse"].dtype == torch.float32
            o = f64(out["lse"])
            err = (o - ref).abs()
            bad, ratio = ER._worst(err, e32)
            ratios[name] = ER._report(f"{what} lse", "fp32 statistics bound", bad, ratio, err, o, ref)
        else:
            ratios[name] = check_out(out[name], ref, e32, f"{what} {name}")
    return ratios


def assert_written(t, what):
    """Outputs start as NaN sentinels: none may be left (a store that was dropped)."""
    n = int(torch.isnan(t).sum())
    assert n == 0, f"{what}: {n} of {t.numel()} elements never written"


# ------------------------------------------------------------------------------------------------- the old criterion (for the pin)
def old_criterion_fraction(out, ref, tol):
    """max|err| / (tol max|ref|): the criterion of test_attention_masks_gpu.py (close_bf16); <= 1 passes."""
    a, b = out.float(), ref.float()
    return float((a - b).abs().max()) / (tol * (float(b.abs().max()) + 1e-6))


# ------------------------------------------------------------------------------------------------- mod_id and key-padding recipes
MOD_RECIPES = ("inside", "aligned", "blocks32", "mod3", "ragged_last")
PAD_RECIPES = ("tile_start", "tile_end", "full_tile", "last5", "headpad")


def mod_id(L, recipe):
    """uint8 [L].  inside: two modalities, boundary inside a 32-tile; aligned: boundary on a multiple of 32 (uniform tiles: T_ZERO from two
    different uniform tiles, T_BIAS from two equal ones; L <= 32 has no such boundary: one modality, SEP adds nothing); blocks32: the
    modality alternates every 32 positions (equal modalities in non-adjacent tiles); mod3: t % 3 (every tile mixed); ragged_last: only
    the positions of the ragged last tile carry another modality (a uniform ragged tile; positions beyond L repeat the last byte)."""
    t = torch.arange(L)
    if recipe == "inside":
        b = L // 2 + (5 if (L // 2) % 32 == 0 and L > 10 else 0)
        assert L < 2 or b % 32 != 0
        m = t >= b
    elif recipe == "aligned":
        b = 32 * max(1, (L // 2) // 32)
        m = t >= b
    elif recipe == "blocks32":
        m = (t // 32) % 2
    elif recipe == "mod3":
        m = t % 3
    elif recipe == "ragged_last":
        m = t >= 32 * ((L - 1) // 32)
    else:
        raise ValueError(recipe)
    return m.to(torch.uint8)


def keypad(B, Lk, recipe):
    """uint8 [B, Lk], 0 = padded.  Sample 0 carries the recipe, the last sample a different single padded key, the middle ones none.
    tile_start / tile_end: a padded key at the start / end of a 32-key tile; full_tile: one fully padded tile; last5: the last 5 keys
    (inside the last ragged 8-key group); headpad: the first 40 keys (test_attention_masks_gpu.py; meant for SEP)."""
    kp = torch.ones(B, Lk, dtype=torch.uint8)
    last = 32 * ((Lk - 1) // 32)
    if recipe == "tile_start":
        kp[0, last] = 0
        if Lk > 64:
            kp[0, 32] = 0
    elif recipe == "tile_end":
        kp[0, 31 if Lk > 32 else Lk - 1] = 0
        if Lk > 64:
            kp[0, 63] = 0
    elif recipe == "full_tile":
        if Lk >= 96:
            kp[0, 32:64] = 0
        elif Lk > 32:
            kp[0, :32] = 0
        else:
            kp[0, :Lk - 1] = 0
    elif recipe == "last5":
        kp[0, Lk - 5:] = 0
    elif recipe == "headpad":
        kp[0, :min(40, Lk // 2)] = 0
    else:
        raise ValueError(recipe)
    if B > 1:
        kp[B - 1, min(5, Lk - 1)] = 0 if Lk > 1 else 1
    return kp


def build_allowed(kp, flags, Lq, mod=None):
    """dropout_refs.allowed_mask, asserting that every query keeps an allowed key (no case builds a row of NaNs)."""
    al = DR.allowed_mask(kp, flags, Lq, mod)
    assert bool(al.any(-1).all()), "a query row without an allowed key"
    return al


# ------------------------------------------------------------------------------------------------- random inputs
def random_inputs(B, heads, Lq, Lk, dh, dtype, device="cpu"):
    """The inputs of test_attention_masks_gpu.py (late keys x 6: late queries exceed the first key tile's reference exponent), and in sample 1
    instead the FIRST key tile x 6: the first tile then holds the row maxima, the exponent the keep-bit forwards keep as their reference."""
    g = lambda seed, L: torch.randn(B, heads, L, dh, generator=torch.Generator().manual_seed(seed))
    q, k, v, d_o = g(1, Lq), g(2, Lk), g(4, Lk), g(3, Lq)
    k[:, :, (3 * Lk) // 4:] *= 6.0
    if B > 1:
        k[1, :, (3 * Lk) // 4:] /= 6.0
        k[1, :, :min(32, Lk)] *= 6.0
    return [t.to(dtype).to(device) for t in (q, k, v, d_o)]


def random_combos(Lq, Lk):
    """(flags, mod recipe) of the random-input checks: flags {0, 1, 2, 5, 7} with the recipes aligned / blocks32 / inside under SEP; flags 0
    on cross shapes (DIAG / CAUSAL / SEP need Lq == Lk); flags 0 and 4 at L = 1100."""
    if Lq != Lk:
        return [(0, None)]
    if Lq >= 1000:
        return [(0, None), (4, "aligned")]
    return [(0, None), (1, None), (2, None)] + [(f, r) for f in (5, 7) for r in ("aligned", "blocks32", "inside")]


# ------------------------------------------------------------------------------------------------- single-pair inputs (mask read-out)
def sgn(L):
    """+1 where (7 k mod 5) < 2, else -1."""
    return torch.where((7 * torch.arange(L)) % 5 < 2, 1.0, -1.0)


def readout_inputs(which, B, heads, Lq, Lk, dh, dtype, device="cpu"):
    """Stacked single-pair inputs q, k, v, d_o, each [nblk, B, heads, L, dh]; scale = dh^-0.5 and S == 0, so P = allowed / n(q).  Every value
    is 0 or +-1: exact in bf16.
      "o_dv": Q = K = 0, V[k, c] = 1 iff k == k0 + c, dO[q, c] = 1 iff q == q0 + c:   o[q, c] = allowed(q, k0 + c) / n(q), lse = ln n(q),
              dv[k, c] = allowed(q0 + c, k) / n(q0 + c)
      "dq":   Q = 0, K[k, c] = 1 iff k == k0 + c, V[k, 0] = sgn(k), dO = e_0:          dq[q, c] = scale dS[q, k0 + c]
      "dk":   Q[q, c] = 1 iff q == q0 + c, K = 0, the same V and dO:                   dk[k, c] = scale dS[q0 + c, k]
    with dS = P (sgn_k - sum_k' P sgn_k')."""
    nq, nk = math.ceil(Lq / dh), math.ceil(Lk / dh)
    nblk = {"o_dv": max(nq, nk), "dq": nk, "dk": nq}[which]
    z = lambda L: torch.zeros(nblk, B, heads, L, dh)
    q, k, v, d_o = z(Lq), z(Lk), z(Lk), z(Lq)

    def onehot(t, L):
        for j in range(nblk):
            n = max(0, min(dh, L - j * dh))
            if n:
                t[j, :, :, j * dh + torch.arange(n), torch.arange(n)] = 1.0
    if which == "o_dv":
        onehot(v, Lk)
        onehot(d_o, Lq)
    else:
        onehot(k if which == "dq" else q, Lk if which == "dq" else Lq)
        v[..., 0] = sgn(Lk)
        d_o[..., 0] = 1.0
    return [t.to(dtype).to(device) for t in (q, k, v, d_o)]


REF_ELEMS = 4e7            # [launches * B, heads, Lq, Lk] elements of one stacked reference evaluation


def _pairs(x, n_other):
    """[nblk, B, h, L, dh] -> [B, h, L, n_other]: column j dh + c of row r = x[j, :, :, r, c]."""
    nblk, B, h, L, dh = x.shape
    return x.permute(1, 2, 3, 0, 4).reshape(B, h, L, nblk * dh)[..., :n_other]


def readout(run, allowed, B, heads, Lq, Lk, dh, dtype, group, what, tensors=("o_dv", "dq", "dk"), device="cpu"):
    """The mask read-out of a launcher `run(q, k, v, d_o) -> dict(o, lse, dq, dk, dv[, mult_p])`: ceil(L / dh) launches per tensor show every
    (q, k) pair.  Asserts that o and dv are nonzero EXACTLY where allowed (& keep, when the launcher drops probabilities and hands back
    its multiplier) holds, that dq and dk are exactly 0 where it does not, and every value (and lse against ln n(q)) against the
    per-element bounds.  Returns {tensor: worst err / bound}."""
    scale = dh ** -0.5
    al = allowed[:, None].expand(B, heads, Lq, Lk)
    worst = {}
    for which in tensors:
        q, k, v, d_o = readout_inputs(which, B, heads, Lq, Lk, dh, dtype, device)
        nblk = q.shape[0]
        outs = [run(q[j], k[j], v[j], d_o[j]) for j in range(nblk)]
        mult_p = outs[0].get("mult_p")
        want = al if mult_p is None else al & (mult_p != 0)
        st = {n: torch.stack([o_[n] for o_ in outs]) for n in ("o", "lse", "dq", "dk", "dv")}
        if which == "o_dv":
            got_o = _pairs(st["o"], Lk) != 0
            got_dv = (_pairs(st["dv"], Lq) != 0).transpose(-1, -2)
            for name, got in (("o", got_o), ("dv", got_dv)):
                ne = got != want
                if ne.any():
                    b, h, qi, ki = [int(i) for i in torch.nonzero(ne)[0]]
                    raise AssertionError(f"{what}: {name} read-out differs from the mask rule at {int(ne.sum())} pairs; first (b {b}, head {h}, q {qi}, "
                                         f"k {ki}): kernel {'attends' if bool(got[b, h, qi, ki]) else 'does not attend'}, rule says {bool(want[b, h, qi, ki])}")
        else:
            got = _pairs(st[which], Lk if which == "dq" else Lq)
            if which == "dk":
                got = got.transpose(-1, -2)
            leak = (got != 0) & ~al
            if leak.any():
                b, h, qi, ki = [int(i) for i in torch.nonzero(leak)[0]]
                raise AssertionError(f"{what}: {which} read-out is nonzero at {int(leak.sum())} disallowed pairs; first (b {b}, head {h}, q {qi}, k {ki})")
        # the values, in chunks of launches that keep the stacked fp64 matrices of the reference small
        step = max(1, int(REF_ELEMS // (B * heads * Lq * Lk)))
        for j0 in range(0, nblk, step):
            j1 = min(nblk, j0 + step)
            flat = lambda t: t[j0:j1].reshape((j1 - j0) * B, *t.shape[2:])
            r = check_all({n: flat(t) for n, t in st.items()}, flat(q), flat(k), flat(v), flat(d_o), allowed.repeat(j1 - j0, 1, 1), scale, group,
                          f"{what} read-out {which}", mult_p=None if mult_p is None else mult_p.repeat(j1 - j0, 1, 1, 1))
            for n, x in r.items():
                worst[n] = max(worst.get(n, 0.0), x)
    return worst


# ------------------------------------------------------------------------------------------------- launch shapes
# (family, dtype, dh, workspace, [L or (Lq, Lk)], why).  Thresholds, read off the launchers (multi_modal_foundation_model_amd/csrc):
#   KEEPBIT_DH32  attention_fast.hip mmfm_attn_fast_takes (:764): dh 32, Lq / Lk % 8 == 0, nqt <= 8, nkt <= 7 (B_CW), nkt <= nqt;
#                 mmfm_attn_fast_launch (:786): nw = 4 for nqt <= 4, 7 for nqt == 7, 6 for nqt 5 / 6, else 8; (:797) the nkt == 7
#                 instantiations at nw >= 7; (:815) the NQT = 7 backward
#   KEEPBIT_LONG  attention_long.hip mmfm_attn_long_takes (:735): dh 64 / 128, workspace, Lq / Lk % 8 == 0; mmfm_attn_long_launch (:773, :783,
#                 :788): F_NW / Q_NW = 8 query tiles per forward / dQ workgroup (256 queries), K_NW = 4 key tiles per dK-dV workgroup
#                 (128 keys), CH = 128-row chunks
#   BF16          attention_bf16.hip mmfm_attn_bf16_takes (:1212): dh 16 / 32 / 64 whose images fit fwd_lds / bwd_lds (:1197, :1201);
#                 fwd_waves_for (:1191): 8 waves from Lq >= 160; bwd1_ok (:790): the single-pass backward while LkP <= 32 * BW1_CW and
#                 LkP <= LqP and the K image fits the staging tiles, else the two-phase pair
#   BF16_TILED    attention_bf16.hip (:1217): dh 128 always, or a head that does not fit; TCH16 = 128-row chunks
#   F32 / _TILED  attention.hip attn_route (:877): fp32 storage, or bf16 storage at dh 8; tiled when fwd_lds_bytes / bwd_lds_bytes pass 160 KB
# The family (and BWD_SINGLE) of every entry is ASSERTED at launch through ops.attn_family, so a threshold that moves fails loudly.
SHAPES = [
    ("KEEPBIT_DH32", "bf16", 32, False, [8, 40, 136, 168, 200, 224, (256, 224), (72, 40)],
     "1 tile; ragged; nqt 5 / 6 -> 6 waves; nqt 7 -> the 7-tile specialisation; nqt 8 / nkt 7 -> 8 waves"),
    ("KEEPBIT_LONG", "bf16", 64, True, [8, 40, 136, 264, 600, (72, 136), (40, 24), (264, 40)],
     "one past the 128-row chunk; one past the 256 queries of an 8-wave workgroup / the 128 keys of a dK-dV workgroup"),
    ("KEEPBIT_LONG", "bf16", 128, True, [8, 40, 136, 264, (72, 136), (40, 24), (264, 40)], "the same at dh 128"),
    ("BF16", "bf16", 16, False, [33, 70, 129, 161, (40, 72), (72, 40)], "L % 8 != 0; the 8-wave forward from 160"),
    ("BF16", "bf16", 32, False, [33, 70, 129, 161, 250, (40, 72)], "nkt 8; (72, 40) belongs to KEEPBIT_DH32 at dh 32"),
    ("BF16", "bf16", 64, False, [33, 70, 129, 161, (40, 72), (72, 40)], "two-phase vs single-pass backward"),
    ("BF16_TILED", "bf16", 128, False, [40, 129, 200], "chunk of 128; ragged"),
    ("BF16_TILED", "bf16", 64, False, [460], "a head that does not fit LDS"),
    ("BF16_TILED", "bf16", 32, False, [1100], "flags 0 and 4 only"),
    ("F32", "bf16", 8, False, [16], "fp32 compute on bf16 storage"),
    ("F32", "f32", 32, False, [70, 330], ""),
    ("F32", "f32", 64, False, [100, 600], ""),
    ("F32", "f32", 128, False, [40, 200, (40, 700)], ""),
]


# entries above that run the tiled fp32 kernels, and BF16 entries whose backward is the two-phase pair (the others: BWD_SINGLE)
F32_TILED = {("f32", 32, 330), ("f32", 64, 600), ("f32", 128, 200), ("f32", 128, (40, 700))}
BF16_TWO_PHASE = {(32, 250), (16, (40, 72)), (32, (40, 72)), (64, (40, 72))}


def expected_family(fam, dt, dh, shape):
    """(family name, backward on the single-pass kernel) of a SHAPES entry's shape."""
    if fam == "F32" and (dt, dh, shape) in F32_TILED:
        return "F32_TILED", False
    return fam, fam == "BF16" and (dh, shape) not in BF16_TWO_PHASE


def group_of(family):
    return "f32" if family.startswith("F32") else "bf16"
