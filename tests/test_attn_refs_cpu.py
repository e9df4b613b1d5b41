"""Proves the tools of attn_refs.py without a GPU.

1. attn_fwd_ref / attn_bwd_ref against fp64 autograd of softmax attention: all 8 flag combinations, cross shapes, both dropouts.
2. A torch emulation of the kernels' honest arithmetic (fp32; 32-key tiles with online rescaling; in the bf16 group P and dS rounded to
   bf16 where the kernels pack them, bf16 output) passes every bound on the GPU test's random inputs and on the read-outs; its worst
   err / bound is printed (DESIGN.md records it).
3. The same emulation with ONE fault injected is rejected.  FAULTS states which tool catches which fault: "bounds" = check_all on the
   random inputs, "readout" = the single-pair mask read-out.
4. The regression pin of the finding that motivated this file: three single-pair mask faults pass the old `tol * max|ref|` criterion
   of test_attention_masks_gpu.py on that test's inputs and fail the new tools."""
import math

import pytest
import torch

import attn_refs as AR
import dropout_refs as DR
from edge_refs import f64

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------- 1. references vs autograd
def _autograd(q, k, v, d_o, allowed, scale, mult_p, mult_o):
    B, h, Lq, dh = q.shape
    qr, kr, vr = [f64(t).clone().requires_grad_(True) for t in (q, k, v)]
    mo = None if mult_o is None else mult_o.transpose(1, 2).reshape(B * Lq, h * dh)
    o, lse = DR.attention_dropout_ref(qr, kr, vr, allowed, scale, mult_p, mo)
    o.backward(f64(d_o).transpose(1, 2).reshape(B * Lq, h * dh))
    return o.detach().view(B, Lq, h, dh).transpose(1, 2), lse.detach(), qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("drop", [False, True])
def test_refs_match_fp64_autograd(flags, drop):
    B, h, L, dh = 2, 2, 72, 16
    q, k, v, d_o = AR.random_inputs(B, h, L, L, dh, torch.float32)
    al = AR.build_allowed(AR.keypad(B, L, "tile_end"), flags, L, AR.mod_id(L, "inside"))
    g = torch.Generator().manual_seed(5)
    mult_p = (torch.rand(B, h, L, L, generator=g) < 0.6).double() / 0.6 if drop else None
    mult_o = (torch.rand(B, h, L, dh, generator=g) < 0.8).double() / 0.8 if drop else None
    scale = dh ** -0.5
    o, lse, dq, dk, dv = _autograd(q, k, v, d_o, al, scale, mult_p, mult_o)
    f = AR.attn_fwd_ref(q, k, v, al, scale, mult_p, mult_o)
    b = AR.attn_bwd_ref(q, k, v, f["o"], f["lse"], d_o, al, scale, mult_p, mult_o)
    for name, got, want in (("o", f["o"], o), ("lse", f["lse"], lse), ("dq", b["dq"], dq), ("dk", b["dk"], dk), ("dv", b["dv"], dv)):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-12 * float(want.abs().max())), f"{name}: {(got - want).abs().max():.3e}"    # fp64: ~1e3 terms at 1.1e-16 each
    # the magnitudes dominate what they bound
    assert bool((f["abs_pv"] >= f["o"].abs() * (1 - 1e-12)).all()) and bool((b["abs_dv"] >= b["dv"].abs() * (1 - 1e-12)).all())
    assert bool((scale * b["absS_k"] >= b["dq"].abs() * (1 - 1e-12)).all()) and bool((scale * b["absS_q"] >= b["dk"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("Lq,Lk", [(40, 72), (72, 40), (8, 136)])
def test_refs_match_fp64_autograd_cross(Lq, Lk):
    B, h, dh = 2, 3, 8
    q, k, v, d_o = AR.random_inputs(B, h, Lq, Lk, dh, torch.float32)
    al = AR.build_allowed(AR.keypad(B, Lk, "last5"), 0, Lq)
    scale = dh ** -0.5
    o, lse, dq, dk, dv = _autograd(q, k, v, d_o, al, scale, None, None)
    f = AR.attn_fwd_ref(q, k, v, al, scale)
    b = AR.attn_bwd_ref(q, k, v, f["o"], f["lse"], d_o, al, scale)
    for name, got, want in (("o", f["o"], o), ("lse", f["lse"], lse), ("dq", b["dq"], dq), ("dk", b["dk"], dk), ("dv", b["dv"], dv)):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-12 * float(want.abs().max())), f"{name}: {(got - want).abs().max():.3e}"    # fp64: ~1e3 terms at 1.1e-16 each
    pad = ~AR.keypad(B, Lk, "last5").bool()
    assert bool((b["dk"][pad[:, None].expand(B, h, Lk)] == 0).all()) and bool((b["dv"][pad[:, None].expand(B, h, Lk)] == 0).all())


def test_readout_identities_fp64():
    """The single-pair inputs read out what their docstring says, in fp64, with every allowed pair's dS nonzero (L = 72, CAUSAL | SEP)."""
    B, h, L, dh = 1, 1, 72, 16
    al = AR.build_allowed(AR.keypad(B, L, "tile_end"), 6, L, AR.mod_id(L, "inside"))
    scale = dh ** -0.5
    n = al.sum(-1).double()
    P = al.double() / n[..., None]
    dS = P * (AR.sgn(L).double()[None, None, :] - (P * AR.sgn(L).double()).sum(-1, keepdim=True))
    assert bool((dS[al] != 0).all())
    for which in ("o_dv", "dq", "dk"):
        q, k, v, d_o = AR.readout_inputs(which, B, h, L, L, dh, torch.float64)
        nblk = q.shape[0]
        fl = lambda t: t.reshape(nblk * B, *t.shape[2:])
        f = AR.attn_fwd_ref(fl(q), fl(k), fl(v), al.repeat(nblk, 1, 1), scale)
        b = AR.attn_bwd_ref(fl(q), fl(k), fl(v), f["o"], f["lse"], fl(d_o), al.repeat(nblk, 1, 1), scale)
        un = lambda t: t.reshape(nblk, B, *t.shape[1:])
        if which == "o_dv":
            assert torch.allclose(AR._pairs(un(f["o"]), L)[:, 0], P, atol=1e-15)
            assert torch.allclose(AR._pairs(un(b["dv"]), L)[:, 0].transpose(-1, -2), P, atol=1e-15)
            assert torch.allclose(f["lse"][0, 0], n[0].log(), atol=1e-14)
        elif which == "dq":
            assert torch.allclose(AR._pairs(un(b["dq"]), L)[:, 0], scale * dS, atol=1e-15)
        else:
            assert torch.allclose(AR._pairs(un(b["dk"]), L)[:, 0].transpose(-1, -2), scale * dS, atol=1e-15)


# ------------------------------------------------------------------------------------------------- 2. the honest emulation
LOG2E = 1.4426950408889634


def emulate(q, k, v, d_o, allowed, scale, group, mult_p=None, mult_o=None, fault=None):
    """The kernels' arithmetic in torch fp32 on the CPU.  Forward: 32-key tiles, online rescaling, l from the unrounded probabilities, P
    rounded to bf16 in front of P.V (bf16 group), o in the storage dtype.  Backward from the STORED o and lse: p = exp(s - lse),
    dS = p (keep dP - delta / ks) rounded to bf16 (bf16 group), delta from the stored o, dk / dq scaled when stored.
    fault: None, or one of the arithmetic faults of FAULTS."""
    pack = (lambda t: t.to(BF).float()) if group == "bf16" else (lambda t: t)
    out_dt = q.dtype
    B, h, Lq, dh = q.shape
    Lk = k.shape[2]
    qf, kf, vf, gf = [t.float() for t in (q, k, v, d_o)]
    al = allowed[:, None].expand(B, h, Lq, Lk)
    keep = torch.ones(B, h, Lq, Lk) if mult_p is None else (mult_p != 0).float()
    ks = 1.0 if mult_p is None else float(mult_p.max())
    s = (qf @ kf.transpose(-1, -2)) * torch.tensor(scale, dtype=torch.float32)
    m_run = torch.full((B, h, Lq), float("-inf"))
    l_run = torch.zeros(B, h, Lq)
    acc = torch.zeros(B, h, Lq, dh)
    nkt = math.ceil(Lk / 32)
    for kt in range(nkt):
        sl = slice(32 * kt, min(Lk, 32 * kt + 32))
        st = s[..., sl].masked_fill(~al[..., sl], float("-inf"))
        m_new = torch.maximum(m_run, st.amax(-1))
        m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.where(torch.isinf(m_run), torch.zeros_like(m_run), torch.exp(m_run - m_use))
        p = torch.exp(st - m_use[..., None])
        l_run = l_run * alpha + p.sum(-1)
        if not (fault == "skip_rescale" and kt == nkt - 1):
            acc = acc * alpha[..., None]
        acc = acc + pack(p * keep[..., sl]) @ vf[:, :, sl]
        m_run = m_new
    o_pre = acc * (ks / l_run)[..., None]
    o = (o_pre if mult_o is None else o_pre * mult_o.float()).to(out_dt)
    lse = (torch.log(l_run) if fault == "lse_no_max" else m_run + torch.log(l_run))
    if fault == "dropped_store":
        o[0, 0, 8:16] = float("nan")
    # backward
    p = torch.exp(s - lse[..., None]).masked_fill(~al, 0.0)
    ge = gf if mult_o is None else pack(gf * mult_o.float())          # dO' = dropout'(d_o): stored as bf16 by the bf16 kernels only
    dP = ge @ vf.transpose(-1, -2)
    o_delta = o_pre.to(out_dt).float() if fault == "delta_undropped" else o.float()
    delta = (gf * o_delta).sum(-1, keepdim=True) / ks
    pm = pack(p * keep)
    ds = pack(p * (keep * dP - delta))
    dk_acc, dv_acc = ds.transpose(-1, -2) @ qf, pm.transpose(-1, -2) @ ge
    if fault == "ragged_rows" and Lq % 32:
        # the rows q >= Lq of the ragged last query tile, holding a copy of the last real row, are not masked out of dK / dV
        n = 32 - Lq % 32
        dk_acc = dk_acc + n * ds[:, :, -1:, :].transpose(-1, -2) @ qf[:, :, -1:]
        dv_acc = dv_acc + n * pm[:, :, -1:, :].transpose(-1, -2) @ ge[:, :, -1:]
    sc = torch.tensor(scale * ks, dtype=torch.float32)
    dq = ((ds @ kf) * sc).to(out_dt)
    dk = (dk_acc * (torch.tensor(ks, dtype=torch.float32) if fault == "dk_no_scale" else sc)).to(out_dt)
    dv = (dv_acc * ks).to(out_dt)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _cases():
    i = 0
    for fam, dt, dh, ws, shapes, _ in AR.SHAPES:
        for sh in shapes:
            Lq, Lk = (sh, sh) if isinstance(sh, int) else sh
            yield fam, dt, dh, Lq, Lk, i
            i += 1


EMU_WORST = {}


@pytest.mark.parametrize("fam,dt,dh,Lq,Lk,i", list(_cases()))
def test_honest_emulation_inside_every_bound(fam, dt, dh, Lq, Lk, i):
    B, h = 3, 3
    dtype = BF if dt == "bf16" else torch.float32
    group = AR.group_of(fam)
    q, k, v, d_o = AR.random_inputs(B, h, Lq, Lk, dh, dtype)
    scale = dh ** -0.5
    for j, (flags, rec) in enumerate(AR.random_combos(Lq, Lk)):         # the GPU test's own cases, key padding included
        mod = AR.mod_id(Lq, rec) if rec else None
        al = AR.build_allowed(AR.keypad(B, Lk, AR.PAD_RECIPES[j % 4]), flags, Lq, mod)
        out = emulate(q, k, v, d_o, al, scale, group)
        r = AR.check_all(out, q, k, v, d_o, al, scale, group, f"emulation {fam} dh {dh} L {Lq}x{Lk} flags {flags} {rec}")
        for n, x in r.items():
            EMU_WORST[(group, n)] = max(EMU_WORST.get((group, n), 0.0), x)
    print("[attn] emulation worst err / bound so far:", {f"{g} {n}": f"{x:.3f}" for (g, n), x in sorted(EMU_WORST.items())})


@pytest.mark.parametrize("group,dtype", [("bf16", BF), ("f32", torch.float32), ("f32", BF)])
def test_honest_emulation_passes_readout_and_dropout(group, dtype):
    B, h, L, dh = 3, 3, 72, 32
    for flags, rec, pad in [(0, None, "last5"), (5, "aligned", "tile_start"), (6, "blocks32", "full_tile"), (7, "ragged_last", "headpad"), (3, None, "tile_end")]:
        mod = AR.mod_id(L, rec) if rec else None
        al = AR.build_allowed(AR.keypad(B, L, pad), flags, L, mod)
        run = lambda q, k, v, g: emulate(q, k, v, g, al, dh ** -0.5, group)
        AR.readout(run, al, B, h, L, L, dh, dtype, group, f"emulation {group} flags {flags}")
    # both dropouts, on random inputs and on the read-out (nonzero exactly where allowed & keep)
    g = torch.Generator().manual_seed(7)
    mult_p = (torch.rand(B, h, L, L, generator=g) < 0.6).float() / 0.6
    mult_o = (torch.rand(B, h, L, dh, generator=g) < 0.8).float() / 0.8
    al = AR.build_allowed(AR.keypad(B, L, "last5"), 5, L, AR.mod_id(L, "inside"))
    q, k, v, d_o = AR.random_inputs(B, h, L, L, dh, dtype)
    out = emulate(q, k, v, d_o, al, dh ** -0.5, group, mult_p, mult_o)
    AR.check_all(out, q, k, v, d_o, al, dh ** -0.5, group, f"emulation {group} dropout", mult_p=mult_p, mult_o=mult_o)
    run = lambda q, k, v, g: dict(emulate(q, k, v, g, al, dh ** -0.5, group, mult_p), mult_p=mult_p)
    AR.readout(run, al, B, h, L, L, dh, dtype, group, f"emulation {group} drop_p", tensors=("o_dv",))


# ------------------------------------------------------------------------------------------------- 3. injected faults
def _rule(kp, flags, L, mod):
    return DR.allowed_mask(kp, flags, L, mod)


def _f_pad_last_group(kp, flags, L, mod):
    al = _rule(kp, flags, L, mod).clone()
    k = torch.arange(L) >= 8 * ((L - 1) // 8)
    al[:, :, k] = True                                      # the whole last 8-key group, padded keys included
    return al


def _f_diag_skip_padded(kp, flags, L, mod):
    return _rule(kp, flags & ~1, L, mod) | (torch.eye(L, dtype=torch.bool)[None] & kp.bool()[:, None, :])


def _f_causal_strict(kp, flags, L, mod):
    c = torch.tril(torch.ones(L, L, dtype=torch.bool), -1)
    c[0, 0] = True
    return _rule(torch.zeros_like(kp), flags & ~2, L, mod) | c[None]          # the DIAG and SEP terms of the rule, and k < q


def _f_causal_keypad(kp, flags, L, mod):
    return _rule(torch.zeros_like(kp), flags & ~2, L, mod) | (torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & kp.bool()[:, None, :])


def _f_sep_tile_first(kp, flags, L, mod):
    mk = mod[32 * (torch.arange(L) // 32)]
    return _rule(kp, flags & ~4, L, mod) | (mod[None, :, None] != mk[None, None, :])


def _f_sep_off_by_one(kp, flags, L, mod):
    m = mod.clone()
    m[int((mod != mod[0]).nonzero()[0])] = mod[0]            # the first modality boundary, one position late
    return _rule(kp, flags, L, m)


def _f_one_pair(kp, flags, L, mod):
    al = _rule(kp, flags, L, mod).clone()
    b, q, k = [int(i) for i in torch.nonzero(~al)[-1]]      # the last disallowed pair: a late query (peaked by the x 6 keys)
    al[b, q, k] = True
    return al


# fault -> (flags, mod recipe, pad recipe, mask fault function or None, arithmetic fault or None, tools that must catch it)
FAULTS = {
    "a padded key admitted in the last ragged 8-key group": (0, None, "last5", _f_pad_last_group, None, {"bounds", "readout"}),
    "DIAG not applied to a padded key": (5, "inside", "tile_start", _f_diag_skip_padded, None, {"bounds", "readout"}),
    "CAUSAL evaluated as k < q away from row 0": (2, None, "tile_end", _f_causal_strict, None, {"bounds", "readout"}),
    "CAUSAL honouring the key padding": (6, "inside", "tile_end", _f_causal_keypad, None, {"bounds", "readout"}),
    "SEP read from the tile's first position": (6, "inside", "last5", _f_sep_tile_first, None, {"bounds", "readout"}),
    "SEP boundary off by one": (4, "inside", "last5", _f_sep_off_by_one, None, {"bounds", "readout"}),
    "one (q, k) pair admitted in a peaked row": (6, "inside", "last5", _f_one_pair, None, {"readout"}),
    "one tile's online rescale skipped": (0, None, "last5", None, "skip_rescale", {"bounds"}),
    "lse without the running maximum": (0, None, "last5", None, "lse_no_max", {"bounds"}),
    "delta taken from the un-dropped output": (0, None, "last5", None, "delta_undropped", {"bounds"}),
    "scale missing from dk": (0, None, "last5", None, "dk_no_scale", {"bounds", "readout"}),
    "rows q >= Lq of a ragged query tile contributing to dk / dv": (0, None, "last5", None, "ragged_rows", {"bounds", "readout"}),
    "one dropped 8-row store": (0, None, "last5", None, "dropped_store", {"bounds", "readout"}),
}


def _rejects(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", list(FAULTS))
@pytest.mark.parametrize("group", ["bf16", "f32"])
def test_injected_fault_is_rejected(name, group):
    flags, rec, pad, maskf, arith, tools = FAULTS[name]
    B, h, L, dh = 3, 3, 72, 32
    dtype = BF if group == "bf16" else torch.float32
    scale = dh ** -0.5
    kp = AR.keypad(B, L, pad)
    mod = AR.mod_id(L, rec) if rec else None
    al = AR.build_allowed(kp, flags, L, mod)
    bad_al = maskf(kp, flags, L, mod) if maskf else al
    assert maskf is None or bool((bad_al != al).any()), "the fault changes nothing on this case"
    assert bool(bad_al.any(-1).all())
    mult_o = None
    if arith == "delta_undropped":
        mult_o = (torch.rand(B, h, L, dh, generator=torch.Generator().manual_seed(9)) < 0.8).float() / 0.8
    q, k, v, d_o = AR.random_inputs(B, h, L, L, dh, dtype)
    # the honest emulation passes this very case ...
    AR.check_all(emulate(q, k, v, d_o, al, scale, group, mult_o=mult_o), q, k, v, d_o, al, scale, group, "honest", mult_o=mult_o)
    # ... and each tool the table names rejects the faulty one
    caught = set()
    if _rejects(lambda: AR.check_all(emulate(q, k, v, d_o, bad_al, scale, group, mult_o=mult_o, fault=arith), q, k, v, d_o, al, scale, group,
                                     name, mult_o=mult_o)):
        caught.add("bounds")
    if mult_o is None:
        run = lambda q_, k_, v_, g_: emulate(q_, k_, v_, g_, bad_al, scale, group, fault=arith)
        if _rejects(lambda: AR.readout(run, al, B, h, L, L, dh, dtype, group, name)):
            caught.add("readout")
    print(f"[attn] fault '{name}' ({group}): caught by {sorted(caught)}")
    assert tools <= caught, f"'{name}' ({group}) must be caught by {sorted(tools)}, was caught by {sorted(caught)}"


# ------------------------------------------------------------------------------------------------- 4. the pin of the finding
def _mask_test_case(L, dh, recipe):
    """Inputs of test_attention_masks_gpu.py / test_attention_long_masks_gpu.py (_run), as [B, h, L, dh]."""
    B, h = 2, 2
    H = h * dh
    rnd = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed))
    q = rnd(B * L, H, seed=1).to(BF)
    kv = rnd(B * L, 2 * H, seed=2)
    kv.view(B, L, 2 * H)[:, (3 * L) // 4:, :H] *= 6.0
    kv = kv.to(BF)
    d_o = rnd(B * L, H, seed=3).to(BF)
    kp = torch.ones(B, L, dtype=torch.uint8)
    kp[0, L - 3:] = 0
    kp[B - 1, 5:9] = 0
    a = torch.arange(L)
    mod = {"half": a >= L // 2, "third": a * 3 // L}[recipe].to(torch.uint8)
    sp = lambda t: t.view(B, L, h, dh).transpose(1, 2).contiguous()
    return sp(q), sp(kv[:, :H].contiguous()), sp(kv[:, H:].contiguous()), sp(d_o), kp, mod


@pytest.mark.parametrize("L,dh,recipe", [(200, 32, "half"), (600, 64, "third")])
@pytest.mark.parametrize("fault,flags", [("DIAG not applied to a padded key", 5), ("SEP boundary off by one", 4), ("one (q, k) pair admitted in a peaked row", 6)])
def test_old_criterion_misses_what_the_new_tools_catch(L, dh, recipe, fault, flags):
    q, k, v, d_o, kp, mod = _mask_test_case(L, dh, recipe)
    B, h = q.shape[:2]
    scale = dh ** -0.5
    al = AR.build_allowed(kp, flags, L, mod)
    bad_al = FAULTS[fault][3](kp, flags, L, mod)
    assert bool((bad_al != al).any())
    out = emulate(q, k, v, d_o, bad_al, scale, "bf16")
    # the old criterion: the correct rule's reference (fp64 here, fp32 autograd there), max|err| <= tol max|ref|, lse rtol 1e-3 / atol 2e-3
    f = AR.attn_fwd_ref(q, k, v, al, scale)
    b = AR.attn_bwd_ref(q, k, v, f["o"], f["lse"], d_o, al, scale)
    fr = {n: AR.old_criterion_fraction(out[n], r, tol) for n, r, tol in (("o", f["o"], 2e-2), ("dq", b["dq"], 3e-2), ("dk", b["dk"], 3e-2), ("dv", b["dv"], 3e-2))}
    print(f"[attn] '{fault}' L {L}: old criterion at {', '.join(f'{n} {x:.2f}' for n, x in fr.items())} of its tolerance")
    assert max(fr.values()) <= 1.0, fr
    assert torch.allclose(out["lse"].double(), f["lse"], rtol=1e-3, atol=2e-3)
    # the new tools
    by_bounds = _rejects(lambda: AR.check_all(out, q, k, v, d_o, al, scale, "bf16", fault))
    ro = lambda q_, k_, v_, g_: emulate(q_, k_, v_, g_, bad_al, scale, "bf16")
    by_readout = _rejects(lambda: AR.readout(ro, al, B, h, L, L, dh, BF, "bf16", fault, tensors=("o_dv",)))
    assert by_readout and (by_bounds or fault.startswith("one (q, k)")), (by_bounds, by_readout)
