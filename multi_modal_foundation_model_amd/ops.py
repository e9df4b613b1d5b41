"""Tensor-level wrappers over the C-ABI.  Each op either runs now (on torch's current stream) or,
when `plan` is a list, is appended to it as a pre-bound `(cfunc, args)` pair: the engine builds such
a plan once per batch shape and replays it every step (no per-step Python marshalling, and the
replay is hipGraph-capturable because no call allocates or synchronises)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_plan(plan, stream=None):
    st = _stream() if stream is None else stream
    for fn, args, _keep in plan:
        rc = fn(*args, st)
        if rc:
            L.check(rc, fn.__name__)


def _emit(plan, fn, args, keep=()):
    if plan is None:
        L.check(fn(*args, _stream()), fn.__name__)
    else:
        plan.append((fn, args, keep))


def P(t):
    return None if t is None else t.data_ptr()


def dt(t):
    if t.dtype == torch.float32:
        return L.F32
    if t.dtype == torch.bfloat16:
        return L.BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def dropout(state, site, p):
    if state is None or p <= 0:
        return L.NO_DROP
    return L.Dropout(state.data_ptr(), site, float(p))


def gemm_desc(A, B, Cout, M, N, K, *, lda, ldb, ldc, a_kcontig=1, b_kcontig=1, bias=None, pre_out=None, act=0,
              act_scale=1.0, gradmul_pre=None, drop=None, residual=None, ldr=0, splits=1, kchunk=0, slab_stride=0,
              dtype=None, c_f32=0, colsum=None):
    d = L.GemmDesc()
    d.dtype = dt(A) if dtype is None else dtype
    d.c_f32 = c_f32
    d.A, d.B, d.C = P(A), P(B), P(Cout)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, ldb, ldc
    d.a_kcontig, d.b_kcontig = a_kcontig, b_kcontig
    d.splits, d.kchunk, d.slab_stride = splits, kchunk, slab_stride
    d.bias, d.pre_out, d.act, d.act_scale, d.gradmul_pre = P(bias), P(pre_out), act, act_scale, P(gradmul_pre)
    d.drop = drop if drop is not None else L.NO_DROP
    d.residual, d.ldr = P(residual), ldr
    d.colsum = colsum if isinstance(colsum, int) else P(colsum)
    return d


def gemm(A, B, Cout, M, N, K, *, plan=None, **kw):
    d = gemm_desc(A, B, Cout, M, N, K, **kw)
    _emit(plan, L.lib().mmfm_gemm, (C.byref(d),), keep=(d,))


def live_rows(rec, B, T):
    """The mmfm_live_rows of a live-bin record tensor (int32, live_bins) over the row space B * T."""
    lv = L.LiveRows()
    lv.rec, lv.B, lv.T = P(rec), B, T
    lv._keep = rec
    return lv


def gemm_live(A, B, Cout, M, N, K, *, live, plan=None, **kw):
    """mmfm_gemm_live: the product over the compact row space of `live` (live_rows); M (or, for dY^T.X, K) is the full B * T."""
    d = gemm_desc(A, B, Cout, M, N, K, **kw)
    _emit(plan, L.lib().mmfm_gemm_live, (C.byref(d), C.byref(live)), keep=(d, live))


def live_bins(keep0, T, M, rec, plan=None):
    """rec int32 [M][live_rec_ints(T)] <- the live-bin records of keep0 u8 [M][T] (mmfm_live_bins)."""
    _emit(plan, L.lib().mmfm_live_bins, (P(keep0), T, M, P(rec)))


def gather_live_rows(src, dst, B, T, row_bytes, rec, plan=None):
    _emit(plan, L.lib().mmfm_gather_live_rows, (P(src), P(dst), B, T, row_bytes, P(rec)))


def gemm_pair(da, db, plan=None):
    """Two independent products (descriptors from gemm_desc) through mmfm_gemm_pair: two streaming weight-gradient launches become one."""
    _emit(plan, L.lib().mmfm_gemm_pair, (C.byref(da), C.byref(db)), keep=(da, db))


def gemm_family(desc, live=None):
    """The kernel family (L.GEMM_FAMILY_*) gemm - or, with `live` (live_rows), gemm_live - runs for `desc` (mmfm_gemm_family: nothing is
    launched, no tensor is read, no GPU is needed); raises where the launch would refuse."""
    fam = L.lib().mmfm_gemm_family(C.byref(desc), None if live is None else C.byref(live))
    if fam < 0:
        L.check(fam, "mmfm_gemm_family")
    return fam


def gemm_pair_fused(da, db):
    """Whether gemm_pair(da, db) leaves as one launch (mmfm_gemm_pair_fused; no GPU is needed); raises where it would refuse."""
    fused = L.lib().mmfm_gemm_pair_fused(C.byref(da), C.byref(db))
    if fused < 0:
        L.check(fused, "mmfm_gemm_pair_fused")
    return bool(fused)


def reduce_slabs(dst, src, n, nslabs, stride, accumulate=False, plan=None):
    _emit(plan, L.lib().mmfm_reduce_slabs, (P(dst), P(src), n, nslabs, stride, int(accumulate)))


def reduce_slabs_multi(items, device, plan=None):
    """items: (dst tensor, slab tensor, n, nslabs, stride, accumulate) -> one launch (mmfm_reduce_slabs_multi).  The table tensor
    is kept alive by the plan entry."""
    import numpy as np
    arr = (L.ReduceEntry * len(items))()
    chunk0 = 0
    for a, (dst, src, n, nslabs, stride, acc) in zip(arr, items):
        a.dst, a.src, a.n, a.slab_stride, a.nslabs, a.accumulate, a.chunk0 = P(dst), P(src), n, stride, nslabs, int(acc), chunk0
        chunk0 += (n + 255) // 256
    table = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)
    _emit(plan, L.lib().mmfm_reduce_slabs_multi, (P(table), len(items), chunk0), keep=(table,))


def colsum(x, R, N, ld, out, ws, accumulate=False, plan=None):
    _emit(plan, L.lib().mmfm_colsum, (dt(x), P(x), R, N, ld, P(out), int(accumulate), P(ws), ws.numel() * ws.element_size()))


def layernorm_fwd(x, gamma, beta, y, mean, rstd, R, H, eps=1e-5, ds_L=0, ds_T=0, plan=None):
    _emit(plan, L.lib().mmfm_layernorm_fwd, (dt(x), P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), R, H, eps, ds_L, ds_T))


def layernorm_bwd(dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, R, H, ws, accumulate=False, ds_L=0, ds_T=0, plan=None):
    _emit(plan, L.lib().mmfm_layernorm_bwd, (dt(x), P(dy), P(x), P(mean), P(rstd), P(gamma), P(dres), P(dx), P(dgamma),
                                             P(dbeta), int(accumulate), R, H, ds_L, ds_T, P(ws), ws.numel() * ws.element_size()))


def scalenorm_fwd(x, g, y, rinv, R, H, eps=1e-5, plan=None):
    """y = x * g / max(||x||, eps) per row; rinv = 1 / max(||x||, eps), negated for clamped rows (include/mmfm.h)."""
    _emit(plan, L.lib().mmfm_scalenorm_fwd, (dt(x), P(x), P(g), P(y), P(rinv), R, H, eps))


def scalenorm_bwd_workspace(R, H):
    return int(L.lib().mmfm_scalenorm_bwd_workspace(R, H))


def scalenorm_bwd(dy, x, rinv, g, dres, dx, dg, R, H, ws, accumulate=False, plan=None):
    """dx = dres + ScaleNorm'(dy) (dx may alias dres); dg (+)= sum over rows of x_hat . dy (deterministic)."""
    _emit(plan, L.lib().mmfm_scalenorm_bwd, (dt(x), P(dy), P(x), P(rinv), P(g), P(dres), P(dx), P(dg), int(accumulate), R, H, P(ws),
                                             ws.numel() * ws.element_size()))


def attn_desc(dtype, B, heads, Lq, Lk, dh, q, k, v, ldq, ldk, ldv, o, ldo, lse, keypad, mod_id, flags, scale,
              drop_p=None, drop_o=None, d_o=None, lddo=0, dq=None, dk=None, dv=None, lddq=0, lddk=0, lddv=0, keepbits=None):
    """keepbits: uint8 tensor of attn_keepbits_bytes(B, heads, Lq, Lk) bytes (one per attention site: the forward writes the keep
    decisions of drop_p there, the backward reads them) or None (both directions hash; include/mmfm.h)."""
    d = L.AttnDesc()
    d.dtype, d.B, d.heads, d.Lq, d.Lk, d.dh = dtype, B, heads, Lq, Lk, dh
    d.q, d.k, d.v, d.ldq, d.ldk, d.ldv = q, k, v, ldq, ldk, ldv
    d.o, d.ldo, d.lse, d.keypad, d.mod_id, d.flags, d.scale = o, ldo, P(lse), P(keypad), P(mod_id), flags, scale
    d.drop_p = drop_p if drop_p is not None else L.NO_DROP
    d.drop_o = drop_o if drop_o is not None else L.NO_DROP
    d.d_o, d.lddo, d.dq, d.dk, d.dv, d.lddq, d.lddk, d.lddv = d_o, lddo, dq, dk, dv, lddq, lddk, lddv
    d.keepbits = P(keepbits)
    return d


def attn_keepbits_bytes(B, heads, Lq, Lk):
    return int(L.lib().mmfm_attn_keepbits_bytes(B, heads, Lq, Lk))


def attn_keep_prob(p):
    """Keep probability the keep-bit attention path applies for drop probability p (quantised to 2^-10)."""
    return float(L.lib().mmfm_attn_keep_prob(float(p)))


def attn_family(desc, backward=False):
    """The kernel family (L.ATTN_FAMILY_*) attn_fwd / attn_bwd runs for `desc` (mmfm_attn_family: nothing is launched, no tensor is read,
    no GPU is needed); raises where the launch would refuse.  A backward on the single-pass bf16 kernel has L.ATTN_FAMILY_BWD_SINGLE set."""
    fam = L.lib().mmfm_attn_family(C.byref(desc), int(backward))
    if fam < 0:
        L.check(fam, "mmfm_attn_family")
    return fam


def attn_fwd(desc, plan=None):
    _emit(plan, L.lib().mmfm_attn_fwd, (C.byref(desc),), keep=(desc,))


def attn_bwd(desc, plan=None):
    _emit(plan, L.lib().mmfm_attn_bwd, (C.byref(desc),), keep=(desc,))


# ---- attention inside a window over time stamps (MMFM_ATTN_WINDOW)
def context_window(forward, backward):
    """(context.forward, context.backward) of mm.yaml -> the closed interval (lo, hi) of allowed pos[k] - pos[q], as upstream's
    create_context_mask reads the two keys: -1 is unbounded, and so is backward 0 (`if context_backward > 0`)."""
    for name, v in (("forward", forward), ("backward", backward)):
        if isinstance(v, bool) or not isinstance(v, int) or v < -1:
            raise ValueError(f"context.{name} must be an int >= -1, got {v!r}")
    hi = min(forward, L.ATTN_WINDOW_INF) if forward >= 0 else L.ATTN_WINDOW_INF
    lo = -min(backward, L.ATTN_WINDOW_INF) if backward > 0 else -L.ATTN_WINDOW_INF
    return lo, hi


def attn_window(pos, lo, hi):
    """mmfm_attn_window over `pos`, int32 [B][L] (attn_pos_prep writes it): allowed(q, k) needs lo <= pos[k] - pos[q] <= hi."""
    if pos.dtype != torch.int32 or not pos.is_contiguous():
        raise TypeError("attn_window: pos must be a contiguous int32 tensor [B][L]")
    return L.AttnWindow(pos.data_ptr(), int(max(lo, -L.ATTN_WINDOW_INF)), int(min(hi, L.ATTN_WINDOW_INF)))


def attn_win_family(desc, win, backward=False):
    """attn_family for a window launch (mmfm_attn_win_family; win None = attn_family): the dh 64 / 128 keep-bit family never takes one."""
    fam = L.lib().mmfm_attn_win_family(C.byref(desc), None if win is None else C.byref(win), int(backward))
    if fam < 0:
        L.check(fam, "mmfm_attn_win_family")
    return fam


def attn_win_fwd(desc, win, plan=None):
    _emit(plan, L.lib().mmfm_attn_win_fwd, (C.byref(desc), None if win is None else C.byref(win)), keep=(desc, win))


def attn_win_bwd(desc, win, plan=None):
    _emit(plan, L.lib().mmfm_attn_win_bwd, (C.byref(desc), None if win is None else C.byref(win)), keep=(desc, win))


def attn_pos_prep(B, Ts, stamps, pos, plan=None):
    """pos[b][off_j + t] = clamp(stamps[j][b][t], +-2^29): one int64 [B][Ts[j]] stamp tensor per slot (the uniform form passes the shared
    tensor once per slot), pos int32 [B][sum Ts]."""
    M = len(Ts)
    if len(stamps) != M:
        raise ValueError("attn_pos_prep: one stamp tensor per slot")
    for T, s in zip(Ts, stamps):
        if s.dtype != torch.int64 or not s.is_contiguous() or s.numel() != B * int(T):
            raise TypeError("attn_pos_prep: stamps must be contiguous int64 [B][T_j]")
    if pos.dtype != torch.int32 or not pos.is_contiguous() or pos.numel() != B * sum(int(t) for t in Ts):
        raise TypeError("attn_pos_prep: pos must be a contiguous int32 tensor [B][sum T_j]")
    seg = _seg_T(Ts)
    src = (C.c_void_p * M)(*[s.data_ptr() for s in stamps])
    _emit(plan, L.lib().mmfm_attn_pos_prep, (B, M, seg, src, P(pos)), keep=(seg, src))


def mask_prep(B, T, masks, strides, attn, channels, tokmask, keypad, keep0, mod_id, count, plan=None):
    M = len(masks)
    src = (C.c_void_p * M)(*[m.data_ptr() for m in masks])
    st = (C.c_int64 * M)(*strides)
    ch = (C.c_int64 * M)(*channels)
    _emit(plan, L.lib().mmfm_mask_prep, (B, T, M, src, st, P(attn), ch, P(tokmask), P(keypad), P(keep0), P(mod_id), P(count)),
          keep=(src, st, ch))


def _stitch_fwd(plan, fn, rec, tok, mod_row, pos, ts, keep0, x, emb, B, T, Lseq, slot, H, max_F):
    """The three stitch forwards: `rec` - (the live-bin record,) for mmfm_stitch_fwd_live, else () - sits behind keep0; `slot` is the
    modality's index m (the uniform and live forms) or its first token (the segment form)."""
    _emit(plan, fn, (dt(tok), P(tok), P(mod_row), P(pos), P(ts), P(keep0), *map(P, rec), P(x), P(emb), B, T, Lseq, slot, H, max_F))


def _stitch_bwd(plan, fn, rec, dx, dextra, ts, keep0, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq, slot, H, max_F, ws):
    """The three stitch backwards; `rec` and `slot` as in _stitch_fwd."""
    _emit(plan, fn, (dt(dx), P(dx), P(dextra), P(ts), P(keep0), *map(P, rec), drop if drop is not None else L.NO_DROP,
                     P(d_tok), P(d_mod_row), P(d_pos), int(acc_mod), int(acc_pos), B, T, Lseq, slot, H, max_F, P(ws),
                     ws.numel() * ws.element_size()))


def stitch_fwd(tok, mod_row, pos, ts, keep0, x, emb, B, T, Lseq, m, H, max_F, plan=None):
    _stitch_fwd(plan, L.lib().mmfm_stitch_fwd, (), tok, mod_row, pos, ts, keep0, x, emb, B, T, Lseq, m, H, max_F)


def stitch_fwd_live(tok, mod_row, pos, ts, keep0, rec, x, emb, B, T, Lseq, m, H, max_F, plan=None):
    _stitch_fwd(plan, L.lib().mmfm_stitch_fwd_live, (rec,), tok, mod_row, pos, ts, keep0, x, emb, B, T, Lseq, m, H, max_F)


def stitch_bwd_live(dx, dextra, ts, keep0, rec, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq, m, H, max_F, ws, plan=None):
    _stitch_bwd(plan, L.lib().mmfm_stitch_bwd_live, (rec,), dx, dextra, ts, keep0, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq,
                m, H, max_F, ws)


def stitch_bwd(dx, dextra, ts, keep0, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq, m, H, max_F, ws, plan=None):
    _stitch_bwd(plan, L.lib().mmfm_stitch_bwd, (), dx, dextra, ts, keep0, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq,
                m, H, max_F, ws)


# ---- modality segments (MMFM_MOD_SEGMENTS): slot j of the stitched sequence has Ts[j] bins, its own stamps and attention mask
def _seg_T(Ts):
    return (C.c_int32 * len(Ts))(*[int(t) for t in Ts])


def mask_prep_seg(B, Ts, masks, strides, attns, channels, tokmask, keypad, keep0, mod_id, count, plan=None):
    M = len(masks)
    if not (len(Ts) == len(attns) == len(strides) == len(channels) == M):
        raise ValueError("mask_prep_seg: one length, mask, stride, attention mask and channel count per slot")
    seg = _seg_T(Ts)
    src = (C.c_void_p * M)(*[m.data_ptr() for m in masks])
    at = (C.c_void_p * M)(*[a.data_ptr() for a in attns])
    st = (C.c_int64 * M)(*strides)
    ch = (C.c_int64 * M)(*channels)
    _emit(plan, L.lib().mmfm_mask_prep_seg, (B, M, seg, src, st, at, ch, P(tokmask), P(keypad), P(keep0), P(mod_id), P(count)),
          keep=(seg, src, st, at, ch))


def stitch_fwd_seg(tok, mod_row, pos, ts, keep0, x, emb, B, T, Lseq, off, H, max_F, plan=None):
    _stitch_fwd(plan, L.lib().mmfm_stitch_fwd_seg, (), tok, mod_row, pos, ts, keep0, x, emb, B, T, Lseq, off, H, max_F)


def stitch_bwd_seg(dx, dextra, ts, keep0, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq, off, H, max_F, ws, plan=None):
    _stitch_bwd(plan, L.lib().mmfm_stitch_bwd_seg, (), dx, dextra, ts, keep0, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq,
                off, H, max_F, ws)


# ---- per-sample token masks (MMFM_TOKEN_MASK_ROWS): every sample's own keep row, keep [B][L], and keep_any [L], their OR
def mask_prep_rows(B, Ts, masks, strides, attns, channels, tokmask, keypad, keep, keep_any, mod_id, count, plan=None):
    """mask_prep_seg's arguments (the uniform form passes T and the one attention mask once per slot); keep u8 [B][L], keep_any u8 [L]."""
    M = len(masks)
    if not (len(Ts) == len(attns) == len(strides) == len(channels) == M):
        raise ValueError("mask_prep_rows: one length, mask, stride, attention mask and channel count per slot")
    seg = _seg_T(Ts)
    src = (C.c_void_p * M)(*[m.data_ptr() for m in masks])
    at = (C.c_void_p * M)(*[a.data_ptr() for a in attns])
    st = (C.c_int64 * M)(*strides)
    ch = (C.c_int64 * M)(*channels)
    _emit(plan, L.lib().mmfm_mask_prep_rows, (B, M, seg, src, st, at, ch, P(tokmask), P(keypad), P(keep), P(keep_any), P(mod_id), P(count)),
          keep=(seg, src, st, at, ch))


def stitch_fwd_rows(tok, mod_row, pos, ts, keep, keep_ld, rec, x, emb, B, T, Lseq, off, H, max_F, plan=None):
    """The slot of T bins at `off` under keep[b * keep_ld + off + t] (keep_ld 0: one shared row); rec: the slot's live-bin record or None."""
    _emit(plan, L.lib().mmfm_stitch_fwd_rows, (dt(tok), P(tok), P(mod_row), P(pos), P(ts), P(keep), int(keep_ld), P(rec), P(x), P(emb), B, T, Lseq,
                                               off, H, max_F))


def stitch_bwd_rows(dx, dextra, ts, keep, keep_ld, rec, drop, d_tok, d_mod_row, d_pos, acc_mod, acc_pos, B, T, Lseq, off, H, max_F, ws, plan=None):
    _emit(plan, L.lib().mmfm_stitch_bwd_rows, (dt(dx), P(dx), P(dextra), P(ts), P(keep), int(keep_ld), P(rec),
                                               drop if drop is not None else L.NO_DROP, P(d_tok), P(d_mod_row), P(d_pos), int(acc_mod),
                                               int(acc_pos), B, T, Lseq, off, H, max_F, P(ws), ws.numel() * ws.element_size()))


def layernorm_fwd_seg(x, gamma, beta, y, mean, rstd, R, H, Ts, eps=1e-5, plan=None):
    seg = _seg_T(Ts)
    _emit(plan, L.lib().mmfm_layernorm_fwd_seg, (dt(x), P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), R, H, eps, len(Ts), seg), keep=(seg,))


def layernorm_bwd_seg(dy, x, mean, rstd, gamma, dres, dx, dgamma, dbeta, R, H, ws, Ts, accumulate=False, plan=None):
    seg = _seg_T(Ts)
    _emit(plan, L.lib().mmfm_layernorm_bwd_seg, (dt(x), P(dy), P(x), P(mean), P(rstd), P(gamma), P(dres), P(dx), P(dgamma), P(dbeta),
                                                 int(accumulate), R, H, len(Ts), seg, P(ws), ws.numel() * ws.element_size()), keep=(seg,))


def masked_loss_fwd(kind, pred, target, rowmask, mask_ld, T, R, N, loss_sum, ws, plan=None):
    _emit(plan, L.lib().mmfm_masked_loss_fwd, (dt(pred), kind, P(pred), P(target), P(rowmask), mask_ld, T, R, N, P(loss_sum), P(ws),
                                               ws.numel() * ws.element_size()))


def masked_loss_kind_fwd(kind, param, flags, pred, target, rowmask, mask_ld, T, R, N, loss_sum, ws, plan=None):
    """Every MMFM_LOSS_* kind (param = eps / beta / delta, flags = L.LOSS_FULL or 0); kinds 0 / 1 give masked_loss_fwd's bits."""
    _emit(plan, L.lib().mmfm_masked_loss_kind_fwd, (dt(pred), kind, float(param), flags, P(pred), P(target), P(rowmask), mask_ld, T, R, N,
                                                    P(loss_sum), P(ws), ws.numel() * ws.element_size()))


def loss_finalize(loss_sum, count, M, loss, inv_n, plan=None):
    _emit(plan, L.lib().mmfm_loss_finalize, (P(loss_sum), P(count), M, P(loss), P(inv_n)))


def masked_loss_bwd(kind, pred, target, rowmask, mask_ld, T, R, N, grad_out, inv_n, dpred, plan=None):
    _emit(plan, L.lib().mmfm_masked_loss_bwd, (dt(pred), kind, P(pred), P(target), P(rowmask), mask_ld, T, R, N, P(grad_out), P(inv_n), P(dpred)))


def masked_loss_kind_bwd(kind, param, flags, pred, target, rowmask, mask_ld, T, R, N, grad_out, inv_n, dpred, plan=None):
    _emit(plan, L.lib().mmfm_masked_loss_kind_bwd, (dt(pred), kind, float(param), flags, P(pred), P(target), P(rowmask), mask_ld, T, R, N,
                                                    P(grad_out), P(inv_n), P(dpred)))


def elem_strides(mask, B, T, N):
    """The (sb, st, sn) element strides of a per-element mask: a u8 tensor of three dimensions, each the full size (B, T, N) or 1 (a
    broadcast dimension: stride 0).  The tensor itself is passed as it is - nothing is expanded in memory."""
    if mask.dtype != torch.uint8 or mask.dim() != 3 or any(s not in (1, full) for s, full in zip(mask.shape, (B, T, N))):
        raise ValueError(f"element mask: a uint8 tensor of shape [{B} or 1, {T} or 1, {N} or 1], got {mask.dtype} {tuple(mask.shape)}")
    return tuple(0 if s == 1 else int(st) for s, st in zip(mask.shape, mask.stride()))


def masked_loss_elem_workspace(B, T, N):
    return L.lib().mmfm_masked_loss_elem_workspace(B * T, N)


def masked_loss_elem_fwd(kind, param, flags, pred, target, mask, B, T, N, loss_sum, count, ws, plan=None):
    """Every elementwise MMFM_LOSS_* kind under a per-element mask (`elem_strides`): the masked sum to loss_sum[0], the exact number
    of set elements to count[0] (int64).  ws: masked_loss_elem_workspace bytes."""
    sb, st, sn = elem_strides(mask, B, T, N)
    _emit(plan, L.lib().mmfm_masked_loss_elem_fwd, (dt(pred), kind, float(param), flags, P(pred), P(target), P(mask), sb, st, sn, B, T, N,
                                                    P(loss_sum), P(count), P(ws), ws.numel() * ws.element_size()), keep=(mask,))


def masked_loss_elem_bwd(kind, param, flags, pred, target, mask, B, T, N, grad_out, inv_n, dpred, plan=None):
    sb, st, sn = elem_strides(mask, B, T, N)
    _emit(plan, L.lib().mmfm_masked_loss_elem_bwd, (dt(pred), kind, float(param), flags, P(pred), P(target), P(mask), sb, st, sn, B, T, N,
                                                    P(grad_out), P(inv_n), P(dpred)), keep=(mask,))


def stage_masked(src, cm, B, T, N, dst, ld, plan=None):
    """dst[b,t,n] = cm(b,t,n) ? 0 : src[b,t,n]: src fp32 [B, T, N] contiguous, cm a per-element mask (`elem_strides`), dst fp32 / bf16 rows
    of pitch ld >= N (the padding columns are not written)."""
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("stage_masked: src must be a contiguous fp32 tensor")
    sb, st, sn = elem_strides(cm, B, T, N)
    _emit(plan, L.lib().mmfm_stage_masked, (dt(dst), P(src), P(cm), sb, st, sn, B, T, N, P(dst), ld), keep=(src, cm))


def chan_ld(chanmask, N):
    """The leading dimension of a channel mask: a contiguous u8 [B, N] tensor (N) or one [1, N] mask for all samples (0)."""
    if chanmask.dtype != torch.uint8 or chanmask.dim() != 2 or chanmask.shape[1] != N or not chanmask.is_contiguous():
        raise ValueError(f"channel mask: a contiguous uint8 tensor of shape [B or 1, {N}], got {chanmask.dtype} {tuple(chanmask.shape)}")
    return 0 if chanmask.shape[0] == 1 else N


def masked_loss_chan_workspace(R, N):
    return L.lib().mmfm_masked_loss_chan_workspace(R, N)


def masked_loss_chan_fwd(kind, param, flags, pred, target, rowmask, mask_ld, T, R, N, chanmask, loss_sum, count, ws, plan=None):
    """Every elementwise MMFM_LOSS_* kind under rowmask[b, t] & chanmask[b, c] (`chan_ld`; mask_ld 0: one row mask for all samples): the
    sum to loss_sum[0], the exact number of set elements to count[0] (int64).  ws: masked_loss_chan_workspace bytes."""
    _emit(plan, L.lib().mmfm_masked_loss_chan_fwd, (dt(pred), kind, float(param), flags, P(pred), P(target), P(rowmask), mask_ld, T, R, N,
                                                    P(chanmask), chan_ld(chanmask, N), P(loss_sum), P(count), P(ws),
                                                    ws.numel() * ws.element_size()), keep=(chanmask,))


def masked_loss_chan_bwd(kind, param, flags, pred, target, rowmask, mask_ld, T, R, N, chanmask, grad_out, inv_n, dpred, plan=None):
    _emit(plan, L.lib().mmfm_masked_loss_chan_bwd, (dt(pred), kind, float(param), flags, P(pred), P(target), P(rowmask), mask_ld, T, R, N,
                                                    P(chanmask), chan_ld(chanmask, N), P(grad_out), P(inv_n), P(dpred)), keep=(chanmask,))


def softmax_ce_fwd(pred, target, weight, eps, rowmask, mask_ld, T, R, N, loss_sum, rowstat, ws, plan=None):
    """Softmax cross-entropy (L.LOSS_SOFTMAX_CE) of [R, N] logits against fp32 targets: the masked sum to loss_sum[0].  weight: fp32 [N]
    class weights or None; eps: label smoothing; rowstat: fp32 [R, 2] for the backward's (lse, sum w t'), or None."""
    _emit(plan, L.lib().mmfm_softmax_ce_fwd, (dt(pred), P(pred), P(target), P(weight), float(eps), P(rowmask), mask_ld, T, R, N, P(loss_sum),
                                              P(rowstat), P(ws), ws.numel() * ws.element_size()))


def softmax_ce_bwd(pred, target, weight, eps, rowmask, mask_ld, T, R, N, rowstat, grad_out, inv_n, dpred, plan=None):
    """rowstat: what softmax_ce_fwd left (one pass over the row), or None (recomputed, the same bits)."""
    _emit(plan, L.lib().mmfm_softmax_ce_bwd, (dt(pred), P(pred), P(target), P(weight), float(eps), P(rowmask), mask_ld, T, R, N, P(rowstat),
                                              P(grad_out), P(inv_n), P(dpred)))


def argmax_confusion(pred, target, rowmask, mask_ld, T, R, N, conf, plan=None):
    """conf int64 [N, N] <- counts of (arg-max of target, arg-max of pred) over the masked rows (rowmask None: all), lowest index on a tie."""
    _emit(plan, L.lib().mmfm_argmax_confusion, (dt(pred), P(pred), P(target), P(rowmask), mask_ld, T, R, N, P(conf)))


def dropout_apply(src, dst, R, N, drop, plan=None):
    _emit(plan, L.lib().mmfm_dropout_apply, (dt(src), P(src), P(dst), R, N, drop))


def cast_bf16(src, dst, n, plan=None):
    _emit(plan, L.lib().mmfm_cast_f32_to_bf16, (P(src), P(dst), n))


def adamw_step(p, g, m, v, p_bf16, n, hyper, plan=None):
    _emit(plan, L.lib().mmfm_adamw_step, (P(p), P(g), P(m), P(v), P(p_bf16), n, P(hyper)))


class OptimRanges:
    """The range table of mmfm_grad_sumsq_ranges / mmfm_adamw_step_ranges (include/mmfm.h, MMFM_OPTIM_RANGES): `ranges` is a list of
    (start, end, hyper_row), sorted and disjoint, over flat buffers of n elements.  The library checks them and cuts them into chunks on
    the host; with a `device` the table is uploaded (once - it lives as long as this object) and the zeroed workspace of the
    sum-of-squares launch allocated beside it.  device=None keeps the host table only (no GPU needed)."""

    def __init__(self, ranges, n, hyper_rows, device=None):
        lib = L.lib()
        self.n, self.hyper_rows, self.n_ranges = int(n), int(hyper_rows), len(ranges)
        self.ranges = (L.OptimRange * max(1, self.n_ranges))(*[L.OptimRange(int(s), int(e), int(row), 0) for s, e, row in ranges])
        self.n_chunks = lib.mmfm_optim_ranges_chunks(self.ranges, self.n_ranges, self.n, self.hyper_rows)
        if self.n_chunks < 0:
            L.check(-1, "mmfm_optim_ranges_chunks")
        nbytes = lib.mmfm_optim_ranges_table_bytes(self.n_chunks, self.n_ranges)
        self.table_host = torch.zeros(nbytes, dtype=torch.uint8)
        L.check(lib.mmfm_optim_ranges_table(self.ranges, self.n_ranges, self.n, self.hyper_rows, self.table_host.data_ptr(), nbytes),
                "mmfm_optim_ranges_table")
        self.table = self.workspace = None
        if device is not None:
            self.table = self.table_host.to(device)
            self.workspace = torch.zeros(lib.mmfm_optim_ranges_workspace(self.n_chunks, self.n_ranges), dtype=torch.uint8, device=device)

    def chunks(self):
        """The host table as a list of (start, len, range, hyper_row), and first_chunk[n_ranges + 1]."""
        raw = bytes(self.table_host.numpy().tobytes())
        ch = (L.OptimChunk * self.n_chunks).from_buffer_copy(raw[:self.n_chunks * C.sizeof(L.OptimChunk)])
        first = (C.c_int32 * (self.n_ranges + 1)).from_buffer_copy(raw[self.n_chunks * C.sizeof(L.OptimChunk):])
        return [(c.start, c.len, c.range, c.hyper_row) for c in ch], list(first)

    def record(self):
        """The device record of the last sum-of-squares launch and the per-range sums (synchronises: a D2H copy)."""
        nrec = C.sizeof(L.OptimRecord)
        raw = bytes(self.workspace[:nrec + 8 * self.n_ranges].cpu().numpy().tobytes())
        rec = L.OptimRecord.from_buffer_copy(raw[:nrec])
        sums = list((C.c_double * self.n_ranges).from_buffer_copy(raw[nrec:]))
        return dict(total=rec.total, clip_coef=rec.clip_coef, nonfinite=int(rec.nonfinite), skipped=int(rec.skipped), range_sumsq=sums)


def grad_sumsq_ranges(g, tab, coef_in=1.0, max_norm=0.0, skip_nonfinite=False, plan=None):
    _emit(plan, L.lib().mmfm_grad_sumsq_ranges, (P(g), tab.n, tab.ranges, tab.n_ranges, P(tab.table), tab.n_chunks, float(coef_in),
                                                 float(max_norm), int(bool(skip_nonfinite)), P(tab.workspace), tab.workspace.numel()),
          keep=(tab,))


def adamw_step_ranges(p, g, m, v, p_bf16, tab, hyper, clipped=False, skip_nonfinite=False, plan=None):
    """hyper: device fp32 [tab.hyper_rows][8].  clipped: read clip_coef (and, with skip_nonfinite, the non-finite flag) from the record
    the last grad_sumsq_ranges(g, tab) left in tab.workspace."""
    _emit(plan, L.lib().mmfm_adamw_step_ranges, (P(p), P(g), P(m), P(v), P(p_bf16), tab.n, tab.ranges, tab.n_ranges, P(tab.table), tab.n_chunks,
                                                 P(hyper), tab.hyper_rows, P(tab.workspace) if clipped else None,
                                                 int(bool(skip_nonfinite)), ), keep=(tab,))


def grad_accumulate(g, stash, start, end, mode, plan=None):
    """mmfm_grad_accumulate over elements [start, end) of the flat fp32 buffers g and stash: mode L.GRAD_STASH copies g into stash,
    L.GRAD_ADD adds stash into g.  An empty range launches nothing."""
    _emit(plan, L.lib().mmfm_grad_accumulate, (P(g), P(stash), g.numel(), int(start), int(end), int(mode)))


def span_table(spans, g_numel, stage_numel, out=None):
    """The host table of mmfm_span_gather / mmfm_span_scatter: int64 [len(spans)][4] rows (g_off, s_off, len, live), checked here because
    the kernels cannot: every span inside its buffer, len >= 1, and no two spans overlapping in either buffer.  out: an int64 tensor
    [>= len(spans)][4] to fill (a pinned one, for a non-blocking upload); its remaining rows are left as they are."""
    rows = [(int(g), int(s), int(n), int(bool(live))) for g, s, n, live in spans]
    if len(rows) > L.SPAN_MAX:
        raise ValueError(f"span_table: {len(rows)} spans, at most {L.SPAN_MAX}")
    for col, size, what in ((0, int(g_numel), "G"), (1, int(stage_numel), "the staging buffer")):
        end = 0
        for r in sorted(rows, key=lambda r: r[col]):
            if r[2] < 1 or r[col] < end or r[col] + r[2] > size:
                raise ValueError(f"span_table: span {r} overlaps its neighbour or leaves {what} of {size} elements")
            end = r[col] + r[2]
    t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    if out is None:
        return t
    out[:len(rows)].copy_(t)
    return out


def span_gather(G, stage, table, n_spans, plan=None):
    """mmfm_span_gather: stage[s_off : s_off + len] = live ? G[g_off : g_off + len] : 0 for the first n_spans rows of the device table
    (span_table); a dead span is never loaded.  n_spans = 0 launches nothing."""
    _emit(plan, L.lib().mmfm_span_gather, (P(G), P(stage), P(table), int(n_spans)))


def span_scatter(stage, G, table, n_spans, plan=None):
    """mmfm_span_scatter: G[g_off : g_off + len] = stage[s_off : s_off + len] for the first n_spans rows of the device table."""
    _emit(plan, L.lib().mmfm_span_scatter, (P(stage), P(G), P(table), int(n_spans)))


def rng_seed(state, seed, plan=None):
    _emit(plan, L.lib().mmfm_rng_seed, (P(state), int(seed) & (2 ** 64 - 1)))


def rng_advance(state, plan=None):
    _emit(plan, L.lib().mmfm_rng_advance, (P(state),))


def collate_csr(B, max_T, max_N, pad_value, data, indices, indptr, indptr_off, nnz_off, T_b, N_b, out, tmask, smask, plan=None):
    _emit(plan, L.lib().mmfm_collate_csr, (B, max_T, max_N, float(pad_value), P(data), P(indices), P(indptr), P(indptr_off), P(nnz_off),
                                           P(T_b), P(N_b), P(out), P(tmask), P(smask)))


# ---------------------------------------------------------------------------------------------- row-owner fused kernels
def prep_table(entries, device):
    """entries: dicts with W (fp32 [N,K]) and optional gamma, beta, bias, Wp, WpT, bp, WpP, WpTP tensors -> (device table, n, tiles, keep).
    scalar_gain=True: gamma is a ScaleNorm's one-element gain, beta is not used (include/mmfm.h: mmfm_prep_entry.scalar_gain)."""
    import numpy as np
    arr = (L.PrepEntry * len(entries))()
    tile0 = 0
    for i, e in enumerate(entries):
        N, Kd = e["W"].shape
        if e.get("WpP") is not None and Kd % 16:
            raise ValueError(f"prep_table: entry {i}: WpP (unit-permuted along K) needs K % 16 == 0, got K = {Kd} (include/mmfm.h)")
        if e.get("WpTP") is not None and N % 16:
            raise ValueError(f"prep_table: entry {i}: WpTP (unit-permuted along N) needs N % 16 == 0, got N = {N} (include/mmfm.h)")
        a = arr[i]
        a.W, a.gamma, a.beta, a.bias = P(e["W"]), P(e.get("gamma")), P(e.get("beta")), P(e.get("bias"))
        a.Wp, a.WpT, a.bp = P(e.get("Wp")), P(e.get("WpT")), P(e.get("bp"))
        a.WpP, a.WpTP = P(e.get("WpP")), P(e.get("WpTP"))
        if e.get("scalar_gain"):
            if e.get("gamma") is None or e["gamma"].numel() != 1 or e.get("beta") is not None:
                raise ValueError(f"prep_table: entry {i}: scalar_gain needs a one-element gamma and no beta")
            a.scalar_gain = 1
        a.N, a.K, a.tile0 = N, Kd, tile0
        tile0 += (N + 31) // 32
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    table = torch.from_numpy(raw).to(device)
    return table, len(entries), tile0


def prep_weights(table, n, tiles, plan=None):
    _emit(plan, L.lib().mmfm_prep_weights, (P(table), n, tiles), keep=(table,))


def rowgemm(x, w, y, R, N, K, *, ldx=None, ldw=None, ldy=None, bias=None, ln=False, eps=1e-5, xhat=None, rstd=None, residual=None,
            ldr=0, stream_out=False, ln_bwd=False, bwd_xhat=None, bwd_rstd=None, rotate=True, plan=None):
    """ln / ln_bwd: False / True (or 0 / 1) = none / LayerNorm, 2 = ScaleNorm (include/mmfm.h: mmfm_rowgemm_desc)."""
    d = L.RowGemmDesc()
    d.R, d.K, d.N = R, K, N
    d.x, d.ldx, d.w, d.ldw = P(x), K if ldx is None else ldx, P(w), K if ldw is None else ldw
    d.bias, d.ln, d.eps, d.xhat, d.rstd = P(bias), int(ln), eps, P(xhat), P(rstd)
    d.residual, d.ldr, d.y, d.ldy = P(residual), ldr, P(y), N if ldy is None else ldy
    d.stream_out, d.ln_bwd, d.bwd_xhat, d.bwd_rstd, d.rotate = int(stream_out), int(ln_bwd), P(bwd_xhat), P(bwd_rstd), int(rotate)
    _emit(plan, L.lib().mmfm_rowgemm, (C.byref(d),), keep=(d,))


def rowgemm_groups(xs, ws, ys, R, N, K, *, ldx=None, ldw=None, ldy=None, biases=None, ln=False, eps=1e-5, xhat=None, rstd=None,
                   residual=None, ldr=0, stream_out=False, ln_bwd=False, bwd_xhat=None, bwd_rstd=None, rotate=True, plan=None):
    """mmfm_rowgemm_groups over len(ws) weight sets.  Forward (ln): xs = [x], ys = one output per group, each what
    rowgemm(x, ws[g], ys[g], ln=ln, bias=biases[g]) writes, the norm's x_hat / rstd written once.  Backward (ln_bwd): xs = one operand
    per group, ys = [y] = residual + norm'(sum_g xs[g] . ws[g]^T)."""
    G = len(ws)
    if not 1 <= G <= L.ROWGEMM_MAX_GROUPS:
        raise ValueError(f"rowgemm_groups: {G} groups (1 .. {L.ROWGEMM_MAX_GROUPS})")
    if len(xs) != (G if ln_bwd else 1) or len(ys) != (1 if ln_bwd else G):
        raise ValueError("rowgemm_groups: forward takes one x and a y per group, backward an x per group and one y")
    d = L.RowGemmGroupsDesc()
    d.R, d.K, d.N, d.groups = R, K, N, G
    for g in range(G):
        d.w[g] = P(ws[g])
        d.bias[g] = P(biases[g]) if biases is not None else None
    for g, x in enumerate(xs):
        d.x[g] = P(x)
    for g, y in enumerate(ys):
        d.y[g] = P(y)
    d.ldx, d.ldw, d.ldy = K if ldx is None else ldx, K if ldw is None else ldw, N if ldy is None else ldy
    d.ln, d.eps, d.xhat, d.rstd = int(ln), eps, P(xhat), P(rstd)
    d.residual, d.ldr = P(residual), ldr
    d.stream_out, d.ln_bwd, d.bwd_xhat, d.bwd_rstd, d.rotate = int(stream_out), int(ln_bwd), P(bwd_xhat), P(bwd_rstd), int(rotate)
    _emit(plan, L.lib().mmfm_rowgemm_groups, (C.byref(d),), keep=(d,))


# transformer.act (a `transformers` ACT2FN name) -> (MMFM_MLP_* kind, beta): the MLP activations the kernels build
MLP_ACTS = {
    "gelu": (L.MLP_GELU, 1.0),
    "relu": (L.MLP_RELU, 1.0),
    "silu": (L.MLP_SIGMOID, 1.0), "swish": (L.MLP_SIGMOID, 1.0), "quick_gelu": (L.MLP_SIGMOID, 1.702),
    "gelu_new": (L.MLP_GELU_TANH, 1.0), "gelu_pytorch_tanh": (L.MLP_GELU_TANH, 1.0), "gelu_fast": (L.MLP_GELU_TANH, 1.0),
}
# MMFM_MLP_* kind -> the mmfm_gemm act codes of its forward and of its gradient (un-fused and fp32 paths)
GEMM_ACTS = {L.MLP_GELU: (L.ACT_GELU, L.ACT_GELU_GRAD), L.MLP_RELU: (L.ACT_RELU, L.ACT_RELU_GRAD),
             L.MLP_SIGMOID: (L.ACT_SIGMOID, L.ACT_SIGMOID_GRAD), L.MLP_GELU_TANH: (L.ACT_GELU_TANH, L.ACT_GELU_TANH_GRAD)}


# embedder.act (a `transformers` ACT2FN name, or `identity`) -> the mmfm_gemm act codes of its forward and of its gradient.  softsign's
# gradient code is the fp32 one (from the saved pre-activation); the bf16 plan takes it from the output instead (ACT_SOFTSIGN_GRAD_OUT)
EMBED_ACTS = {
    "softsign": (L.ACT_SOFTSIGN, L.ACT_SOFTSIGN_GRAD),
    "identity": (L.ACT_EMB_IDENTITY, L.ACT_EMB_IDENTITY_GRAD), "linear": (L.ACT_EMB_IDENTITY, L.ACT_EMB_IDENTITY_GRAD),
    "relu": (L.ACT_EMB_RELU, L.ACT_EMB_RELU_GRAD),
    "gelu": (L.ACT_EMB_GELU, L.ACT_EMB_GELU_GRAD),
    "silu": (L.ACT_EMB_SILU, L.ACT_EMB_SILU_GRAD), "swish": (L.ACT_EMB_SILU, L.ACT_EMB_SILU_GRAD),
    "quick_gelu": (L.ACT_EMB_QUICK_GELU, L.ACT_EMB_QUICK_GELU_GRAD),
    "gelu_new": (L.ACT_EMB_GELU_TANH, L.ACT_EMB_GELU_TANH_GRAD), "gelu_pytorch_tanh": (L.ACT_EMB_GELU_TANH, L.ACT_EMB_GELU_TANH_GRAD),
    "gelu_fast": (L.ACT_EMB_GELU_TANH, L.ACT_EMB_GELU_TANH_GRAD),
    "tanh": (L.ACT_EMB_TANH, L.ACT_EMB_TANH_GRAD),
}


def embed_act(name):
    """(forward code, gradient code) of an embedder.act name; NotImplementedError for names without a kernel."""
    if name not in EMBED_ACTS:
        raise NotImplementedError(f"embedder act {name!r} has no kernel; accepted: {', '.join(EMBED_ACTS)}")
    return EMBED_ACTS[name]


def mlp_act(name):
    """(kind, beta) of a transformer.act name; NotImplementedError for names without a kernel."""
    if name not in MLP_ACTS:
        raise NotImplementedError(f"MLP act {name!r} has no kernel; accepted: {', '.join(MLP_ACTS)}")
    return MLP_ACTS[name]


def mlp_desc(R, *, x=None, ldx=256, eps=1e-5, w_up=None, b_up=None, w_down=None, b_down=None, drop=None, y=None, ldy=256, xhat=None,
             rstd=None, dy=None, lddy=256, w_down_t=None, w_up_t=None, t1=None, g=None, du=None, dx=None, lddx=256, rotate=True,
             scalenorm=False, act=L.MLP_GELU, act_beta=1.0):
    d = L.MlpDesc()
    d.R, d.x, d.ldx, d.eps = R, P(x), ldx, eps
    d.w_up, d.b_up, d.w_down, d.b_down = P(w_up), P(b_up), P(w_down), P(b_down)
    d.drop = drop if drop is not None else L.NO_DROP
    d.y, d.ldy, d.xhat, d.rstd = P(y), ldy, P(xhat), P(rstd)
    d.dy, d.lddy, d.w_down_t, d.w_up_t = P(dy), lddy, P(w_down_t), P(w_up_t)
    d.t1, d.g, d.du, d.dx, d.lddx, d.rotate = P(t1), P(g), P(du), P(dx), lddx, int(rotate)
    d.scalenorm, d.act, d.act_beta = int(scalenorm), int(act), float(act_beta)
    return d


def mlp_fwd(desc, plan=None):
    _emit(plan, L.lib().mmfm_mlp_fwd, (C.byref(desc),), keep=(desc,))


def mlp_bwd(desc, plan=None):
    _emit(plan, L.lib().mmfm_mlp_bwd, (C.byref(desc),), keep=(desc,))


def ln_linear_grad_workspace(K, device):
    """Zeroed workspace of mmfm_ln_linear_grad (partials + self re-arming tickets)."""
    return torch.zeros(L.lib().mmfm_ln_linear_grad_workspace(K) // 4, dtype=torch.float32, device=device)


def ln_linear_grad(Gdb, W, gamma, beta, N, K, dW, dbias, dgamma, dbeta, ws, accumulate_ln=False, plan=None):
    _emit(plan, L.lib().mmfm_ln_linear_grad, (P(Gdb), P(W), P(gamma), P(beta), N, K, P(dW), P(dbias), P(dgamma), P(dbeta), int(accumulate_ln),
                                              P(ws), ws.numel() * 4), keep=(ws,))


def sn_linear_grad(Gdb, W, g, N, K, dW, dbias, dg, ws, accumulate=False, plan=None):
    """ScaleNorm-fed linear: dW = g * G, dbias = db, dg (+)= sum W * G (mmfm_sn_linear_grad; ws as for ln_linear_grad)."""
    _emit(plan, L.lib().mmfm_sn_linear_grad, (P(Gdb), P(W), P(g), N, K, P(dW), P(dbias), P(dg), int(accumulate), P(ws), ws.numel() * 4),
          keep=(ws,))


def mt19937_jump(state, consumed, n):
    """Moves an MT19937 state on by `n` outputs without drawing (mmfm_mt19937_jump; host memory, no device involved).
    `state`: contiguous CPU int32 tensor of the 624 state words, updated in place; `consumed`: words of the current block
    already handed out (0..624).  Returns the new `consumed`."""
    if state.device.type != "cpu" or state.dtype != torch.int32 or state.numel() != 624 or not state.is_contiguous():
        raise TypeError("mt19937_jump: state must be a contiguous CPU int32 tensor of 624 words")
    c = C.c_int32(int(consumed))
    L.check(L.lib().mmfm_mt19937_jump(state.data_ptr(), C.byref(c), int(n)), "mmfm_mt19937_jump")
    return c.value


def mt19937_jump_reset():
    """Drops the cached jump polynomials (cold-cost measurements)."""
    L.check(L.lib().mmfm_mt19937_jump_reset(), "mmfm_mt19937_jump_reset")


# ---------------------------------------------------------------------------------------------- MT19937 on the device (MMFM_MT_DEVICE)
def mt_plan(n, streams=None):
    """(streams, blocks_per_stream) of a device draw of `n` outputs (mmfm_mt_plan; no HIP call): run s covers outputs
    [s * blocks * 624, min(n, (s + 1) * blocks * 624)).  `streams=None`: the library's choice; an int forces the count (never more runs
    than blocks)."""
    s, b = C.c_int32(0), C.c_int64(0)
    L.check(L.lib().mmfm_mt_plan(int(n), 0 if streams is None else int(streams), C.byref(s), C.byref(b)), "mmfm_mt_plan")
    return s.value, b.value


def mt_workspace(n, streams=None, device=None):
    """The workspace of the device draws of `n` outputs per draw (mmfm_mt_workspace), contents arbitrary."""
    nbytes = L.lib().mmfm_mt_workspace(int(n), 0 if streams is None else int(streams))
    if nbytes < 0:
        L.check(-1, "mmfm_mt_workspace")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _mt_state(state, what):
    if state.device.type != "cpu" or state.dtype != torch.int32 or state.numel() != 624 or not state.is_contiguous():
        raise TypeError(f"{what}: state must be a contiguous CPU int32 tensor of 624 words")
    return state.data_ptr()


def _mt_out(out, n, dtype, device, what):
    if out is None:
        if device is None:
            raise ValueError(f"{what}: give `out` or `device`")
        return torch.empty(n, dtype=dtype, device=device)
    if not out.is_cuda or out.dtype != dtype or out.numel() != n or not out.is_contiguous():
        raise TypeError(f"{what}: out must be a contiguous device {dtype} tensor of {n} elements")
    return out


def mt_uniform(state, consumed, n, skip=0, streams=None, out=None, device=None, ws=None):
    """out[i] = torch.rand's value for output skip + i of the MT19937 position (state, consumed) (rngjump.py; consumed as for
    mt19937_jump), generated on the device (mmfm_mt_uniform).  fp32, `n` elements; the host generator is not moved."""
    sp = _mt_state(state, "mt_uniform")
    out = _mt_out(out, n, torch.float32, device, "mt_uniform")
    ws = mt_workspace(n, streams, out.device) if ws is None else ws
    L.check(L.lib().mmfm_mt_uniform(sp, int(consumed), int(skip), int(n), P(out), 0 if streams is None else int(streams), P(ws), ws.numel(),
                                    _stream()), "mmfm_mt_uniform")
    return out


def mt_bernoulli(state, consumed, n, p, skip=0, streams=None, out=None, device=None, ws=None):
    """out[i] = torch.bernoulli(full(p))'s value (uint8 0 / 1) for output skip + i (mmfm_mt_bernoulli)."""
    sp = _mt_state(state, "mt_bernoulli")
    out = _mt_out(out, n, torch.uint8, device, "mt_bernoulli")
    ws = mt_workspace(n, streams, out.device) if ws is None else ws
    L.check(L.lib().mmfm_mt_bernoulli(sp, int(consumed), int(skip), int(n), float(p), P(out), 0 if streams is None else int(streams), P(ws),
                                      ws.numel(), _stream()), "mmfm_mt_bernoulli")
    return out


def mt_corrupt(state, consumed, src, cm, zero_ratio, random_ratio, streams=None, out=None, ws=None):
    """The masker's corruption of `src` (fp32 [B, T, N], contiguous, on the device) under the compact mask `cm` (`elem_strides`), drawn
    from outputs [0, 3 B T N) of the position (state, consumed): mmfm_mt_corrupt.  Returns the corrupted copy (`out=src` corrupts in place)."""
    sp = _mt_state(state, "mt_corrupt")
    if not src.is_cuda or src.dtype != torch.float32 or src.dim() != 3 or not src.is_contiguous():
        raise TypeError("mt_corrupt: src must be a contiguous fp32 device tensor [B, T, N]")
    B, T, N = src.shape
    if not cm.is_cuda:
        raise TypeError("mt_corrupt: cm must be on the device")
    sb, st, sn = elem_strides(cm, B, T, N)
    if out is None:
        out = torch.empty_like(src)
    elif out.data_ptr() != src.data_ptr() and (not out.is_cuda or out.dtype != torch.float32 or out.shape != src.shape or not out.is_contiguous()):
        raise TypeError("mt_corrupt: out must be src or a contiguous fp32 device tensor of its shape")
    ws = mt_workspace(B * T * N, streams, src.device) if ws is None else ws
    L.check(L.lib().mmfm_mt_corrupt(sp, int(consumed), B, T, N, P(src), P(cm), sb, st, sn, float(zero_ratio), float(random_ratio), P(out),
                                    0 if streams is None else int(streams), P(ws), ws.numel(), _stream()), "mmfm_mt_corrupt")
    return out


# ---------------------------------------------------------------------------------------------- per-session linear layers (MMFM_SESSION_LINEAR)
def session_desc(dtype, B, T, width, N_max, S, sid, n, w_off, *, ld_pad=None, ld_p=None, b_off=None, w=None, w_elems=None, bias=None, b_elems=None):
    """mmfm_session_desc over the device tables sid int32 [B], n int32 [S], w_off / b_off int64 [S] and the flat buffers `w` (storage
    `dtype`: L.F32 / L.BF16) and `bias` (fp32).  w_elems / b_elems default to the tensors' sizes (give them where w is None: mmfm_session_dw
    bounds the gradient buffers with them)."""
    d = L.SessionDesc()
    d.dtype, d.B, d.T, d.P, d.N_max, d.S = dtype, B, T, width, N_max, S
    d.ld_pad = N_max if ld_pad is None else ld_pad
    d.ld_p = width if ld_p is None else ld_p
    d.sid, d.n, d.w_off, d.b_off = P(sid), P(n), P(w_off), P(b_off)
    d.w, d.w_elems = P(w), int(w.numel() if w_elems is None else w_elems)
    d.bias, d.b_elems = P(bias), int((bias.numel() if bias is not None else 0) if b_elems is None else b_elems)
    d._keep = (sid, n, w_off, b_off, w, bias)
    return d


def session_reduce(desc, x_pad, y, plan=None):
    """y [B*T, P] = x_pad[.., :n_s] . W_s (+ bias_s), the session s of each sample from desc.sid (mmfm_session_reduce)."""
    _emit(plan, L.lib().mmfm_session_reduce, (C.byref(desc), P(x_pad), P(y)), keep=(desc,))


def session_expand(desc, f, y_pad, plan=None):
    """y_pad [B*T, ld_pad] = f . W_s^T (+ bias_s) in columns [0, n_s), zeros in [n_s, N_max) (mmfm_session_expand)."""
    _emit(plan, L.lib().mmfm_session_expand, (C.byref(desc), P(f), P(y_pad)), keep=(desc,))


def session_dw_chunk(B):
    """Samples per chunk of mmfm_session_dw's run table: about 64 chunks over the batch, so that one session owning the whole batch
    still spreads over the chip and many small sessions keep one chunk (a direct write) each."""
    return max(1, -(-int(B) // 64))


def session_runs_ints(B, S, chunk):
    """The int32 elements of the run table (mmfm_session_runs_ints)."""
    return L.SESSION_RUN_HDR + int(B) + L.SESSION_RUN_ENT * session_dw_chunks(B, S, chunk)


def session_dw_chunks(B, S, chunk):
    """The capacity of the chunk table (mmfm_session_dw_chunks): min(B, ceil(B / chunk) + min(S, B, 64))."""
    return min(int(B), -(-int(B) // int(chunk)) + min(int(S), int(B), L.SESSION_MAX_PER_BATCH))


def session_runs(sid, S, chunk, names=None):
    """The run table of mmfm_session_dw as a numpy int32 array (include/mmfm.h), from the per-sample session indices: a pure function
    of its arguments, no device involved.  Samples keep their batch order inside a session and sessions come in index order, so the
    table - and with it every sum - depends on the mix alone.  ValueError for an index outside [0, S) and for more than 64 distinct
    sessions in the batch (`names`: index -> eid for the message)."""
    import numpy as np
    sid = np.asarray(sid, dtype=np.int64).reshape(-1)
    B, S, chunk = int(sid.size), int(S), int(chunk)
    if B < 1 or S < 1 or chunk < 1:
        raise ValueError(f"session_runs: B {B}, S {S}, chunk {chunk} must all be >= 1")
    bad = sid[(sid < 0) | (sid >= S)]
    if bad.size:
        raise ValueError(f"session_runs: session index {int(bad[0])} outside [0, {S})")
    present = np.unique(sid)
    if present.size > L.SESSION_MAX_PER_BATCH:
        label = [str(names[int(k)]) if names is not None else str(int(k)) for k in present]
        raise ValueError(f"session_runs: {present.size} distinct sessions in one batch, at most {L.SESSION_MAX_PER_BATCH} are built: "
                         + ", ".join(label))
    cap = session_dw_chunks(B, S, chunk)
    order = np.argsort(sid, kind="stable")
    entries, start = [], 0
    for k in present:
        m = int((sid == k).sum())
        nch = -(-m // chunk)
        for j in range(nch):
            cnt = min(chunk, m - j * chunk)
            entries.append((int(k), start, cnt, nch if j == 0 else 0))
            start += cnt
    assert len(entries) <= cap and start == B
    out = np.zeros(L.SESSION_RUN_HDR + B + L.SESSION_RUN_ENT * cap, dtype=np.int32)
    out[:4] = (len(entries), chunk, cap, B)
    out[4:4 + B] = order
    if entries:
        out[4 + B:4 + B + 4 * len(entries)] = np.asarray(entries, dtype=np.int32).reshape(-1)
    return out


def session_dw_workspace(B, width, N_max, S, chunk, device):
    """The slab workspace of mmfm_session_dw (contents arbitrary: nothing in it is read before it is written)."""
    nbytes = L.lib().mmfm_session_dw_workspace(B, width, N_max, S, chunk)
    if nbytes < 0:
        L.check(-1, "mmfm_session_dw_workspace")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def session_dw(desc, a_pad, q, runs, chunk, dw, db, bias_from_pad, ws, plan=None):
    """dW_s = sum over the samples of s of a_pad[.., :n_s]^T . q at dw + w_off[s]; db (or None) the column sum of q (bias_from_pad False:
    the read-in) or of a_pad (True: the read-out) at db + b_off[s].  runs: the device copy of session_runs(...) for the same chunk;
    absent sessions keep their spans (mmfm_session_dw)."""
    _emit(plan, L.lib().mmfm_session_dw, (C.byref(desc), P(a_pad), P(q), P(runs), int(chunk), P(dw), P(db), int(bool(bias_from_pad)), P(ws),
                                          ws.numel() * 4), keep=(desc, runs, ws))
