"""Attention output dropout (drop_o), kernel body by kernel body, against torch fp64 fed the kernels' own masks.

Thirteen kernel bodies apply `dout` (the nn.Dropout in front of out_proj): the forward epilogues scale / zero the output, the backward
bodies re-apply the mask to d_o and form delta = sum d_o' * (o before drop_o) from the stored output AFTER drop_o.  Which launch reaches
which body (mmfm_attn_fwd / mmfm_attn_bwd in csrc/attention.hip try attention_fast, attention_long, attention_bf16, then fp32 compute):

  body                                        reached by
  attention.hip      attn_fwd_kernel          fp32, K/V (fwd) and Q/dO/K/V (bwd) images fit 160 KB of LDS:   (3,4,16,8) (2,8,200,32) x(40,72,32)
                     attn_bwd_kernel            the same launches (one decision per shape for both directions)
                     attn_fwd_tiled_kernel    fp32, images do not fit:                                       (2,4,600,64) x(40,700,64)
                     attn_bwd_tiled_kernel      the same launches (PHASE 0 dK/dV and PHASE 1 dQ share the body)
                     (T = bf16 storage)       bf16 with dh = 8 (no MFMA kernel takes it):                    bf16 (3,4,16,8)
  attention_bf16.hip attn_fwd_bf16_kernel     bf16, dh 16 / 64 (and dh 32 when the fast pair refuses), fits:  (2,4,48,16) (2,2,70,64) x(224,100,16)
                                                                                                             x(200,200,64) x(72,40,32)+drop_p x(40,72,32)
                     attn_bwd1_bf16_kernel    ... and ceil32(Lk) <= min(224, ceil32(Lq)) (single pass):      all of those but x(40,72,32)
                     attn_bwd_bf16_kernel     ... and Lk > Lq or Lk > 224 (two-phase; both phases drop d_o):  x(40,72,32)
                     attn_fwd_bf16_tiled_k.   bf16 without the keep-bit workspace, images do not fit:        (1,2,600,64)
                     attn_bwd_bf16_tiled_k.     the same launch (both phases)
  attention_fast.hip attn_fwd_fast_kernel     bf16, dh 32, L % 8 == 0, Lq <= 256, Lk <= 224, Lk tiles <= Lq tiles; with drop_p only when the
                     attn_bwd_fast_kernel     keep-bit workspace is passed:   (2,8,200,200) x(3,4,72,40) (2,2,104,104), + CAUSAL, + SEP
                                              (x(72,40,32) of the bf16 row runs here in the setting without drop_p: no workspace needed)
  attention_long.hip attn_fwd_long_kernel     bf16, dh 64, L % 8 == 0, keep-bit workspace passed:   (2,2,600,600) x(1,1,40,24) x(1,2,608,600),
                     attn_bwd_long_prep_k.    + CAUSAL, + SEP.  The prep kernel writes dropout'(d_o) into dq and delta behind the bit tiles.

(x = cross attention Lq, Lk, dh with B = 2, heads = 4 unless given; the shapes are those of the existing tests of each family.)

Every case runs two settings - drop_p off / drop_o 0.25, and drop_p 0.4 / drop_o 0.25 on another site - with padded keys in the first
and the last batch element.  The drop_o multiplier comes from mmfm_dropout_apply on ones (counter row * heads * dh + col: independent
of every attention kernel), the drop_p multiplier from the keep bits or the one-hot-V read-out (tests/dropout_refs.py).  Tolerances are
those of the existing test of the same family (dropout adds one multiply and no rounding step): fp32 test_attention_fwd_bwd, bf16
test_attention_bf16_fwd_bwd, keep-bit test_attention_fast_dropout_matches_reference / test_attention_long_keepbit_kernels_match_reference."""
import pytest
import torch

import dropout_refs as DR

pytestmark = pytest.mark.gpu

P_ATT, P_OUT, SITE_P, SITE_O = 0.4, 0.25, 5, 6
DIAG, CAUSAL, SEP = 1, 2, 4


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def close(a, b, rtol, atol, msg):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{msg}: max abs err {err:.3e} (ref max {b.abs().max().item():.3e})"


def close_bf16(a, b, msg, tol):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= tol * scale, f"{msg}: max abs err {err:.3e} vs scale {scale:.3e}"


#        family      B  heads Lq   Lk   dh  flags  wide
CASES = [("fp32",    3, 4,    16,  16,  8,  DIAG,  True),
         ("fp32",    2, 8,    200, 200, 32, DIAG,  False),
         ("fp32",    2, 4,    600, 600, 64, DIAG,  True),          # tiled
         ("fp32",    2, 4,    40,  72,  32, 0,     False),
         ("fp32",    2, 4,    40,  700, 64, 0,     False),         # tiled
         ("bf16",    3, 4,    16,  16,  8,  DIAG,  False),         # fp32 compute on bf16 storage
         ("bf16",    2, 4,    48,  48,  16, CAUSAL, True),
         ("bf16",    2, 2,    70,  70,  64, DIAG,  False),
         ("bf16",    2, 4,    224, 100, 16, 0,     False),
         ("bf16",    2, 4,    200, 200, 64, 0,     True),
         ("bf16",    2, 4,    72,  40,  32, 0,     False),
         ("bf16",    2, 4,    40,  72,  32, 0,     True),          # two-phase backward
         ("bf16",    1, 2,    600, 600, 64, DIAG,  True),          # tiled bf16
         ("fast",    2, 8,    200, 200, 32, DIAG,  True),
         ("fast",    3, 4,    72,  40,  32, 0,     False),
         ("fast",    2, 2,    104, 104, 32, DIAG,  False),
         ("fast",    2, 2,    104, 104, 32, CAUSAL, False),
         ("fast",    2, 8,    200, 200, 32, SEP,   False),
         ("long",    2, 2,    600, 600, 64, DIAG,  True),
         ("long",    1, 1,    40,  24,  64, 0,     False),
         ("long",    1, 2,    608, 600, 64, 0,     False),
         ("long",    1, 2,    200, 200, 64, CAUSAL, False),
         ("long",    2, 2,    600, 600, 64, SEP,   False)]


@pytest.mark.parametrize("family,B,heads,Lq,Lk,dh,flags,wide", CASES)
def test_attention_output_dropout_matches_reference(ops, family, B, heads, Lq, Lk, dh, flags, wide):
    from multi_modal_foundation_model_amd import _lib as Lb
    H = heads * dh
    keepbit = family in ("fast", "long")
    dtype = torch.float32 if family == "fp32" else torch.bfloat16
    code, es = (Lb.F32, 4) if family == "fp32" else (Lb.BF16, 2)
    q = rnd(B * Lq, H, seed=1).to(dtype)
    kv = rnd(B * Lk, 2 * H, seed=2)
    if keepbit:                             # as the keep-bit families' own tests: a late jump of the running maximum
        kv.view(B, Lk, 2 * H)[:, (3 * Lk) // 4:, :H] *= 6.0
    kv = kv.to(dtype)
    # o and d_o inside wider buffers (wide): 8 guard columns on either side, leading dim H + 16
    off, ld = (8, H + 16) if wide else (0, H)
    d_o_buf = torch.full((B * Lq, ld), 77.0, device="cuda", dtype=dtype)
    d_o = d_o_buf[:, off:off + H]
    d_o.copy_(rnd(B * Lq, H, seed=3))
    kp = torch.ones(B, Lk, dtype=torch.uint8)
    kp[0, Lk - 3:] = 0
    kp[B - 1, 5:9] = 0
    kp = kp.cuda()
    mod_id = (torch.arange(max(Lq, Lk)) >= Lq // 2).to(torch.uint8).cuda()
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 2024)
    mult_o = DR.flat_multiplier(ops, state, SITE_O, P_OUT, B * Lq, H)
    rate = (mult_o != 0).float().mean().item()
    assert abs(rate - (1 - P_OUT)) < 5 * (P_OUT * (1 - P_OUT) / mult_o.numel()) ** 0.5 + 1e-4, f"drop_o keep rate {rate}"
    allowed = DR.allowed_mask(kp, flags, Lq, mod_id)

    for p_att in (0.0, P_ATT):
        tag = f"{family} ({B},{heads},{Lq},{Lk},{dh}) flags {flags} drop_p {p_att}"
        o_buf = torch.full((B * Lq, ld), 55.0, device="cuda", dtype=dtype)
        o = o_buf[:, off:off + H]
        lse = torch.empty(B, heads, Lq, device="cuda")
        dq, dkv = torch.full_like(q, float("nan")), torch.full_like(kv, float("nan"))
        kb = torch.zeros(ops.attn_keepbits_bytes(B, heads, Lq, Lk), dtype=torch.uint8, device="cuda") if keepbit else None
        desc = ops.attn_desc(code, B, heads, Lq, Lk, dh, q.data_ptr(), kv.data_ptr(), kv.data_ptr() + H * es, H, 2 * H, 2 * H, o.data_ptr(), ld, lse,
                             kp, mod_id, flags, dh ** -0.5, drop_p=ops.dropout(state, SITE_P, p_att), drop_o=ops.dropout(state, SITE_O, P_OUT),
                             d_o=d_o.data_ptr(), lddo=ld, dq=dq.data_ptr(), dk=dkv.data_ptr(), dv=dkv.data_ptr() + H * es, lddq=H, lddk=2 * H,
                             lddv=2 * H, keepbits=kb)
        ops.attn_fwd(desc)
        mult_p = None
        if p_att > 0:
            if keepbit:
                mult_p = DR.keepbit_multiplier(ops, kb, p_att, B, heads, Lq, Lk)
            else:
                mult_p = DR.general_attn_multiplier(ops, state, SITE_P, p_att, dtype, dh, B, heads, Lq, Lk)
            al = allowed[:, None].expand(B, heads, Lq, Lk)
            rate = (mult_p[al] != 0).float().mean().item()
            keep_p = ops.attn_keep_prob(p_att) if keepbit else 1 - p_att
            assert abs(rate - keep_p) < 5 * (p_att * (1 - p_att) / int(al.sum())) ** 0.5 + 1e-4, f"{tag}: drop_p keep rate {rate}"
        ops.attn_bwd(desc)
        if wide:
            assert torch.all(o_buf[:, :off] == 55.0) and torch.all(o_buf[:, off + H:] == 55.0), f"{tag}: guard columns of o"
            assert torch.all(d_o_buf[:, :off] == 77.0) and torch.all(d_o_buf[:, off + H:] == 77.0), f"{tag}: guard columns of d_o"

        qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
        Q = qr.view(B, Lq, heads, dh).transpose(1, 2)
        K_, V_ = [t.view(B, Lk, heads, dh).transpose(1, 2) for t in kvr.split(H, dim=1)]
        oref, lref = DR.attention_dropout_ref(Q, K_, V_, allowed, dh ** -0.5, mult_p, mult_o)
        oref.backward(d_o.double())
        if family == "fp32":
            close(o, oref.detach(), 1e-4, 2e-5, f"{tag}: o")
            close(lse, lref.detach(), 1e-5, 1e-4, f"{tag}: lse")
            close(dq, qr.grad, 1e-3, 5e-5, f"{tag}: dq")
            close(dkv[:, :H], kvr.grad[:, :H], 1e-3, 5e-5, f"{tag}: dk")
            close(dkv[:, H:], kvr.grad[:, H:], 1e-3, 5e-5, f"{tag}: dv")
        else:
            close_bf16(o, oref.detach(), f"{tag}: o", 2e-2)
            close(lse, lref.detach(), 1e-3, 2e-3, f"{tag}: lse")
            close_bf16(dq, qr.grad, f"{tag}: dq", 3e-2)
            close_bf16(dkv[:, :H], kvr.grad[:, :H], f"{tag}: dk", 3e-2)
            close_bf16(dkv[:, H:], kvr.grad[:, H:], f"{tag}: dv", 3e-2)
