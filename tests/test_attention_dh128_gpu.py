"""Head dim 128 through ops.attn_fwd / attn_bwd: everything the mmfm_attn_desc contract of include/mmfm.h promises at dh 64,

    allowed(b,q,k) = (DIAG && q==k) | (CAUSAL ? k<=q : keypad[b][k]) | (SEP && mod_id[q]!=mod_id[k]),

Lq != Lk, attention dropout drop_p and output dropout drop_o, the LSE and dq / dk / dv, on the three kernel families: the bf16 keep-bit
kernels (csrc/attention_long.hip, selected by the workspace), the bf16 general tiled kernels (csrc/attention_bf16.hip, no workspace) and
the fp32 parity kernels (csrc/attention.hip).  The reference is torch fp64 autograd on the same inputs (tests/dropout_refs.py).  With
dropout on, the reference is fed the kernels' own masks: the keep bits the forward left in the workspace, or - where the launch hashes -
the one-hot-V read-out of the same kernel family, and the flat hash of drop_o through mmfm_dropout_apply.

Shapes: B = 2, heads = 2, dh = 128, a fused qkv buffer with leading dim 3 * 256 (self attention) or a q / kv pair (cross attention).
  L = 40    one tile and a ragged one, less than one chunk; the fp32 untiled kernels (K / V still fit the LDS)
  L = 129   one key past the 128-row chunk boundary.  Not a multiple of 8: with a workspace the launch still runs the general kernels
            (the keep-bit kernels move 16-byte bit groups), which is part of the contract, so the hash read-out serves it
  L = 136   the keep-bit kernels' own "one group past the chunk boundary"
  L = 200   two chunks, ragged chunk and tile; the fp32 tiled kernels with three 64-row chunks
  Lq = 72, Lk = 129   cross attention (no flags); 129 again sends the workspace launches to the general kernels
  Lq = 72, Lk = 136   cross attention on the keep-bit kernels: more key tiles than query tiles, a ragged query tile against a key past
                      the chunk boundary, query chunks streamed in the dK / dV phase against key chunks in the dQ phase
  Lq = 40, Lk = 24    cross attention on the keep-bit kernels with fewer keys than queries, both ragged and below one tile pair
Wherever the keep-bit kernels are expected the test asserts that they ran: with dropout the forward leaves bits in the (zeroed)
workspace, and with or without it the backward leaves delta / the dropout scale per query in the workspace's tail.
mod_id puts the modality boundary at 3 L // 5 (24, 77, 81, 120: never a multiple of 32, so mixed tiles occur); keypad pads the last 5 keys
of batch row 1 and key 7 of row 0.  "headpad" pads sample 0's first 40 keys under SEP: no allowed key in the first key tile for its
modality-0 queries (the keep-bit forward's reference exponent comes from that tile).  As in the dh-64 tests every query row keeps at
least one allowed key (asserted): the engine never builds a row without one.

Tolerances.  fp32: the bounds of test_kernels_gpu.py::test_attention_fwd_bwd.  bf16: the bounds of test_attention_long_masks_gpu.py,
unchanged.  The reduction that doubles with dh is the one of S = Q K^T and dP = dO V^T: exact products of bf16 inputs (the reference
gets the same bf16 values) summed in fp32, 128 terms at 2^-24 each - nothing against the 2^-9 of rounding P and dS to bf16, whose
reductions (over keys for O and dQ, over queries for dK and dV) have the length they have at dh 64.  So no bound is widened."""
import math

import pytest
import torch

import dropout_refs as DR

pytestmark = pytest.mark.gpu

DH, B, HEADS = 128, 2, 2
H = HEADS * DH
P_DROP = 0.4
LENGTHS = [40, 129, 136, 200]
FLAGS = [0, 1, 2, 3, 4, 5, 6, 7]          # 5 = DIAG | SEP: the one MASKED combination that keeps the key padding beside the diagonal
SELF_CASES = [(L, f, False) for L in LENGTHS for f in FLAGS] + [(136, 4, True), (200, 4, True)]
CROSS = [(72, 129), (72, 136), (40, 24)]


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def close(a, b, rtol, atol, msg):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs()
    print(f"{msg}: max abs err {err.max().item():.3e}, worst err / (atol + rtol |ref|) {(err / (atol + rtol * b.abs())).max().item():.3f}")
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{msg}: max abs err {err.max().item():.3e} (ref max {b.abs().max().item():.3e})"


def close_bf16(a, b, msg, tol):
    a, b = a.double().cpu(), b.double().cpu()
    err, scale = (a - b).abs().max().item(), b.abs().max().item() + 1e-6
    print(f"{msg}: max abs err / scale {err / scale:.3e} (bound {tol})")
    assert err <= tol * scale, f"{msg}: max abs err {err:.3e} vs scale {scale:.3e}"


# which (Lq, Lk) of this file the keep-bit kernels take when a workspace is passed (the table of the module docstring: bit groups of 8
# queries / keys); every launch asks the library (ops.attn_family) and compares its answer with this and with the workspace writes
KEEPBIT_SHAPES = {(40, 40): True, (129, 129): False, (136, 136): True, (200, 200): True, (72, 129): False, (72, 136): True, (40, 24): True}


def run_case(ops, path, Lq, Lk, flags, headpad, p):
    """path: "keep" (bf16 + workspace), "general" (bf16, no workspace) or "fp32"."""
    from multi_modal_foundation_model_amd import _lib as Lb
    fp32 = path == "fp32"
    dt, code, es = (torch.float32, Lb.F32, 4) if fp32 else (torch.bfloat16, Lb.BF16, 2)
    self_attn = Lq == Lk
    if self_attn:                                                    # fused qkv rows [q | k | v], leading dim 3 H
        buf = rnd(B * Lq, 3 * H, seed=1)
        if not fp32:
            buf.view(B, Lq, 3 * H)[:, (3 * Lq) // 4:, H:2 * H] *= 6.0      # late keys exceed the first key tile's reference exponent
        buf = buf.to(dt)
        grad = torch.full_like(buf, float("nan"))
        qp, kp_, vp, ldq, ldk = buf.data_ptr(), buf.data_ptr() + H * es, buf.data_ptr() + 2 * H * es, 3 * H, 3 * H
        dqp, dkp, dvp = grad.data_ptr(), grad.data_ptr() + H * es, grad.data_ptr() + 2 * H * es
        q_in, k_in, v_in = buf[:, :H], buf[:, H:2 * H], buf[:, 2 * H:]
        dq, dk, dv = grad[:, :H], grad[:, H:2 * H], grad[:, 2 * H:]
    else:                                                            # q [B Lq, H] and kv rows [k | v], leading dim 2 H
        qb, kvb = rnd(B * Lq, H, seed=1).to(dt), rnd(B * Lk, 2 * H, seed=2).to(dt)
        gq, gkv = torch.full_like(qb, float("nan")), torch.full_like(kvb, float("nan"))
        qp, kp_, vp, ldq, ldk = qb.data_ptr(), kvb.data_ptr(), kvb.data_ptr() + H * es, H, 2 * H
        dqp, dkp, dvp = gq.data_ptr(), gkv.data_ptr(), gkv.data_ptr() + H * es
        q_in, k_in, v_in = qb, kvb[:, :H], kvb[:, H:]
        dq, dk, dv = gq, gkv[:, :H], gkv[:, H:]
    d_o = rnd(B * Lq, H, seed=3).to(dt)
    kp = torch.ones(B, Lk, dtype=torch.uint8)
    kp[1, Lk - 5:] = 0
    kp[0, 7] = 0
    if headpad:
        kp[0, :40] = 0
    kp = kp.cuda()
    mi = (torch.arange(max(Lq, Lk)) >= (3 * Lk) // 5).to(torch.uint8).cuda()
    assert ((3 * Lk) // 5) % 32 != 0
    allowed = DR.allowed_mask(kp, flags, Lq, mi)
    assert bool(allowed.any(-1).all()), "a query row without an allowed key"
    o, lse = torch.full((B * Lq, H), float("nan"), device="cuda", dtype=dt), torch.empty(B, HEADS, Lq, device="cuda")
    kw = {}
    kb, nbits = None, B * HEADS * ((Lq + 31) // 32) * ((Lk + 31) // 32) * 128
    if path == "keep":                                               # zeroed: only the keep-bit kernels write it
        kb = torch.zeros(ops.attn_keepbits_bytes(B, HEADS, Lq, Lk), dtype=torch.uint8, device="cuda")
        kw["keepbits"] = kb
    state = None
    if p > 0:
        state = torch.zeros(2, dtype=torch.int32, device="cuda")
        ops.rng_seed(state, 4321)
        kw["drop_p"], kw["drop_o"] = ops.dropout(state, 7, p), ops.dropout(state, 9, p)
    desc = ops.attn_desc(code, B, HEADS, Lq, Lk, DH, qp, kp_, vp, ldq, ldk, ldk, o.data_ptr(), H, lse, kp, mi if flags & 4 else None, flags,
                         DH ** -0.5, d_o=d_o.data_ptr(), lddo=H, dq=dqp, dk=dkp, dv=dvp, lddq=ldq, lddk=ldk, lddv=ldk, **kw)
    fam = ops.attn_family(desc)
    on_keepbit = fam == Lb.ATTN_FAMILY_KEEPBIT_LONG
    assert on_keepbit == (path == "keep" and KEEPBIT_SHAPES[(Lq, Lk)]), f"{path} Lq {Lq} Lk {Lk}: family {fam}"
    assert ops.attn_family(desc, backward=True) & Lb.ATTN_FAMILY_MASK == fam, "forward and backward on different kernel families"
    ops.attn_fwd(desc)
    mult_p = mult_o = None
    if p > 0:
        am = allowed[:, None].expand(B, HEADS, Lq, Lk)
        if on_keepbit:
            assert bool(kb[:nbits].any()), "dropout on the keep-bit kernels: the forward writes the bit tiles"
            mult_p = DR.keepbit_multiplier(ops, kb, p, B, HEADS, Lq, Lk)
            keep_p = ops.attn_keep_prob(p)                           # the keep-bit path honours p to 2^-10
            assert abs(keep_p - (1 - p)) <= 2 ** -11
        else:
            mult_p = DR.general_attn_multiplier(ops, state, 7, p, dt, DH, B, HEADS, Lq, Lk)
            keep_p = 1 - p
        n = int(am.sum().item())
        rate = (mult_p[am] != 0).float().mean().item()
        print(f"keep rate over {n} allowed elements: {rate:.5f} (keep {keep_p:.5f})")
        assert abs(rate - keep_p) < 5 * math.sqrt(p * (1 - p) / n) + 1e-4, f"keep rate {rate} over {n} allowed elements"
        mult_o = DR.flat_multiplier(ops, state, 9, p, B * Lq, H)
    elif on_keepbit:
        assert not bool(kb[:nbits].any()), "no dropout: no bit tile is written"
    ops.attn_bwd(desc)
    if kb is not None:                                               # delta / dropout scale per (b, head, query), behind the bit tiles
        tail = kb[nbits:nbits + B * HEADS * Lq * 4]
        assert bool(tail.any()) == on_keepbit, "only the keep-bit backward writes the workspace's tail"
    leaves = [t.double().contiguous().requires_grad_(True) for t in (q_in, k_in, v_in)]
    Q = leaves[0].view(B, Lq, HEADS, DH).transpose(1, 2)
    K_, V_ = [t.view(B, Lk, HEADS, DH).transpose(1, 2) for t in leaves[1:]]
    oref, lref = DR.attention_dropout_ref(Q, K_, V_, allowed, DH ** -0.5, mult_p, mult_o)
    oref.backward(d_o.double())
    what = f"{path} Lq {Lq} Lk {Lk} flags {flags} p {p}"
    if fp32:
        close(o, oref, rtol=1e-4, atol=2e-5, msg=f"{what}: o")
        close(lse, lref, rtol=1e-5, atol=1e-4, msg=f"{what}: lse")
        for name, g, leaf in (("dq", dq, leaves[0]), ("dk", dk, leaves[1]), ("dv", dv, leaves[2])):
            close(g, leaf.grad, rtol=1e-3, atol=5e-5, msg=f"{what}: {name}")
    else:
        close_bf16(o, oref, f"{what}: o", tol=2e-2)
        close(lse, lref, rtol=1e-3, atol=2e-3, msg=f"{what}: lse")
        for name, g, leaf in (("dq", dq, leaves[0]), ("dk", dk, leaves[1]), ("dv", dv, leaves[2])):
            close_bf16(g, leaf.grad, f"{what}: {name}", tol=3e-2)


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("L,flags,headpad", SELF_CASES)
def test_dh128_bf16_keepbit_workspace(ops, L, flags, headpad, p):
    """bf16 with the keep-bit workspace: csrc/attention_long.hip wherever L is a multiple of 8 (40, 136, 200), drop_p and drop_o on in
    the dropout cases, the keep mask read out of the workspace; o 2e-2, lse rtol 1e-3 / atol 2e-3, gradients 3e-2 of the tensor's scale."""
    run_case(ops, "keep", L, L, flags, headpad, p)


@pytest.mark.parametrize("L,flags,headpad", SELF_CASES)
def test_dh128_bf16_general_kernels(ops, L, flags, headpad):
    """bf16 without the workspace, dropout 0: attn_fwd_bf16_tiled_kernel<128> / attn_bwd_bf16_tiled_kernel<128, 0 / 1>; same bounds."""
    run_case(ops, "general", L, L, flags, headpad, 0.0)


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("L,flags,headpad", SELF_CASES)
def test_dh128_fp32(ops, L, flags, headpad, p):
    """fp32 parity kernels (untiled at L = 40, tiled from 129 on), hash dropout read off the same kernels; the fp32 bounds of
    test_kernels_gpu.py: o rtol 1e-4 / atol 2e-5, lse rtol 1e-5 / atol 1e-4, gradients rtol 1e-3 / atol 5e-5."""
    run_case(ops, "fp32", L, L, flags, headpad, p)


@pytest.mark.parametrize("path,p", [("keep", 0.0), ("keep", P_DROP), ("general", 0.0), ("fp32", 0.0), ("fp32", P_DROP)])
@pytest.mark.parametrize("Lq,Lk", CROSS)
def test_dh128_cross_attention(ops, Lq, Lk, path, p):
    """Lq != Lk, no flags, a q / kv buffer pair.  With the workspace, (72, 136) and (40, 24) run the keep-bit kernels and (72, 129) the
    general ones; run_case asserts which of the two wrote the workspace."""
    run_case(ops, path, Lq, Lk, 0, False, p)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("L", [129, 200])
def test_dh128_hash_dropout_forward_backward_agree(ops, dtype, L):
    """General kernels, hash dropout (no workspace): the backward regenerates the forward's mask.  As test_attention_dropout_consistency:
    q = k = 0 gives uniform probabilities, V = 1 gives O[q] = kept fraction / (1 - p), d_o = 1 gives dV[k] = sum_q keep(q, k) / ((1 - p) L):
    both sums count the kept (q, k) pairs."""
    from multi_modal_foundation_model_amd import _lib as Lb
    dt, code, es = (torch.float32, Lb.F32, 4) if dtype == "fp32" else (torch.bfloat16, Lb.BF16, 2)
    p = P_DROP
    qkv = torch.zeros(B * L, 3 * H, device="cuda", dtype=dt)
    qkv[:, 2 * H:] = 1.0
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.rng_seed(state, 1234)
    kp = torch.ones(B, L, dtype=torch.uint8, device="cuda")
    o, lse = torch.empty(B * L, H, device="cuda", dtype=dt), torch.empty(B, HEADS, L, device="cuda")
    d_o = torch.ones(B * L, H, device="cuda", dtype=dt)
    dqkv = torch.empty(B * L, 3 * H, device="cuda", dtype=dt)
    base = qkv.data_ptr()
    desc = ops.attn_desc(code, B, HEADS, L, L, DH, base, base + H * es, base + 2 * H * es, 3 * H, 3 * H, 3 * H, o.data_ptr(), H, lse, kp, None, 0,
                         DH ** -0.5, drop_p=ops.dropout(state, 7, p), d_o=d_o.data_ptr(), lddo=H, dq=dqkv.data_ptr(),
                         dk=dqkv.data_ptr() + H * es, dv=dqkv.data_ptr() + 2 * H * es, lddq=3 * H, lddk=3 * H, lddv=3 * H)
    ops.attn_fwd(desc)
    o1 = o.clone()
    ops.attn_fwd(desc)
    assert torch.equal(o, o1), "same state / site must give the same mask"
    of = o.float().view(B, L, HEADS, DH)
    assert bool((of == of[..., :1]).all()), "every column of a head sees the same kept keys"
    frac = of[..., 0] * (1 - p)
    assert abs(frac.mean().item() - (1 - p)) < 0.02 and frac.std().item() > 0.01
    ops.attn_bwd(desc)
    dv = dqkv[:, 2 * H:].float().view(B, L, HEADS, DH)[..., 0]
    # bf16: o and dv are each rounded once (2^-9 relative), the sums of L of them agree to that
    rtol = 1e-4 if dtype == "fp32" else 2 ** -8
    close(dv.sum(1), of[..., 0].sum(1), rtol=rtol, atol=1e-3, msg="fwd / bwd dropout masks agree")
    ops.rng_advance(state)
    ops.attn_fwd(desc)
    assert not torch.equal(o, o1), "advancing the RNG state must change the mask"


def test_dh128_is_the_widest_head(ops):
    """The launch check names the accepted head dims; 256 is not one."""
    from multi_modal_foundation_model_amd import _lib as Lb
    from multi_modal_foundation_model_amd._lib import MmfmError
    L, dh = 8, 256
    x = torch.zeros(L, 3 * dh, device="cuda")
    o, lse = torch.empty(L, dh, device="cuda"), torch.empty(1, 1, L, device="cuda")
    kp = torch.ones(1, L, dtype=torch.uint8, device="cuda")
    desc = ops.attn_desc(Lb.F32, 1, 1, L, L, dh, x.data_ptr(), x.data_ptr() + dh * 4, x.data_ptr() + 2 * dh * 4, 3 * dh, 3 * dh, 3 * dh, o.data_ptr(),
                         dh, lse, kp, None, 0, dh ** -0.5)
    with pytest.raises(MmfmError, match=r"\{8,16,32,64,128\}"):
        ops.attn_fwd(desc)
