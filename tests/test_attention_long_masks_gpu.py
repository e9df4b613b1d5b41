"""The dh = 64 keep-bit attention pair (csrc/attention_long.hip) under CAUSAL and SEP, i.e. the whole mask rule of include/mmfm.h

    allowed(b,q,k) = (DIAG && q==k) | (CAUSAL ? k<=q : keypad[b][k]) | (SEP && mod_id[q]!=mod_id[k])

against torch fp32 autograd on the same bf16 inputs, with and without attention-probability dropout: the dh = 64 twin of
test_attention_masks_gpu.py (same reference, same tolerances - they describe bf16, not the kernel).  At dh = 64 the keep-bit workspace
is what selects the pair, so every case passes one.  With dropout the keep mask is read out of the bit tiles the forward leaves in the
workspace (documented layout): only the keep-bit kernels' generator writes it, so these cases fail wherever CAUSAL / SEP launches of
this head width still run on the general kernels."""
import math

import pytest
import torch

import dropout_refs as DR

pytestmark = pytest.mark.gpu

DH = 64
# (B, heads, L, mod_id recipe), the smallest shapes that reach each structural case of the streamed kernels (128-key chunks of four
# 32-key tiles, eight query tiles per forward / dQ workgroup, four key tiles per dK / dV workgroup):
#   72  "half" : one chunk, ragged last tile, the modality boundary inside a tile
#   104 "mod3" : non-contiguous modalities: every tile mixed under SEP
#   200 "third": two chunks, ragged chunk and tile, three modalities
#   296 "third": ten query tiles: a second workgroup of the 8-wave forward with inactive waves; three chunks
#   600 "third": BASELINE configs[4]'s own L: 19 tiles, 5 chunks, whole chunks skipped under CAUSAL
SHAPES = [(2, 2, 72, "half"), (2, 2, 104, "mod3"), (2, 2, 200, "third"), (1, 2, 296, "third"), (1, 2, 600, "third")]
FLAGS = [2, 4, 6, 5, 7]
# "headpad": sample 0 has no allowed key in the first key tile for some queries (the exact pass under the mask rule)
CASES = [(*s, f, False) for s in SHAPES for f in FLAGS] + [(2, 2, 72, "half", 4, True), (1, 2, 296, "third", 5, True)]


@pytest.fixture(scope="module")
def ops():
    from multi_modal_foundation_model_amd import _lib as L, ops as K
    L.check(L.lib().mmfm_device_check(0), "device_check")
    return K


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def bf(t):
    return t.to(torch.bfloat16)


def close(a, b, rtol, atol, msg):
    a, b = a.float().cpu(), b.float().cpu()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{msg}: max abs err {(a - b).abs().max().item():.3e} (ref max {b.abs().max().item():.3e})"


def close_bf16(a, b, msg, tol):
    a, b = a.float().cpu(), b.float().cpu()
    err, scale = (a - b).abs().max().item(), b.abs().max().item() + 1e-6
    assert err <= tol * scale, f"{msg}: max abs err {err:.3e} vs scale {scale:.3e}"


def _mod_id(L, recipe):
    a = torch.arange(L)
    return {"half": a >= L // 2, "mod3": a % 3, "third": a * 3 // L}[recipe].to(torch.uint8)


def _run(ops, B, heads, L, recipe, flags, headpad, p):
    from multi_modal_foundation_model_amd import _lib as Lb
    H = heads * DH
    q = bf(rnd(B * L, H, seed=1))
    kv = rnd(B * L, 2 * H, seed=2)
    kv.view(B, L, 2 * H)[:, (3 * L) // 4:, :H] *= 6.0            # late queries exceed the first key tile's reference exponent
    kv = bf(kv)
    d_o = bf(rnd(B * L, H, seed=3))
    kp = torch.ones(B, L, dtype=torch.uint8)
    kp[0, L - 3:] = 0
    kp[B - 1, 5:9] = 0
    if headpad:                                                  # no allowed key in the first key tile of sample 0's modality-0 queries
        kp[0, :40] = 0
    kp, mi = kp.cuda(), _mod_id(L, recipe).cuda()
    kpb = kp.bool()
    allowed = torch.tril(torch.ones(L, L, dtype=torch.bool, device="cuda"))[None].expand(B, L, L) if flags & 2 else kpb[:, None, :].expand(B, L, L)
    if flags & 1:
        allowed = allowed | torch.eye(L, dtype=torch.bool, device="cuda")[None]
    if flags & 4:
        allowed = allowed | (mi[None, :, None] != mi[None, None, :])
    assert bool(allowed.any(-1).all())
    o, lse = torch.empty(B * L, H, device="cuda", dtype=torch.bfloat16), torch.empty(B, heads, L, device="cuda")
    dq, dkv = torch.full_like(q, float("nan")), torch.full_like(kv, float("nan"))
    # the workspace (zeroed: only the keep-bit kernels write it) selects the dh = 64 pair, with or without dropout
    kb = torch.zeros(ops.attn_keepbits_bytes(B, heads, L, L), dtype=torch.uint8, device="cuda")
    kw = dict(keepbits=kb)
    if p > 0:
        state = torch.zeros(2, dtype=torch.int32, device="cuda")
        ops.rng_seed(state, 4321)
        kw["drop_p"] = ops.dropout(state, 7, p)
    desc = ops.attn_desc(Lb.BF16, B, heads, L, L, DH, q.data_ptr(), kv.data_ptr(), kv.data_ptr() + H * 2, H, 2 * H, 2 * H, o.data_ptr(), H, lse,
                         kp, mi, flags, DH ** -0.5, d_o=d_o.data_ptr(), lddo=H, dq=dq.data_ptr(), dk=dkv.data_ptr(), dv=dkv.data_ptr() + H * 2,
                         lddq=H, lddk=2 * H, lddv=2 * H, **kw)
    for backward in (False, True):                               # the family this file is about, in both directions
        assert ops.attn_family(desc, backward) == Lb.ATTN_FAMILY_KEEPBIT_LONG
    ops.attn_fwd(desc)
    am = allowed[:, None].expand(B, heads, L, L)
    keep, keep_p = None, 1.0
    if p > 0:
        keep = DR.unpack_keepbits(kb, B, heads, L, L).cuda()
        keep_p = ops.attn_keep_prob(p)
        assert abs(keep_p - (1 - p)) <= 2 ** -11
        n = int(am.sum().item())
        rate = keep[am].float().mean().item()                   # bits of elements that are not allowed are unspecified
        print(f"keep rate over {n} allowed elements: {rate:.5f} (keep {keep_p:.5f})")
        assert abs(rate - keep_p) < 5 * math.sqrt(p * (1 - p) / n) + 1e-4, f"keep rate {rate}"
    ops.attn_bwd(desc)
    qr, kvr = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    Q = qr.view(B, L, heads, DH).transpose(1, 2)
    K_, V_ = [t.view(B, L, heads, DH).transpose(1, 2) for t in kvr.split(H, dim=1)]
    s = ((Q @ K_.transpose(-1, -2)) * DH ** -0.5).masked_fill(~am, float("-inf"))
    P = torch.softmax(s, -1)
    if flags & 2:                                                # CAUSAL replaces the key padding: a padded key is attended to
        assert bool((P.detach()[(~kpb)[:, None, None, :].expand(B, heads, L, L)] > 0).any())
    Pk = P if keep is None else P * (keep & am).float() / keep_p
    oref = (Pk @ V_).transpose(1, 2).reshape(B * L, H)
    close_bf16(o, oref, "masked attn fwd", tol=2e-2)
    close(lse, torch.logsumexp(s, -1), rtol=1e-3, atol=2e-3, msg="masked attn lse")
    oref.backward(d_o.float())
    close_bf16(dq, qr.grad, "masked attn dq", tol=3e-2)
    close_bf16(dkv[:, :H], kvr.grad[:, :H], "masked attn dk", tol=3e-2)
    close_bf16(dkv[:, H:], kvr.grad[:, H:], "masked attn dv", tol=3e-2)


@pytest.mark.parametrize("B,heads,L,recipe,flags,headpad", CASES)
def test_attention_long_masks_with_dropout(ops, B, heads, L, recipe, flags, headpad):
    """drop_p = 0.4 through the keep-bit workspace: the workspace is zeroed, the forward fills it, the keep mask read back out of the
    bit tiles has the keep rate over the allowed elements (5 sigma), and o / lse / dq / dk / dv match softmax -> keep / keep_p -> P.V
    and its autograd (forward 2e-2, lse rtol 1e-3 / atol 2e-3, gradients 3e-2 of the tensor's scale: bf16 has 8 significant bits)."""
    _run(ops, B, heads, L, recipe, flags, headpad, 0.4)


@pytest.mark.parametrize("B,heads,L,recipe,flags,headpad", CASES)
def test_attention_long_masks_without_dropout(ops, B, heads, L, recipe, flags, headpad):
    """The same shapes and flags without dropout; the workspace is still passed (it selects the pair, and its tail holds the backward's
    delta): correctness only, same tolerances."""
    _run(ops, B, heads, L, recipe, flags, headpad, 0.0)
