"""Dropout masks read off the kernels, and the references they drive.

Every dropout mask of the library is a pure function of (state, site, index): none has to be matched by an RNG, each can be read
back and handed to a plain reference.  The read-out helpers below return the MULTIPLIER tensor a site applies (0, or the kernel's
own survivor scale); `attention_dropout_ref` is the fp64 attention the per-kernel tests compare with, `oracle_dropout_fn` turns the
sites of a built engine plan into the hook of oracle.mm_oracle.forward.

Which hash serves which site (csrc/common.h, csrc/attn_common.h, csrc/rowchain.h, csrc/attention_fast.hip):
  flat counter hash   GEMM epilogue, mmfm_dropout_apply, stitch_bwd and attention drop_o: counter row * N + col (drop_o: N = heads * dh,
                      whatever ldo is); survivor scale 1 / (1 - p) in fp32.
  attention drop_p    general kernels: fp32 compute hashes the counter (bh * Lq + q) * Lk + key, the bf16 MFMA kernels a row key of
                      bh * Lq + q and the key pair; either way a function of (state, site, b, head, q, key, Lq[, Lk]) alone - not of
                      dh, the mask flags, the leading dims or the data - with scale 1 / (1 - p).  Keep-bit kernels: the bits of the
                      workspace, scale 1 / mmfm_attn_keep_prob(p).
  RowDrop             the fused MLP: a key per row, a short mix per feature pair; scale 1 / (1 - p)."""
import numpy as np
import torch


def survivor_scale(p):
    """1.f / (1.f - p) as drop_init (csrc/common.h) computes it."""
    one, pf = torch.tensor(1.0, dtype=torch.float32), torch.tensor(float(p), dtype=torch.float32)
    return float(one / (one - pf))


# ------------------------------------------------------------------------------------ flat counter hash
def flat_multiplier(ops, state, site, p, R, N):
    """[R, N] fp32 multiplier of the flat counter hash at (state, site, p): mmfm_dropout_apply on ones."""
    ones = torch.ones(R, N, device="cuda")
    out = torch.empty_like(ones)
    ops.dropout_apply(ones, out, R, N, ops.dropout(state, site, p))
    return out


# ------------------------------------------------------------------------------------ attention drop_p, keep-bit kernels
def unpack_keepbits(kb, B, heads, Lq, Lk):
    """keep[b, h, q, k] out of the documented bit-tile layout (csrc/attention_fast.hip header): words [bh][qt][kt][32], word 2 r + kh
    of a tile = key 32 kt + (r & 3) + 8 (r >> 2) + 4 kh, bit j = query 32 qt + j."""
    nqt, nkt = (Lq + 31) // 32, (Lk + 31) // 32
    w = kb[:B * heads * nqt * nkt * 128].view(torch.int32).view(B * heads, nqt, nkt, 32).cpu().numpy().astype(np.uint32)      # (behind the tiles: scratch)
    bits = ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)          # [bh, qt, kt, word, qbit]
    widx = np.arange(32)
    key_of_word = ((widx >> 1) & 3) + 8 * (widx >> 3) + 4 * (widx & 1)
    keep = np.zeros((B * heads, nqt * 32, nkt * 32), dtype=bool)
    for qt in range(nqt):
        for kt in range(nkt):
            keep[:, 32 * qt:32 * qt + 32, 32 * kt + key_of_word] = bits[:, qt, kt].transpose(0, 2, 1)
    return torch.from_numpy(keep[:, :Lq, :Lk]).view(B, heads, Lq, Lk)


def extract_attn_keep_mask(ops, state, site, p, B, heads, Lq, Lk):
    """keep[b, h, q, k] of the attention-probability dropout at (state, site), read off the kernel itself: the decisions depend on
    (state, site, b, head, query, key) only, not on the data, so with q = k = 0 (uniform probabilities 1 / Lk) and a one-hot V block
    (V[k, d] = 1 iff k == 32 blk + d) the forward output is keep(q, 32 blk + d) / (Lk (1 - p)): ceil(Lk / 32) launches show every key."""
    from multi_modal_foundation_model_amd import _lib as Lb
    dh = 32
    H = heads * dh
    q = torch.zeros(B * Lq, H, device="cuda", dtype=torch.bfloat16)
    kp = torch.ones(B, Lk, dtype=torch.uint8, device="cuda")
    keep = torch.zeros(B, heads, Lq, Lk, dtype=torch.bool, device="cuda")
    kb = torch.empty(ops.attn_keepbits_bytes(B, heads, Lq, Lk), dtype=torch.uint8, device="cuda")
    for blk in range((Lk + 31) // 32):
        kv = torch.zeros(B, Lk, 2, heads, dh, device="cuda", dtype=torch.bfloat16)
        n = min(32, Lk - 32 * blk)
        kv[:, 32 * blk + torch.arange(n), 1, :, torch.arange(n)] = 1.0
        kv = kv.view(B * Lk, 2 * H)
        o, lse = torch.empty(B * Lq, H, device="cuda", dtype=torch.bfloat16), torch.empty(B, heads, Lq, device="cuda")
        desc = ops.attn_desc(Lb.BF16, B, heads, Lq, Lk, dh, q.data_ptr(), kv.data_ptr(), kv.data_ptr() + H * 2, H, 2 * H, 2 * H, o.data_ptr(), H, lse,
                             kp, None, 0, dh ** -0.5, drop_p=ops.dropout(state, site, p), keepbits=kb)
        ops.attn_fwd(desc)
        keep[:, :, :, 32 * blk:32 * blk + n] = (o.view(B, Lq, heads, dh).permute(0, 2, 1, 3)[..., :n] != 0)
    return keep


def keepbit_multiplier(ops, kb, p, B, heads, Lq, Lk):
    """[B, heads, Lq, Lk] fp32 multiplier of drop_p on the keep-bit kernels, from the workspace the forward left (bits of elements the
    mask rule does not allow are unspecified: their probability is zero anyway)."""
    return unpack_keepbits(kb, B, heads, Lq, Lk).float().cuda() / ops.attn_keep_prob(p)


# ------------------------------------------------------------------------------------ attention drop_p, general kernels
def general_attn_multiplier(ops, state, site, p, dtype, dh, B, heads, Lq, Lk):
    """[B, heads, Lq, Lk] fp32 multiplier of drop_p on the general kernels (attention.hip in fp32, attention_bf16.hip without the
    keep-bit workspace): the one-hot-V read-out of extract_attn_keep_mask at the launch's own dtype, dh, B, heads, Lq and Lk (so the
    dispatch picks the same kernel family), drop_o off, no mask flags, no padded keys - the decisions depend on none of them (module
    docstring) - ceil(Lk / dh) launches of dh keys each."""
    from multi_modal_foundation_model_amd import _lib as Lb
    H = heads * dh
    code, es = (Lb.F32, 4) if dtype == torch.float32 else (Lb.BF16, 2)
    q = torch.zeros(B * Lq, H, device="cuda", dtype=dtype)
    kp = torch.ones(B, Lk, dtype=torch.uint8, device="cuda")
    keep = torch.zeros(B, heads, Lq, Lk, dtype=torch.bool, device="cuda")
    for blk in range((Lk + dh - 1) // dh):
        kv = torch.zeros(B, Lk, 2, heads, dh, device="cuda", dtype=dtype)
        n = min(dh, Lk - dh * blk)
        kv[:, dh * blk + torch.arange(n), 1, :, torch.arange(n)] = 1.0
        kv = kv.view(B * Lk, 2 * H)
        o, lse = torch.empty(B * Lq, H, device="cuda", dtype=dtype), torch.empty(B, heads, Lq, device="cuda")
        desc = ops.attn_desc(code, B, heads, Lq, Lk, dh, q.data_ptr(), kv.data_ptr(), kv.data_ptr() + H * es, H, 2 * H, 2 * H, o.data_ptr(), H, lse,
                             kp, None, 0, dh ** -0.5, drop_p=ops.dropout(state, site, p))
        ops.attn_fwd(desc)
        keep[:, :, :, dh * blk:dh * blk + n] = (o.view(B, Lq, heads, dh).permute(0, 2, 1, 3)[..., :n] != 0)
    return keep.float() * survivor_scale(p)


# ------------------------------------------------------------------------------------ RowDrop (fused MLP)
def rowdrop_multiplier(ops, state, site, p, R):
    """[R, 256] fp32 multiplier of the fused MLP's row-keyed hash: the front half of mmfm_mlp_bwd with dy = 1 gives t1 = dropout'(1),
    whatever the other operands hold (zeros here).  t1 is bf16: only its zero pattern is read, the scale is the fp32 one the
    forward applies to its accumulator."""
    BF = torch.bfloat16
    z = lambda *s, dt=BF: torch.zeros(*s, device="cuda", dtype=dt)
    dy = torch.ones(R, 256, device="cuda", dtype=BF)
    t1, g, du = z(R, 256), z(R, 512), z(R, 512)
    ops.mlp_bwd(ops.mlp_desc(R, w_up=z(512, 256), b_up=z(512, dt=torch.float32), drop=ops.dropout(state, site, p), xhat=z(R, 256), dy=dy,
                             w_down_t=z(512, 256), t1=t1, g=g, du=du, dx=None))
    return (t1 != 0).float() * survivor_scale(p)


# ------------------------------------------------------------------------------------ fp64 attention with given masks
def allowed_mask(keypad, flags, Lq, mod_id=None):
    """allowed[b, q, k] of include/mmfm.h: (DIAG && q == k) | (CAUSAL ? k <= q : keypad[b][k]) | (SEP && mod_id[q] != mod_id[k])."""
    B, Lk = keypad.shape
    dev = keypad.device
    if flags & 2:
        m = torch.tril(torch.ones(Lq, Lk, dtype=torch.bool, device=dev))[None].expand(B, Lq, Lk)
    else:
        m = keypad.bool()[:, None, :].expand(B, Lq, Lk)
    if flags & 1:
        m = m | torch.eye(Lq, Lk, dtype=torch.bool, device=dev)[None]
    if flags & 4:
        m = m | (mod_id[None, :Lq, None] != mod_id[None, None, :Lk])
    return m


def attention_dropout_ref(q, k, v, allowed, scale, mult_p=None, mult_o=None):
    """softmax -> drop_p multiplier -> P V -> drop_o multiplier, in the dtype of its inputs (the tests pass fp64 leaves that require
    grad: autograd then gives dq, dk, dv for a d_o taken AFTER drop_o, include/mmfm.h).
    q [B, heads, Lq, dh], k / v [B, heads, Lk, dh], allowed bool [B, Lq, Lk], mult_p [B, heads, Lq, Lk], mult_o [B * Lq, heads * dh].
    Returns o [B * Lq, heads * dh] and lse [B, heads, Lq]."""
    B, heads, Lq, dh = q.shape
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~allowed[:, None], float("-inf"))
    P = torch.softmax(s, -1)
    if mult_p is not None:
        P = P * mult_p.to(P.dtype)
    o = (P @ v).transpose(1, 2).reshape(B * Lq, heads * dh)
    if mult_o is not None:
        o = o * mult_o.to(o.dtype)
    return o, torch.logsumexp(s, -1)


# ------------------------------------------------------------------------------------ a whole step's masks -> the oracle's hook
def attn_site_descs(engine, B, T):
    """{site id: (forward, backward) mmfm_attn_desc the built training plan of batch shape (B, T) launches at that attention drop_p site}."""
    plan = engine.plans[(B, T, True, True)]
    by_site = lambda entries, name: {keep[0].drop_p.site: keep[0] for fn, _, keep in entries if fn.__name__ == name and keep[0].drop_p.p > 0}
    fwd = by_site(plan["fwd"], "mmfm_attn_fwd")
    bwd = by_site([e for _, seg in plan["bwd"] for e in seg], "mmfm_attn_bwd")
    assert set(fwd) == set(bwd)
    return {site: (fwd[site], bwd[site]) for site in fwd}


def on_keepbit_kernels(fwd_desc, bwd_desc=None):
    """Whether the launch of `fwd_desc` draws drop_p from the keep-bit workspace: the library's own answer (ops.attn_family), and the
    same answer for the backward's descriptor - or the pair would be split."""
    from multi_modal_foundation_model_amd import _lib as Lb, ops
    fam = ops.attn_family(fwd_desc)
    assert bwd_desc is None or ops.attn_family(bwd_desc, backward=True) & Lb.ATTN_FAMILY_MASK == fam
    return fam in Lb.ATTN_KEEPBIT_FAMILIES


def collect_step_multipliers(ops, engine, B, T):
    """{site key: multiplier (fp64, on the GPU, in the shape the oracle's tensor has at that site)} of the training step the engine just ran
    at batch shape (B, T): engine.rng still holds the state that step used, engine.dropout_sites names id, p, kind and shape, and the
    keep-bit sites are read from the engine's own workspaces."""
    out = {}
    M = len(engine.cfg.mods)
    descs = attn_site_descs(engine, B, T)
    for s in engine.dropout_sites(B, T):
        key, site, p = s["key"], s["site"], s["p"]
        if s["kind"] == "flat":
            R, N = s["shape"]
            m = flat_multiplier(ops, engine.rng, site, p, R, N)
        elif s["kind"] == "rowdrop":
            R, N = s["shape"]
            assert N == 256
            m = rowdrop_multiplier(ops, engine.rng, site, p, R)
        else:
            Bq, heads, Lq, Lk = s["shape"]
            if on_keepbit_kernels(*descs[site]):
                assert s["keepbits"] is not None
                m = keepbit_multiplier(ops, s["keepbits"], p, Bq, heads, Lq, Lk)
            else:
                m = general_attn_multiplier(ops, engine.rng, site, p, engine.adt, s["dh"], Bq, heads, Lq, Lk)
        if s["kind"] != "attn":
            m = m.view(B, -1, m.shape[-1])          # [B, T or M T, H]
        out[key] = m.double()
    assert len(out) == len(engine._sites) and M > 0
    return out


def oracle_dropout_fn(mults, used=None):
    """The `dropout_fn` of oracle.mm_oracle.forward that replays `mults` ({site key: multiplier}); `used` (a set) records the keys asked for."""
    def fn(key, x):
        m = mults[key]
        assert tuple(m.shape) == tuple(x.shape), (key, tuple(m.shape), tuple(x.shape))
        if used is not None:
            used.add(key)
        return m.to(x.dtype)
    return fn
