"""fp64 references for the modality-segment kernels (MMFM_MOD_SEGMENTS in include/mmfm.h): mask preparation, stitch and the
de-stitching LayerNorm over modalities of different length, each with its own time stamps and attention mask.

Every reference is the uniform one of tests/edge_refs.py applied per slot and concatenated: slot j of the stitched sequence is
the T_j positions from off_j = sum_{i<j} T_i, so a slot on its own is the uniform case with M = 1 on its slice of the sequence.
Nothing is restated here but the segment arithmetic (offsets, the de-stitch permutation); the bounds are edge_refs' own.
tests/test_mod_segments_refs_cpu.py proves these against nn.Embedding autograd, against edge_refs at equal lengths and against
the boolean gather upstream de-stitches with; tests/test_mod_segments_kernels_gpu.py compares the HIP kernels with them."""
import torch

import edge_refs as E


def offsets(Ts):
    """[off_0 .. off_M]: off_j = sum of the lengths in front of slot j, off_M = L."""
    off = [0]
    for t in Ts:
        off.append(off[-1] + int(t))
    return off


def mod_mask(Ts, device=None):
    """mm.py:102 for segments: position l of the stitched sequence belongs to slot mod_mask[l]."""
    return torch.repeat_interleave(torch.arange(len(Ts), device=device), torch.tensor([int(t) for t in Ts], device=device))


def mask_prep(masks, strides, attns, channels):
    """edge_refs.mask_prep per slot (its own attention mask attns[j], [B, T_j]), concatenated along the token axis.
    Returns tokmask, keypad [B, L] u8, keep0, mod_id [L] u8 and count [M] int64."""
    parts = [E.mask_prep([mk], [s], a, [c]) for mk, s, a, c in zip(masks, strides, attns, channels)]
    tokmask, keypad = (torch.cat([p[i] for p in parts], 1) for i in (0, 1))
    keep0 = torch.cat([p[2] for p in parts])
    mod_id = torch.cat([torch.full_like(p[3], j) for j, p in enumerate(parts)])
    return tokmask, keypad, keep0, mod_id, torch.cat([p[4] for p in parts])


def stitch_fwd(tok, mod_row, pos, ts, keep0, off, max_F):
    """edge_refs.stitch_fwd for the slot of T = ts.shape[1] bins at offset off: (x, emb, mag), each [B, T, H], the slice
    [:, off:off + T] of the [B, L, H] outputs."""
    T = ts.shape[1]
    return E.stitch_fwd(tok, mod_row, pos, ts, keep0[off:off + T], 0, max_F)


def stitch_bwd(dx, dextra, ts, keep0, keep, p, off, max_F):
    """edge_refs.stitch_bwd for the slot at offset off: dx / dextra are the whole [B, L, H] gradients, keep0 the whole [L]."""
    T = ts.shape[1]
    return E.stitch_bwd(dx[:, off:off + T], None if dextra is None else dextra[:, off:off + T], ts, keep0[off:off + T], keep, p, 0, max_F)


def destitch_perm(R, Ts, device=None):
    """Row r = b*L + off_j + t of the stitched [B, L, H] sequence -> row B*off_j + b*T_j + t: one contiguous [B*T_j][H] block per
    slot, slot j's at row B*off_j (decoder_embeddings.py:105-107 gathers y[mod_mask == j])."""
    off = offsets(Ts)
    L = off[-1]
    assert R % L == 0
    B = R // L
    r = torch.arange(R, device=device)
    b, l = r // L, r % L
    j = mod_mask(Ts, device)[l]
    o, T = torch.tensor(off[:-1], device=device)[j], torch.tensor([int(t) for t in Ts], device=device)[j]
    return B * o + b * T + (l - o)


def layernorm_fwd(x, gamma, beta, Ts, eps=1e-5):
    """edge_refs.layernorm_fwd with y's rows in the segment de-stitched order.  Returns (y, mean, rstd)."""
    y, mu, rstd = E.layernorm_fwd(x, gamma, beta, eps)
    out = torch.empty_like(y)
    out[destitch_perm(x.shape[0], Ts, x.device)] = y
    return out, mu, rstd


def layernorm_bwd(dy, x, gamma, dres, Ts, eps=1e-5):
    """edge_refs.layernorm_bwd with dy's rows in the segment de-stitched order (the same dict)."""
    return E.layernorm_bwd(dy[destitch_perm(x.shape[0], Ts, x.device)], x, gamma, dres, eps)
